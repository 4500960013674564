"""The fused 4096 kernel's Rice search without a GPU: the window proof as a search for violations, and the lane model of
tests/rice_scatter_model.py -- window, path predicate, tagged entries, the two scatter steps, the quad layout, the level
totals -- against oracle.find_partitioned_rice_parameter on order, parameters and code bits."""
import numpy as np
import pytest

import rice_scatter_model as rsm
from oracle import oracle as orc

N = 4096


# ---- the window [p0 - 1, p0 + 1] of one partition (or merged group) ---------------------------------------------------
def _partition_batch(rng, count, kind):
    """(count, 256) codes, zero beyond each row's length, and the lengths (52 .. 256)."""
    length = rng.integers(52, 257, count)
    live = np.arange(256)[None, :] < length[:, None]
    top = rng.integers(0, 26, count)  # codes up to 2^25
    amp = (np.int64(1) << top)[:, None]
    if kind == "uniform":
        u = rng.integers(0, 2 ** 62, (count, 256)) % (amp + 1)
    elif kind == "impulses":
        u = np.where(rng.random((count, 256)) < rng.random((count, 1)) * 0.1, amp, 0)
    elif kind == "constant":
        u = np.broadcast_to(rng.integers(0, 2 ** 62, (count, 1)) % (amp + 1), (count, 256))
    elif kind == "geometric":
        u = np.minimum(rng.geometric(1.0 / (1.0 + amp * rng.random((count, 1))), (count, 256)) - 1, amp)
    else:  # laplace
        u = np.minimum(np.abs(rng.laplace(0.0, 1.0, (count, 256)) * amp * rng.random((count, 1)) / 8).astype(np.int64), amp)
    return np.where(live, u, 0).astype(np.uint32), length


@pytest.mark.parametrize("kind", ["uniform", "impulses", "constant", "geometric", "laplace"])
def test_window_has_no_violation(kind):
    """200 000 partitions over the five families: no parameter p <= p0 - 2 and none > p0 + 1 wins or ties, so the first
    minimum of the unclamped table lies in {p0 - 1, p0, p0 + 1}."""
    rng = np.random.default_rng(0x51CE0000 + len(kind))
    for _ in range(4):
        u, length = _partition_batch(rng, 10000, kind)
        s = u.sum(axis=1, dtype=np.uint64)
        p0 = rsm._floor_log2(s // length.astype(np.uint64) + np.uint64(1))  # floor(log2(m + 1)) = floor(log2(floor(m) + 1))
        table = np.stack([(u >> np.uint32(p)).sum(axis=1, dtype=np.int64) + length * (p + 1) + 4 for p in range(32)], axis=1)
        first = table.argmin(axis=1)
        assert (np.abs(first - p0) <= 1).all()
        best = table.min(axis=1)
        p = np.arange(32)[None, :]
        outside = (p <= p0[:, None] - 2) | (p > p0[:, None] + 1)
        assert (table[outside] > np.broadcast_to(best[:, None], table.shape)[outside]).all()


# ---- residual blocks ---------------------------------------------------------------------------------------------------
WARMS = (1, 8, 12, 0, 2, 4, 10)


def _blocks(rng, count):
    """Residual blocks of every class the search distinguishes (see test_model_matches_oracle)."""
    out = np.zeros((count, N), np.int32)
    kind = rng.integers(0, 8, count)
    for b in range(count):
        k = kind[b]
        if k == 0:  # white noise at amplitude 2^1 .. 2^15: means share one or two binades
            a = 1 << rng.integers(1, 16)
            out[b] = rng.integers(-a, a + 1, N)
        elif k == 1:  # Laplace residuals, what a predictor leaves
            out[b] = np.rint(rng.laplace(0.0, 2.0 ** rng.uniform(0, 12), N))
        elif k == 2:  # amplitude steps x2, x4 or x64 between partitions: windows of 4, 5 and more
            step = (2, 4, 64)[rng.integers(0, 3)]
            a = (1 << rng.integers(0, 8)) * np.where(rng.random(64) < 0.5, 1, step)
            out[b] = (rng.integers(-1000, 1001, (64, 64)) * a[:, None] // 1000).reshape(N)
        elif k == 3:  # silence with sparse impulses
            hit = rng.random(N) < 2.0 ** -rng.integers(3, 10)
            out[b] = np.where(hit, rng.integers(-(1 << rng.integers(1, 20)), 1 << 10, N), 0)
        elif k == 4:  # |s| <= 1: rich in ties
            out[b] = rng.integers(-1, 2, N) * (rng.random(N) < rng.random())
        elif k == 5:  # constants and zeros
            out[b] = rng.integers(-3, 4)
        elif k == 6:  # periodic in the partition length: equal tables, equal totals across orders
            out[b] = np.tile(rng.integers(-2, 3, 64 << rng.integers(0, 3)), N)[:N]
        else:  # full-scale material
            out[b] = rng.integers(-(1 << 24), 1 << 24, N)
    return out


@pytest.fixture(scope="module")
def classified():
    """20 160 blocks through the model and the oracle, once: per (warm, configured limit) batch."""
    rng = np.random.default_rng(0x51CE5CA7)
    rows = []
    for warm in WARMS:
        for max_rice in (30, 30, 30, 30, 13, 3):
            blocks = _blocks(rng, 480)
            if warm in (1, 8, 12):  # lane 0 decides the upper end: a loud first partition, quiet elsewhere
                blocks[:40, 64:] >>= 3
            blocks[:, :warm] = 0
            got = rsm.search(blocks, warm, max_rice)
            for b in range(len(blocks)):
                order, ps, code_bits, _ = orc.find_partitioned_rice_parameter(blocks[b], warm, max_rice)
                rows.append((warm, max_rice, got[b], order, ps, code_bits))
    return rows


def test_model_matches_oracle(classified):
    assert len(classified) >= 20000
    for warm, max_rice, got, order, ps, code_bits in classified:
        assert got["order"] == order, (warm, max_rice, got["fast"], got["width"])
        assert got["params"].tolist() == ps.tolist(), (warm, max_rice, got["fast"], got["width"])
        assert got["code_bits"] == code_bits


def test_every_class_is_drawn(classified):
    fast = [r for r in classified if r[2]["fast"]]
    slow = [r for r in classified if not r[2]["fast"]]
    assert any(r[2]["width"] == 3 for r in fast), "window 3 wide"
    assert any(r[2]["width"] == 4 for r in fast), "window 4 wide"
    assert any(r[2]["width"] > 4 for r in slow), "window wider than 4 (fallback)"
    assert any(r[2]["p0min"] < 2 for r in fast), "p0min < 2"
    assert any(r[2]["param_tie"] for r in fast), "a tie between two parameters at the chosen level"
    assert any(r[2]["order_tie"] for r in fast), "a tie between two orders"
    for warm in (1, 8, 12):
        assert any(r[0] == warm for r in fast) and any(r[0] == warm for r in slow), warm
    assert any(r[1] < 30 for r in slow), "a configured limit below the bit length"


def test_fast_path_layout(classified):
    """pk[K] is valid on every lane that is a multiple of 2^K, and replicated over the quad from level 2 on."""
    for warm, max_rice, got, order, ps, code_bits in classified[::97]:
        if not got["fast"]:
            continue
        pk = got["pk"]
        for K in range(2, 7):
            lead = pk[K].reshape(-1, 4)[:: max(1, (1 << K) // 4)]
            assert (lead == lead[:, :1]).all()
