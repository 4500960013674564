"""tests/direct_mse_cases.py held to itself, to the oracle and to the mathematics, without a GPU.

  * the table covers what it must: every kernel template instantiation launch_direct_mse can select, every LW of the
    batched solve, every order edge, every window edge; every case reaches the form it names; the regulariser is reached
    0, 1-3 and 4 and more doublings deep; the 25-bit side row needs its 25th bit;
  * the oracle's status and record are well-formed on every case and its residual decodes to the samples;
  * the oracle's unquantised solution solves the covariance method's system built in exact integer arithmetic straight
    from src/lpc.rs:533-548, :573-600, :853-883 -- so the estimator is pinned to the mathematics, not only to the
    oracle's own restatement; what stays unpinned is bit-equality with nalgebra's Cholesky itself;
  * IRLS never answers a solution worse (in sum of |error|) than its first step's.
"""
import re
import os

import numpy as np
import pytest

import direct_mse_cases as dc
from oracle import oracle as orc

U = 2.0 ** -53


def ocfg(order, steps=0, window=dc.RECT):
    return orc.make_config(lpc_order=order, window=window, use_direct_mse=True, mae_optimization_steps=steps)


def bound(n, P):
    """The backward-error bound of test_oracle_solves_the_exact_system: 2^-4 (n + P^2) 2^-53.

    Shape: an entry of G or r is a chain of at most n fma roundings (error <= n u relative to the sum of |terms|, which
    the norm of G bounds), Cholesky and the two triangular solves add O(P^2) u (Higham, Accuracy and Stability, thm
    10.4).  Constant: measured on the well-conditioned families (music and full-range noise at 16 and 24 bits, orders 8,
    12, 32, n = 256, 1152, 4096, two seeds each: 72 systems) the largest backward error is 59.4 u = 0.0481 (n + P^2) u
    (24-bit noise, n = 1152, order 8; 16-bit material stays below 1.5 u because its sums are exact integers below
    2^53); the smallest power of two that covers 0.0481 is 2^-4.  The two mutants sit between 1.5e-6 and 6.9e-3, the
    bound between 2.2e-15 and 3.6e-14."""
    return 2.0 ** -4 * (n + P * P) * U


# ------------------------------------------------------------------------------------------------------ the table
def test_the_table_covers_what_it_must():
    gpu = dc.GPU_CASES
    forms = [dc.case_form(c) for c in gpu]
    named = set().union(*[f["kernels"] for f in forms])
    assert dc.selectable_kernels() <= named, sorted(dc.selectable_kernels() - named)
    assert len(dc.selectable_kernels()) == 23
    one_kernel = {k for k in named if k.startswith("direct_mse_kernel<")}
    assert len(one_kernel) == 6, one_kernel
    assert {f["lw"] for f in forms if f["lw"]} == {64, 32, 16, 8, 4}
    assert {f["block_rows"] for f in forms} >= {1, 2, 3, 4, 7, 8, 9}           # (P + 4) >> 2 on either side of 3|4, 7|8
    # order edges, with and without IRLS steps
    host = [c for c in gpu if c.layout == "host" and c.entry == "qlpc"]
    for order in dc.ORDERS:
        assert any(c.order == order and c.steps == 0 and len(c.rows) >= 11 for c in host), order
    for order in dc.IRLS_ORDERS:
        assert {c.steps for c in host if c.order == order and len(c.rows) >= 11} >= {0, 1, 3}, order
    # window edges: chain lengths at one order of each form (1 and 2 cannot launch: the module docstring), blocks with IRLS
    for order in dc.FORM_ORDERS:
        lengths = {c.n - c.order for c in dc.CASES if c.order == order}
        assert lengths >= set(dc.CHAIN_LENGTHS), (order, lengths)
        launched = {c.n - c.order for c in gpu if c.order == order}
        assert launched >= {511, 512, 513, 1024, 1025}, order
        assert {c.n for c in gpu if c.order == order and c.steps > 0} >= set(dc.IRLS_BLOCKS), order
    assert {(c.n, c.order) for c in dc.CASES if c.n <= c.order} == {(8, 8), (5, 8)}
    # every device layout on every device entry point's list, every entry point once
    dev = [c for c in gpu if c.layout != "host"]
    assert {c.layout for c in dev} == set(dc.DEVICE_LAYOUTS)
    assert {c.entry for c in dev} == {"qlpc", "stereo_qlpc", "stereo_frames", "frames3"}
    assert all(not dc.is_aligned(c) for c in dev)
    # sizes
    for c in gpu:
        small = c.n <= 4096 and len(c.rows) <= 12
        assert small or c.name.startswith("solve ") or "wg" in c.name, c.name
    assert len({c.name for c in dc.CASES}) == len(dc.CASES)


def test_every_case_reaches_the_form_it_names():
    for c in dc.CASES:
        f = dc.case_form(c)
        assert f["name"] == c.claim, c.name
        assert f["weighted"] == (c.steps > 0)
    # the claims, spelled out for the cases that exist for one
    want = {"order 11": "small", "order 12": "tiles", "order 31": "tiles", "order 32": "blocks",
            "order 32 irls 3": "blocks+w", "one-kernel mono": "one-kernel", "one-kernel stereo irls": "one-kernel+w",
            "one-kernel wg mono": "one-kernel-wg+w", "one-kernel wg stereo": "one-kernel-wg+w"}
    for name, claim in want.items():
        assert dc.by_name(name).claim == claim, name
    assert dc.case_form(dc.by_name("one-kernel wg mono"))["kernels"] == {"direct_mse_kernel<false, true, true>"}
    assert dc.case_form(dc.by_name("one-kernel wg stereo"))["kernels"] == {"direct_mse_kernel<true, true, true>"}
    for order, lw in ((8, 64), (10, 64), (11, 32), (12, 32), (15, 32), (16, 16), (21, 16), (22, 8), (24, 8), (31, 8),
                      (32, 4)):
        assert dc.solve_lanes(order) == lw, order
    for c in dc.CASES:                                                 # the seams of the batched solve
        if c.name.startswith("solve ") and c.entry == "qlpc":
            lw = dc.solve_lanes(c.order)
            assert len(c.rows) in (lw + 1, 2 * lw + 3) and len(set(c.rows)) == len(c.rows), c.name
            for s, at in enumerate(range(lw, len(c.rows), lw)):
                kinds = [r.startswith("music") for r in (c.rows[at - 1], c.rows[at])]
                assert kinds == ([True, False] if s % 2 else [False, True]), (c.name, at)
    arrangements = {(len(c.rows) > dc.solve_lanes(c.order) + 1) for c in dc.CASES if c.name.startswith("solve ")}
    assert arrangements == {False, True}


def test_the_table_of_forms_states_the_launcher():
    """The constants and comparisons form() restates are the ones in csrc/direct_mse.cpp."""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "flacenc_rs_amd", "csrc", "direct_mse.cpp")
    src = open(path).read()
    launcher = src[src.index("hipError_t launch_direct_mse"):]
    assert "constexpr int kStreamPiece = %d;" % dc.STREAM_PIECE in src
    assert "constexpr int kErrChunk = %d;" % dc.ERR_CHUNK in src
    assert "a.block_size > %du" % dc.WG_ABOVE in launcher
    assert "per * (size_t)lw > 64 * 1024" in launcher and "int lw = 64;" in launcher
    assert "d.lpc_order <= 11" in launcher and "d.lpc_order <= 31" in launcher
    assert "(reinterpret_cast<uintptr_t>(a.samples) & 15) == 0 && (a.stride & 3) == 0" in launcher
    # every instantiation the table can name is one the launcher spells
    spelled = set()
    for st, wt in re.findall(r"direct_mse_stream_small_kernel<(true|false), (true|false)>", launcher):
        spelled.add("direct_mse_stream_small_kernel<%s, %s>" % (st, wt))
    for st, wt in re.findall(r"direct_mse_stream_tiles_kernel<(true|false), (true|false)>", launcher):
        spelled.add("direct_mse_stream_tiles_kernel<%s, %s>" % (st, wt))
    for st, wt in re.findall(r"FLACENC_DM_STREAM_N\((true|false), (true|false)\)", launcher):
        spelled.add("direct_mse_stream_kernel<%s, %s, 4>" % (st, wt))
    for st, ir, wg in re.findall(r"FLACENC_DM_LAUNCH\((true|false), (true|false), \d, (true|false)\)", launcher):
        spelled.add("direct_mse_kernel<%s, %s, %s>" % (st, ir, wg))
    for ph in re.findall(r"FLACENC_DM_SOLVE\((\d)\)", launcher):
        spelled.add("direct_mse_solve_kernel<%s>" % ph)
    for st in re.findall(r"direct_mse_irls_error_kernel<(true|false)>", launcher):
        spelled.add("direct_mse_irls_error_kernel<%s>" % st)
    assert spelled == dc.selectable_kernels(), spelled ^ dc.selectable_kernels()


def test_material_is_what_it_says():
    for bits in (8, 16, 24):
        lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
        for name in dc.EXTREMES:
            x = dc.material(name, 601, bits, 1)
            assert x.min() >= lo and x.max() <= hi and len(x) == 601, (name, bits)
        assert set(dc.material("alternation", 64, bits)) == {lo, hi}
        sq = dc.material("square", 4096, bits)
        assert set(sq) == {lo, hi} and 4096 % (2 * dc.SQUARE_HALF_PERIOD) != 0 and 1152 % (2 * dc.SQUARE_HALF_PERIOD) != 0
        ramp = dc.material("ramp", 601, bits)
        assert ramp[0] == lo and ramp[-1] == hi
        assert np.count_nonzero(dc.material("impulse", 601, bits)) == 1 and dc.material("impulse", 601, bits).min() == lo
        clipped = dc.material("clipped", 601, bits)
        assert (clipped == hi).sum() > 50 and (clipped == lo).sum() > 50
        for name in dc.PAIRS:
            p = dc.stereo_pair(name, 256, bits, 1)
            assert p.shape == (2, 256) and p.min() >= lo and p.max() <= hi
    side = dc.material("side25", 256, 24)
    assert np.abs(side).max() == (1 << 24) - 1 > (1 << 23)              # needs the 25th bit; exact in f32
    assert np.array_equal(side.astype(np.float32).astype(np.int64), side)
    hl = dc.stereo_pair("hi_lo", 64, 24)
    assert int((hl[0] - hl[1]).max()) == (1 << 24) - 1
    inv = dc.stereo_pair("inverted", 64, 24)
    assert np.array_equal(inv[1], -inv[0] - 1) and ((inv[0] + inv[1]) >> 1 == -1).all()


def test_the_regulariser_is_reached_at_every_depth():
    """0 doublings on music and noise, 1-3 on silence and the 8- and 16-bit constants, 4 and more on the 24-bit rows whose
    Gram entries are near 2^58: a load of 1, 2, 4 or 8 is below half an ulp of the diagonal and changes nothing.  The
    deepest reached is 11 (24-bit square wave and ramp at orders 31 and 32, n = 601)."""
    depth = {}
    for name in ("order 8", "order 32", "order 16", "order 12", "side25"):
        c = dc.by_name(name)
        for (x, _), spec in zip(dc.mono_rows(c), c.rows):
            depth[(name, spec.split(":")[0])] = dc.regulariser_steps(x, ocfg(c.order))[0]
    assert depth[("order 8", "music")] == 0 and depth[("order 8", "noise")] == 0 and depth[("order 32", "music")] == 0
    assert depth[("order 16", "zero")] == 1 and depth[("order 12", "const_hi")] == 1
    assert 1 <= depth[("order 12", "alternation")] <= 3
    assert depth[("order 8", "alternation")] >= 4 and depth[("order 8", "ramp")] >= 4
    assert depth[("order 32", "square")] == 11 == max(depth.values())
    assert depth[("side25", "side25")] >= 4
    k, lam = dc.regulariser_steps(dc.material("zero", 64, 16), ocfg(8))
    assert (k, lam) == (1, 1.0)


# ----------------------------------------------------------------------------------------------------- the oracle
@pytest.mark.parametrize("index", range(0, len(dc.CASES), 8))
def test_the_oracle_is_well_formed_and_lossless(index):
    for c in dc.CASES[index:index + 8]:
        cfg = ocfg(c.order, c.steps, c.window)
        for x, bps in dc.mono_rows(c):
            e = orc.estimated_qlpc(x, bps, cfg)
            assert e["status"] == 0, c.name
            assert 1 <= e["order"] <= c.order and 0 <= e["shift"] <= 15 and e["precision"] == 15, c.name
            assert np.isfinite(e["lpc_coefs"]).all() and np.isfinite(e["autocorr"]).all(), c.name
            if c.n <= c.order:                                         # nothing to estimate from: a one-tap zero predictor
                assert e["order"] == 1 and not e["coefs"].any() and not e["autocorr"].any(), c.name
                assert not e["lpc_coefs"].any()
            assert not e["residual"][:e["order"]].any()
            got = orc.decode_lpc(x[:e["order"]], e["coefs"], e["shift"], e["residual"])
            assert np.array_equal(got, x), c.name


# ------------------------------------------------------------------------------------------------ the mathematics
def pinned(x, order, window=dc.RECT, weight=None):
    """The oracle's unquantised solution against the exact system -> backward error."""
    cfg = ocfg(order, 0, window)
    x = np.ascontiguousarray(x, np.int32)
    k, lam = dc.regulariser_steps(x, cfg, weight)
    _, _, a, st = orc.lpc_with_direct_mse(x, cfg, weight)
    assert st == 0
    G, r = dc.exact_system(x, window, order, weight)
    return dc.backward_error(G, r, a, lam), k


@pytest.mark.parametrize("order", [8, 12, 32])
def test_oracle_solves_the_exact_system_on_well_conditioned_material(order):
    """bound(): its shape, the measured maximum and the constant.  Prints every figure before it asserts."""
    for fam in dc.WELL_CONDITIONED:
        for bits in (16, 24):
            for n in (256, 1152, 4096):
                be, k = pinned(dc.material(fam, n, bits, 0), order)
                print("%s %d bits n %d order %d: %.3g u = %.4f (n + P^2) u" % (fam, bits, n, order, be / U,
                                                                              be / U / (n + order * order)))
                assert k == 0 and be <= bound(n, order), (fam, bits, n, order, be / U)


MATH_CASES = [c.name for c in dc.CASES
              if c.name.startswith(("order ", "side25", "short ", "steps 1 ", "steps 2 ", "steps 513 "))]


@pytest.mark.parametrize("name", MATH_CASES)
def test_oracle_solves_the_exact_system_on_every_extreme(name):
    """Rank-deficient rows with the load the reference's loop reaches; the Tukey cases with their f32 windowed samples;
    the cases with IRLS steps with the weights of the first re-weighting (f32, src/lpc.rs:828), through the oracle's
    weighted entry."""
    c = dc.by_name(name)
    for (x, _), spec in zip(dc.mono_rows(c), c.rows):
        weight = None
        if c.steps > 0 and c.n > c.order:
            a0 = orc.lpc_with_direct_mse(x, ocfg(c.order, 0, c.window))[2]
            err = np.abs(orc.compute_raw_errors(x, a0))
            norm = np.float32(np.abs(x.astype(np.int64)).max())
            with np.errstate(divide="ignore", invalid="ignore"):
                wv = np.power(np.maximum(np.maximum(err, np.float32(1.0)) / norm, np.float32(0.01)), np.float32(-1.2))
            weight = np.ones(c.n, np.float32)
            weight[c.order:] = wv[c.order:].astype(np.float32)
        be, k = pinned(x, c.order, c.window, weight)
        assert be <= bound(c.n, c.order), (name, spec, k, be / U)


@pytest.mark.parametrize("order,n", [(8, 256), (8, 4096), (32, 256), (32, 4096), (12, 1152)])
def test_the_bound_rejects_a_shifted_time_range_and_shifted_lags(order, n):
    """A solution of the same system read with G's time range one sample late, and one with r's lags off by one, differ
    from the true one at about 1 / n: far above the bound.  (Replacing bound() by 1.0 makes this test fail: tried.)"""
    x = dc.material("music", n, 16, 0)
    G, r = dc.exact_system(x, dc.RECT, order)
    assert dc.backward_error(G, r, dc.float_solution(G, r), 0) <= bound(n, order)   # the unmutated solver passes
    for mutant in ("time", "lag"):
        Gm, rm = dc.exact_system(x, dc.RECT, order, mutant=mutant)
        am = dc.float_solution(Gm, rm)
        assert dc.backward_error(Gm, rm, am, 0) <= bound(n, order)                  # it does solve its own system
        be = dc.backward_error(G, r, am, 0)
        assert be > 1e4 * bound(n, order), (mutant, be, bound(n, order))
        assert not be <= bound(n, order)


def test_exact_system_on_a_hand_computed_block():
    """n = 4, order 1: r[1] = x1 x0 + x2 x1 + x3 x2 over t = 1..3, G = x0^2 + x1^2 + x2^2 over t = 0..2."""
    G, r = dc.exact_system(np.array([3, -5, 7, 11]), dc.RECT, 1)
    assert r == [3 * -5 + -5 * 7 + 7 * 11] and G == [[9 + 25 + 49]]
    G, r = dc.exact_system(np.array([3, -5, 7, 11]), dc.RECT, 2)
    assert r == [-5 * 7 + 7 * 11, 3 * 7 + -5 * 11]                                   # t = 2, 3
    assert G == [[25 + 49, -15 - 35], [-15 - 35, 9 + 25]]                            # t = 1, 2: x[t] x[t], x[t] x[t-1], ..


# --------------------------------------------------------------------------------------------------------- IRLS
@pytest.mark.parametrize("name", [c.name for c in dc.CASES if c.steps > 0 and c.entry in ("qlpc", "oracle")
                                  and not c.name.startswith("solve ")])
def test_irls_never_answers_worse_than_its_first_step(name):
    """lpc_with_irls_mae keeps the step with the smallest f32 sum of |error| (src/lpc.rs:839-844), and step 0 is the
    unweighted solution.  In float64 the chosen solution's sum may exceed step 0's by the error of the f32 sums
    compared: a chain of n additions is off by at most n 2^-24 of the sum, the margin."""
    c = dc.by_name(name)
    cfg = ocfg(c.order, c.steps, c.window)
    for x, _ in dc.mono_rows(c):
        a0 = orc.lpc_with_direct_mse(x, ocfg(c.order, 0, c.window))[2]
        a, st = orc.lpc_with_irls_mae(x, cfg, c.steps)
        assert st == 0
        s0 = np.abs(orc.compute_raw_errors(x, a0).astype(np.float64)).sum()
        s = np.abs(orc.compute_raw_errors(x, a).astype(np.float64)).sum()
        assert s <= s0 + c.n * 2.0 ** -24 * s0, (name, s, s0)
