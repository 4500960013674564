"""The deterministic corpus of the order-guess suites (tests/test_order_guess_cpu.py through the model alone,
tests/test_gpu_order_guess.py on the GPU): every case names one subframe, its configuration, K, the extra-window list and
the regimes of the rule (include/flacenc_hip.h, FLACENC_HIP_FLAG_ORDER_GUESS) it stands for.  claims(case) asserts each named
regime from tests/guess_model.py, so the corpus cannot go stale and a GPU case proves what it reaches before a byte is
compared.

Regimes:
  wins     the winner is a guess other than (0, P), strictly shorter than (0, P), and it is the exhaustive search's choice
  loses    a guess other than (0, P) is coded and (0, P) still wins
  early    the chain of window 0 ends before P with at least one eligible order
  none     window 0 has no eligible order at all
  clipped  every eligible b_o of window 0 is +0.0, so the costs are o (q + w) and the guesses are orders 1..K
  short    K is above the eligible count of window 0
  differ   two windows of the list guess different orders
"""
import collections

import numpy as np

import guess_model as gm
import order_model as om
import util
import window_model as wm

Case = collections.namedtuple("Case", "name x bps order q extras K regimes guesses")


def case(name, x, bps, order, K=1, q=15, extras=(), regimes=(), guesses=None):
    x = np.ascontiguousarray(np.asarray(x, np.int64).astype(np.int32))
    return Case(name, x, bps, order, q, tuple(extras), K, frozenset(regimes), guesses)


def ar2(n, seed=1):
    """y_t = 1.8 y_(t-1) - 0.9 y_(t-2) + N(0, 1), scaled by 300."""
    e = np.random.default_rng(seed).standard_normal(n)
    y = np.zeros(n)
    for t in range(n):
        y[t] = 1.8 * (y[t - 1] if t > 0 else 0.0) - 0.9 * (y[t - 2] if t > 1 else 0.0) + e[t]
    return np.round(300 * y).astype(np.int64)


def white(n, bits, seed):
    return np.random.default_rng(seed).integers(-(1 << (bits - 1)), 1 << (bits - 1), n)


def sine8(n, period=32):
    return np.round(127 * np.sin(2 * np.pi * np.arange(n) / period)).astype(np.int64)


def impulse(n, t, v=1000):
    x = np.zeros(n, np.int64)
    x[t] = v
    return x


def golden(n, start=0):
    return util.test_signal("ras103", 0)[start:start + n]


def all_cases():
    return [
        case("ar2_256", ar2(256), 16, 12, regimes={"wins"}, guesses=[2]),
        case("ar2_576", ar2(576), 16, 12, regimes={"wins"}, guesses=[2]),
        case("ar2_4096", ar2(4096), 16, 12, regimes={"wins"}, guesses=[2]),
        case("white24_4096", white(4096, 24, 5), 24, 12, regimes={"wins"}, guesses=[1]),
        case("constant_256", np.full(256, 1234), 16, 8, regimes={"loses", "early"}, guesses=[1]),
        case("sine8_512", sine8(512), 8, 8, regimes={"loses"}, guesses=[2]),
        case("sine_noise_64", util.sine_noise(64, 16, 36.0, 0.4, 0.04, 0), 16, 12, regimes={"early"}, guesses=[1]),
        # the sums start at t = P: over 32 samples of 64 R[1] can exceed R[0], |k_1| > 1 and e_1 < 0
        case("ar2_64_32", ar2(64, seed=10), 16, 32, regimes={"none"}, guesses=[]),
        case("silence_256", np.zeros(256), 16, 8, K=3, regimes={"clipped"}, guesses=[1, 2, 3]),
        # an impulse in front of t = P: R[] is all zero
        case("impulse_256", impulse(256, 3), 16, 8, K=3, regimes={"clipped"}, guesses=[1, 2, 3]),
        case("constant_256_K3", np.full(256, 1234), 16, 8, K=3, regimes={"short", "early"}, guesses=[1]),
        case("sine_noise_64_K32", util.sine_noise(64, 16, 36.0, 0.4, 0.04, 0), 16, 12, K=32, regimes={"short"},
             guesses=[1]),
        case("ar2_64_32_K2", ar2(64, seed=10), 16, 32, K=2, regimes={"none", "short"}, guesses=[]),
        case("golden_32_default", golden(4096), 16, 32, extras=wm.DEFAULT, regimes={"differ"}),
        case("golden_32_default_K2", golden(4096), 16, 32, K=2, extras=wm.DEFAULT, regimes={"differ"}),
        case("ar2_256_q5", ar2(256), 16, 12, q=5, regimes={"wins"}),
    ]


def config(c):
    return om.config(order=c.order, quant_precision=c.q)


def claims(c):
    """Assert from the model every regime case c names -> (winner, coded candidates, per-window guess records)."""
    cfg = config(c)
    best, cands, per_window = gm.search(c.x, c.bps, cfg, c.K, c.extras)
    P, g0 = c.order, per_window[0]
    ref = next(k for k in cands if k["j"] == 0 and k["o"] == P)
    if c.guesses is not None:
        assert g0["guesses"] == c.guesses, (c.name, g0["guesses"])
    assert all(len(g["guesses"]) == min(c.K, g["eligible"]) for g in per_window), c.name
    others = [k for k in cands if (k["j"], k["o"]) != (0, P)]
    if "wins" in c.regimes:
        exhaustive, _ = wm.search(c.x, c.bps, cfg, c.extras, True)
        assert (best["j"], best["o"]) != (0, P) and best["subframe_bits"] < ref["subframe_bits"], c.name
        assert (best["j"], best["o"]) == (exhaustive["j"], exhaustive["o"]), c.name
    if "loses" in c.regimes:
        assert others and all(k["status"] == om.STATUS_OK for k in others) and best is ref, c.name
    if "early" in c.regimes:
        assert 1 <= g0["eligible"] < P, (c.name, g0["eligible"])
    if "none" in c.regimes:
        assert g0["eligible"] == 0 and not others and best is ref, c.name
    if "clipped" in c.regimes:
        assert g0["eligible"] >= c.K and all(float(b) == 0.0 for b in g0["b"]), c.name
        assert g0["cost"] == [float(o * (c.q + c.bps)) for o in range(1, g0["eligible"] + 1)], c.name
        assert g0["guesses"] == list(range(1, c.K + 1)), c.name
    if "short" in c.regimes:
        assert c.K > g0["eligible"], (c.name, g0["eligible"])
    if "differ" in c.regimes:
        assert len({tuple(g["guesses"]) for g in per_window}) > 1, c.name
    return best, cands, per_window


def ids(cases):
    return [c.name for c in cases]
