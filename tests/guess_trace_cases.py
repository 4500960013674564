"""The deterministic calls of the order-guess trace suite (tests/test_gpu_order_guess_trace.py on the GPU,
tests/test_order_guess_cpu.py through the model alone), in the style of tests/guess_cases.py: every call names an entry
point, its rows, widths, configuration, K and extra-window list, and the properties of the guess -- the per-window
eligible count, mask and cost[] that order_guess_kernel computes and flacenc_hip_debug_set_order_guess_trace makes visible
-- that it stands for.  claims(call) asserts each named property from tests/guess_model.py on the CPU, so a GPU case
proves what it reaches before a byte is compared.

Entry points ("entry"):
  batch          qlpc_batch: rows [k][n], bps one width or one per row
  stereo         stereo_qlpc_batch: rows [f][2][n] at one width; subframe 4 f + role, the side role one bit wider
  stereo_frames  encode_stereo_frames: as stereo
  wasted         encode_frames with FLACENC_HIP_FLAG_WASTED_BITS on ONE frame rows [1][C][n] whose every row has zero low
                 bits: the search runs once, over the shifted rows x >> k at w - k

Properties ("reach"):
  full       some subframe's window 0 has every order 1..P eligible (cost[o - 1] of every o: the k_o extraction at every
             index of the order's bucket)
  early      some window's chain ends before P with at least one eligible order
  none       some window has no eligible order
  width      every subframe's costs differ in every eligible entry from those at one bit less (the o (q + w) term), so
             the neighbouring row's width, the side role's missing bit or a missing shift cannot give them
  clip_low   some x_o = (float)(e_o / 2n) lies in (1 - 2^-10, 1) and its b_o is +0.0
  clip_one   some x_o is exactly 1.0f and its b_o is +0.0
  clip_high  some x_o lies in (1, 1 + 2^-10) and its b_o is positive
  large      some x_o is at least 2^46 (the bound is 2^47, see tests/test_gpu_order_guess_trace.py) and every x_o is finite
  dead       some extra window has no non-zero weight: R is all zero, every order is eligible, every b_o is +0.0, the costs
             are o (q + w) and the guesses 1..K
  k_at       K equals window 0's eligible count in some subframe; k_below / k_above: one below, one above it
  all32      P = K = 32 and some window has all 32 orders eligible: every order is a guess
  windows    within one subframe the windows' eligible counts differ and so do their masks

log2f_indices(calls) is the set of dev_log2f table indices (ix - 0x3f330000) >> 19 & 15 the calls' x_o take.

No tie of two costs is in the corpus.  With b = +0.0 (silence, the impulse, a dead window) the costs are o (q + w), no
two alike.  With b > 0 none was found: over the 40000 seeded trials of clip_noise (seeds 0..39999, 320000 chain entries:
the search that found the clip cases) no two costs of one chain were bitwise equal, and none is expected -- b_o (n - o)
is the exact product of a float and an integer, and two of them would have to differ by exactly (o' - o)(q + w).  The
pick loop's strict comparison is held to the model on the host build (tests/test_order_guess_cpu.py) only.
"""
import collections

import numpy as np

import extreme_signals as es
import guess_cases as gc
import guess_model as gm
import order_model as om
import wasted_model
import window_cases as wc
import window_model as wm
from oracle import oracle

Call = collections.namedtuple("Call", "name entry rows bps order q K extras kw reach")

ENTRIES = ("batch", "stereo", "stereo_frames", "wasted")


def call(name, entry, rows, bps, order, K=1, q=15, extras=(), kw=None, reach=()):
    assert entry in ENTRIES
    rows = np.ascontiguousarray(np.asarray(rows, np.int64).astype(np.int32))
    assert rows.ndim == (2 if entry == "batch" else 3)
    if np.ndim(bps):
        bps = np.asarray(bps, np.uint8)
    return Call(name, entry, rows, bps, order, q, K, tuple(extras), dict(kw or {}), frozenset(reach))


def config(c):
    return om.config(order=c.order, quant_precision=c.q, **c.kw)


def frame_config(c):
    """The model's frame config of the two frame-level entries (every stereo assignment for stereo_frames)."""
    st = c.entry == "stereo_frames"
    return oracle.make_frame_config(config(c), use_leftside=st, use_rightside=st, use_midside=st)


def subframes(c):
    """[(signal, width)] in the order of the call's subframes: what the search of the call sees."""
    if c.entry == "batch":
        return [(x, int(c.bps[i]) if np.ndim(c.bps) else int(c.bps)) for i, x in enumerate(c.rows)]
    out = []
    if c.entry in ("stereo", "stereo_frames"):
        for l, r in c.rows:
            m, s = oracle.stereo_to_midside(l, r)
            out += [(l, c.bps), (r, c.bps), (m, c.bps), (s, c.bps + 1)]
        return out
    fc = frame_config(c)
    assert len(c.rows) == 1
    for x in c.rows[0]:
        k = wasted_model.wasted_of(x, fc)
        assert k > 0, c.name  # (every row is shifted: the unflagged pass over every frame is left out)
        out.append((x >> k, c.bps - k))
    return out


def model(c):
    """gm.search(...)[2] of every subframe: [[per-window guess record]]."""
    cfg = config(c)
    return [gm.search(x, w, cfg, c.K, c.extras)[2] for x, w in subframes(c)]


def mask_of(g):
    return sum(1 << (o - 1) for o in g["guesses"])


def xs_of(g, n):
    """x_o of a guess record's chain, as bits_per_sample forms them."""
    with np.errstate(over="ignore", under="ignore"):
        return [np.float32(float(e) * (0.5 / float(n))) for e in g["e"]]


def log2f_indices(calls):
    out = set()
    for c in calls:
        n = c.rows.shape[-1]
        for per_window in model(c):
            for g in per_window:
                out |= {((int(np.float32(x).view(np.uint32)) - 0x3f330000) >> 19) & 15 for x in xs_of(g, n) if x > 0}
    return out


def claims(c):
    """Assert from the model every property call c names -> model(c)."""
    found = model(c)
    cfg, n, P = config(c), c.rows.shape[-1], c.order
    subs = subframes(c)
    records = [g for per_window in found for g in per_window]
    pairs = [(g, x, b) for g in records for x, b in zip(xs_of(g, n), g["b"])]
    one, eps = np.float32(1.0), np.float32(2.0 ** -10)
    for g in records:
        assert len(g["guesses"]) == min(c.K, g["eligible"]) and len(g["cost"]) == g["eligible"] <= P, c.name
    if "full" in c.reach:
        assert any(per_window[0]["eligible"] == P for per_window in found), c.name
    if "early" in c.reach:
        assert any(1 <= g["eligible"] < P for g in records), c.name
    if "none" in c.reach:
        assert any(g["eligible"] == 0 for g in records), c.name
    if "width" in c.reach:
        assert all(per_window[0]["eligible"] >= 1 for per_window in found), c.name
        for (x, w), per_window in zip(subs, found):
            less = gm.search(x, w - 1, cfg, c.K, c.extras)[2]
            for g, l in zip(per_window, less):
                assert g["eligible"] == l["eligible"] and all(a != b for a, b in zip(g["cost"], l["cost"])), c.name
    if "clip_low" in c.reach:
        assert any(one - eps < x < one and float(b) == 0.0 and not np.signbit(b) for _, x, b in pairs), c.name
    if "clip_one" in c.reach:
        assert any(x == one and float(b) == 0.0 and not np.signbit(b) for _, x, b in pairs), c.name
    if "clip_high" in c.reach:
        assert any(one < x < one + eps and float(b) > 0.0 for _, x, b in pairs), c.name
    if "large" in c.reach:
        assert all(np.isfinite(x) for _, x, _ in pairs) and max(float(x) for _, x, _ in pairs) >= 2.0 ** 46, c.name
    if "dead" in c.reach:
        dead = [j for j, e in enumerate(c.extras, 1) if not np.any(wm.weights(e, n))]
        assert dead, c.name
        for (_, w), per_window in zip(subs, found):
            for j in dead:
                g = per_window[j]
                assert g["eligible"] == P >= c.K and all(float(b) == 0.0 for b in g["b"]), (c.name, j)
                assert g["cost"] == [float(o * (c.q + w)) for o in range(1, P + 1)], (c.name, j)
                assert g["guesses"] == list(range(1, c.K + 1)), (c.name, j)
    for name, d in (("k_at", 0), ("k_below", -1), ("k_above", 1)):
        if name in c.reach:
            assert c.K >= 1 and any(per_window[0]["eligible"] + d == c.K for per_window in found), (c.name, name)
    if "all32" in c.reach:
        assert P == c.K == 32 and any(g["eligible"] == 32 and mask_of(g) == 0xFFFFFFFF for g in records), c.name
    if "windows" in c.reach:
        assert any(len({g["eligible"] for g in per_window}) > 1 and len({mask_of(g) for g in per_window}) > 1
                   for per_window in found), c.name
    return found


# ---- material ----
def music_rows(n, order, bits=16):
    """Four rows of n samples for one order: two music rows, white noise and an AR(2) row (well conditioned: every order
    is eligible on the last two at any block size)."""
    return [es.music(n, bits, start=order * n), es.music(n, bits, start=(3 * order + 11) * n),
            gc.white(n, bits, 100 + order), gc.ar2(n, seed=order) << (bits - 16)]


def clip_noise(seed):
    """Trial `seed` of the search for chains at the clip b = 0: Gaussian noise of 1.3 to 2.6 LSB, 64..576 samples, for
    order 8 at 16 bits under the default window."""
    rng = np.random.default_rng(seed)
    n = int(rng.integers(64, 577))
    amp = float(rng.uniform(1.3, 2.6))
    return np.round(rng.standard_normal(n) * amp).astype(np.int64)


def unit_energy(n=64, order=2):
    """A row with R[1] = 0 and R[0] = 2 n exactly under the rectangular window (sums from t = order on): k_1 = 0,
    e_1 = R[0] and x_1 = 1.0f.  Non-zero samples at odd t only: 23 of +-2, 4 of +-3, 128 = 2 * 64 in all."""
    assert n == 64 and order == 2
    x = np.zeros(n, np.int64)
    t = np.arange(3, 3 + 2 * 27, 2)
    x[t] = [2] * 23 + [3] * 4
    x[t[::2]] *= -1
    return x


def square4(n, bits):
    """Full scale with period 4 (hi, hi, lo, lo): R[1] is next to nothing, so e_1 is next to R[0], the largest there is."""
    lo, hi = es.full_scale(bits)
    return np.where(np.arange(n) % 4 < 2, hi, lo).astype(np.int64)


def opposed(x, bits):
    """A stereo frame whose side channel l - r is x's full scale one bit up: r = -l - 1 (clipped to the width)."""
    lo, hi = es.full_scale(bits)
    return np.stack([x, np.clip(-x - 1, lo, hi)])


# ---- the calls ----
DEAD64 = (wc.DEAD[0], (wm.TUKEY, 0.2, 0, 0), wc.DEAD[2])  # entries 1 and 3 have no non-zero weight on 64 samples
CLIP_BOTH, CLIP_ONE = 464, 1424  # clip_noise trials: x_5..x_7 above 1 and x_8 below it in one chain; x_7 = 1.0f


def bucket_calls():
    out = []
    for order in wc.BUCKET_EDGES:
        for K in sorted({1, order}):
            reach = {"full"} | ({"all32"} if order == K == 32 else set())
            out.append(call("bucket_%d_K%d" % (order, K), "batch", music_rows(256, order), 16, order, K=K, reach=reach))
    return out


def size_calls():
    return [call("size_%d" % n, "batch", [es.music(n, 16, start=5 * n), gc.white(n, 16, n)], 16, 8, reach={"full"})
            for n in (64, 65, 4096, 32767)]


def width_calls():
    n, order = 256, 8
    widths = (8, 16, 17, 24, 25)
    rows = [es.music(n, min(b, 24), start=(b + 1) * n) for b in widths]
    shifted = np.stack([es.music(n, 16, start=3 * n) << 8, es.music(n, 16, start=4 * n) << 4,
                        es.music(n, 20, start=5 * n) << 4])[None]
    out = [call("width_rows", "batch", rows, widths, order, K=2, reach={"width", "full"}),
           call("width_wasted", "wasted", shifted, 24, order, K=2, reach={"width"})]
    for bits in (16, 24):
        frames = np.stack([es.music(n, bits, start=(2 * f + c + bits) * n) for f in range(2) for c in range(2)])
        frames = frames.reshape(2, 2, n)
        for entry in ("stereo", "stereo_frames"):
            out.append(call("width_%s_%d" % (entry, bits), entry, frames, bits, order, K=2, reach={"width"}))
    return out


def log2f_calls():
    n = 32767
    out = [call("clip_both_sides", "batch", [clip_noise(CLIP_BOTH)], 16, 8, reach={"clip_low", "clip_high"}),
           call("clip_exactly_one", "batch", [clip_noise(CLIP_ONE)], 16, 8, reach={"clip_one"}),
           call("clip_unit_energy", "batch", [unit_energy()], 16, 2, kw=dict(window="rectangle"), reach={"clip_one"}),
           # full-scale alternation on the side of 24-bit stereo (x_1 near 2^21: order 1 predicts it) and the period-4
           # square wave, whose x_1 is within a factor of two of the bound 2^47
           call("largest_alternation", "stereo", [opposed(es.alternation(n, 24), 24)], 24, 8),
           call("largest_square", "stereo", [opposed(square4(n, 24), 24)], 24, 8, reach={"large"})]
    return out


def chain_calls():
    music64 = [es.music(64, 16, start=7 * 64), es.music(64, 16, start=900 * 64), es.noise(64, 16, seed=64)]
    seven = [es.music(256, 16, start=7 * 256)]  # window 0's chain has 6 eligible orders of 32
    out = [call("dead_64", "batch", music64, 16, 8, K=3, extras=DEAD64, reach={"dead", "none"})]
    out += [call("eligible_6_K%d" % K, "batch", seven, 16, 32, K=K, reach={name, "early"})
            for K, name in ((5, "k_below"), (6, "k_at"), (7, "k_above"))]
    out.append(call("windows_127", "batch", [es.music(127, 16, start=7 * 127), es.music(127, 16, start=900 * 127)], 16,
                    32, K=2, extras=wc.E7, reach={"windows", "none", "early"}))
    return out


def all_calls():
    return bucket_calls() + size_calls() + width_calls() + log2f_calls() + chain_calls()


def corpus_call(c):
    """A case of tests/guess_cases.py as a call of this suite."""
    return call(c.name, "batch", c.x[None, :], c.bps, c.order, K=c.K, q=c.q, extras=c.extras)


def ids(calls):
    return [c.name for c in calls]
