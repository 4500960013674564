"""Material, branch predicates and the case table of the covariance-method estimators (use_direct_mse /
mae_optimization_steps), shared by tests/test_direct_mse_cases_cpu.py (which holds every case to the
branch it names and the oracle to the mathematics) and tests/test_gpu_direct_mse_extremes.py (which holds the kernels to
the oracle on every case).

  * material(name, n, bits): worst-case rows -- full-scale alternation and square waves, ramps, constants at both ends of
    the range, one impulse, silence, a clipped sine, full-range noise, a pure sine (rank 2), a golden music fixture --
    and stereo_pair(name, n, bits);
  * form(n, order, steps, aligned, stereo): the kernels launch_direct_mse (csrc/direct_mse.cpp) takes for a launch,
    restated from the launcher's rules as a table, without the library;
  * regulariser_steps(x, cfg, weight): how often the reference's loop (src/lpc.rs:887-894) doubles the diagonal load;
  * exact_system(...), backward_error(...): G and r of the covariance method in exact integer arithmetic, straight from
    src/lpc.rs:533-548, :573-600 and :853-883;
  * CASES: the table.  A case names the form it claims to reach; the CPU suite checks the claim.

Two kinds of edge cannot reach a kernel: every entry point that runs the estimator requires
block_size >= 64 (the candidate batches answer FLACENC_HIP_ERR_BAD_ARGUMENT below it, the frame-level calls code
Constant / Verbatim only), so a chain has at least 64 - 32 = 32 steps and n <= P never launches.  The cases of 1 and 2
steps and of n <= P are `entry="oracle"`: held to the mathematics on the CPU, and on the GPU to the documented answer."""
from collections import namedtuple
from fractions import Fraction

import numpy as np

import extreme_signals as xs
from oracle import oracle as orc

# ---- material ----
SQUARE_HALF_PERIOD = 7  # a period of 14 samples: no divisor of any block size used here


def material(name, n, bits, seed=0):
    """One row of worst-case material -> int64 [n] within `bits` bits."""
    lo, hi = xs.full_scale(bits)
    t = np.arange(n)
    if name == "alternation":
        return xs.alternation(n, bits)
    if name == "square":
        return np.where((t // SQUARE_HALF_PERIOD) % 2 == 0, hi, lo).astype(np.int64)
    if name == "ramp":
        return np.linspace(lo, hi, n).astype(np.int64)
    if name == "const_lo":
        return np.full(n, lo, np.int64)
    if name == "const_hi":
        return np.full(n, hi, np.int64)
    if name == "impulse":
        x = np.zeros(n, np.int64)
        x[n // 3] = lo
        return x
    if name == "zero":
        return np.zeros(n, np.int64)
    if name == "clipped":
        return np.clip(np.sin(t / 7.3) * hi * 2.5, lo, hi).astype(np.int64)
    if name == "noise":
        return xs.noise(n, bits, 1000 + seed).astype(np.int64)
    if name == "sine":
        return np.round(np.sin(2.0 * np.pi * t / 64.0) * 0.5 * hi).astype(np.int64)
    if name == "music":
        return xs.music(n, bits, seed=seed, start=257 * seed).astype(np.int64)
    if name == "side25":
        # the side channel of the 24-bit pair (alternation, -alternation - 1): 2 L + 1 = +-(2^24 - 1), a 25-bit row.
        # (No valid input leaves the integers a float holds exactly: |l - r| <= 2^24 - 1 at 24 bits and a 25-bit row
        # reaches -2^24 at most, so (float)(l - r) is exact everywhere; this is the widest it gets.)
        a = xs.alternation(n, 24)
        return 2 * a + 1
    raise KeyError(name)


EXTREMES = ("alternation", "square", "ramp", "const_lo", "const_hi", "impulse", "zero", "clipped", "noise", "sine",
            "music")
WELL_CONDITIONED = ("music", "noise")


def stereo_pair(name, n, bits, seed=0):
    """-> int64 [2, n]: L = hi / R = lo, L = R, R = -L - 1, one channel silent."""
    lo, hi = xs.full_scale(bits)
    if name == "hi_lo":
        return np.stack([np.full(n, hi, np.int64), np.full(n, lo, np.int64)])
    if name == "equal":
        m = material("music", n, bits, seed)
        return np.stack([m, m])
    if name == "inverted":
        l = material("alternation" if seed % 2 == 0 else "noise", n, bits, seed)
        return np.stack([l, -l - 1])
    if name == "silent":
        return np.stack([material("music", n, bits, seed), np.zeros(n, np.int64)])
    if name == "square_noise":
        return np.stack([material("square", n, bits), material("noise", n, bits, seed)])
    raise KeyError(name)


PAIRS = ("hi_lo", "equal", "inverted", "silent")


# ---- the launcher's rules (csrc/direct_mse.cpp: launch_direct_mse) ----
STREAM_PIECE = 512        # kStreamPiece: the sliding window of the chains
ERR_CHUNK = 1024          # kErrChunk: the window of the IRLS error pass
WG_ABOVE = 16384          # the one-kernel form keeps the IRLS weights in HBM scratch above this block size
SOLVE_LDS = 64 * 1024     # direct_mse_solve_kernel: LW lanes of (P^2 + 2 P) doubles each


def solve_lanes(order):
    """LW of direct_mse_solve_kernel: 64 halved while LW subframes' matrices exceed 64 KiB."""
    per = (order * order + 2 * order) * 8
    lw = 64
    while lw > 1 and per * lw > SOLVE_LDS:
        lw >>= 1
    return lw


def stream_niw(order):
    """NIW of direct_mse_stream_kernel<., ., NIW>: the accumulators per wave."""
    nb = (order + 1 + 3) >> 2
    ni = (nb + nb * (nb + 1) // 2 - 1 + 3) // 4
    nw = (ni + 3) // 4
    return (ni + nw - 1) // nw


def _b(v):
    return "true" if v else "false"


def form(n, order, steps, aligned, stereo=False):
    """What launch_direct_mse launches for a batch of `n`-sample subframes at `order` with `steps` IRLS steps, on rows that
    are `aligned` (16-byte aligned base, stride % 4 == 0: every host call, whose rows are staged at a padded stride) or
    not -> dict(name, chains, weighted, solve=(phases of direct_mse_solve_kernel), lw, block_rows, kernels={template
    instantiations}).  The entry points always pass the Gram scratch, the IRLS state and the weight scratch."""
    assert 1 <= order <= 32 and steps >= 0
    weighted = steps > 0
    lw = solve_lanes(order)
    kernels = set()
    if aligned:
        chains = "small" if order <= 11 else "tiles" if order <= 31 else "blocks"
        for wt in ((False, True) if weighted else (False,)):     # (step 0's weights are 1: the unweighted chain)
            if chains == "small":
                kernels.add("direct_mse_stream_small_kernel<%s, %s>" % (_b(stereo), _b(wt)))
            elif chains == "tiles":
                kernels.add("direct_mse_stream_tiles_kernel<%s, %s>" % (_b(stereo), _b(wt)))
            else:
                kernels.add("direct_mse_stream_kernel<%s, %s, %d>" % (_b(stereo), _b(wt), stream_niw(order)))
        solve = (1, 2) if weighted else (0,)
        if weighted:
            kernels.add("direct_mse_irls_error_kernel<%s>" % _b(stereo))
    else:
        wg = weighted and n > WG_ABOVE
        chains = "one-kernel-wg" if wg else "one-kernel"
        kernels.add("direct_mse_kernel<%s, %s, %s>" % (_b(stereo), _b(weighted), _b(wg)))
        solve = () if weighted else (0,)                         # with IRLS steps the kernel solves on its wave 0
    for ph in solve:
        kernels.add("direct_mse_solve_kernel<%d>" % ph)
    return dict(name=chains + ("+w" if weighted else ""), chains=chains, weighted=weighted, solve=solve,
                lw=lw if solve else None, block_rows=(order + 4) >> 2, kernels=kernels)


def selectable_kernels():
    """Every template instantiation of direct_mse.cpp the launcher can select.  (direct_mse_stream_kernel is
    instantiated for NIW = 1..4, but it is taken at order 32 only, where NIW = 4.)"""
    out = set()
    for st in (False, True):
        for order in range(1, 33):
            for steps in (0, 1):
                for aligned in (False, True):
                    for n in (4096, WG_ABOVE + 1):
                        out |= form(n, order, steps, aligned, st)["kernels"]
    return out


# ---- the reference's regulariser loop ----
def regulariser_steps(x, cfg, weight=None):
    """The doublings `while !solve_sym_mut(..)` (src/lpc.rs:887-894) takes on subframe x: 0 when the first Cholesky
    factorisation succeeds.  Replayed on the oracle's pre-regularisation Gram matrix with its Cholesky; the diagonal is
    loaded in f64 as the reference loads it, so a load below half an ulp of the diagonal changes nothing and the loop
    goes on.  -> (doublings, lambda = the load reached, 0 or 2^(doublings - 1))."""
    corr, gram, _, st = orc.lpc_with_direct_mse(np.ascontiguousarray(x, np.int32), cfg, weight)
    assert st == 0
    g = gram.copy()
    P = g.shape[0]
    reg, k = 0.0, 0
    while not orc.cholesky_solve(g, corr[1:])[0]:
        old = reg
        reg = max(1.0, reg + reg)
        for i in range(P):
            g[i, i] += reg - old
        k += 1
        assert k <= 2000
    return k, reg


# ---- the covariance method in exact arithmetic ----
def exact_ints(v):
    """f32 / f64 array -> (object array of Python ints m, s) with v == m * 2^-s exactly."""
    fr = [Fraction(float(a)) for a in np.asarray(v).reshape(-1)]
    den = max([f.denominator for f in fr] + [1])
    s = den.bit_length() - 1
    assert den == 1 << s
    return np.array([f.numerator * (den // f.denominator) for f in fr], dtype=object), s


def exact_system(x, window, order, weight=None, mutant=None):
    """G [P][P] and r [P] of weighted_lpc_with_direct_mse as Fractions, from the definition (src/lpc.rs):
      x_w[t] = f32(x[t] * w[t])                                                       (:751-754, one f32 rounding)
      r[k]   = sum_{t = P .. n-1}    x_w[t - k] * f32(weight[t] * x_w[t]),            k = 1..P     (:533-548, :872-877)
      G[i][j] = sum_{t = P-1 .. n-2} x_w[t - i] * f32(weight[t + 1] * x_w[t - j]),    i <= j       (:573-600, :878-883;
                the signal without its last sample, ShiftedWeight<1>), mirrored below the diagonal.
    Every factor is an f32 value, so every sum is an exact rational.  The mutants (unweighted) are two misreadings of
    those lines: "time" sums G over t = P .. n-1 (the whole signal, its range one sample late), "lag" takes
    r[k] at lag k - 1 (corr[0..P] for corr[1..=P])."""
    x = np.ascontiguousarray(x, np.int32)
    n, P = len(x), order
    assert mutant is None or weight is None
    xw = orc.fill_windowed_signal(x, orc.window_weights(window, n))
    w = np.ones(n + 1, np.float32)
    if weight is not None:
        w[:n] = np.ascontiguousarray(weight, np.float32)
    a, sa = exact_ints(xw)
    G = [[Fraction(0)] * P for _ in range(P)]
    r = [Fraction(0)] * P
    if n >= P + 1:
        b, sb = exact_ints((w[:n] * xw).astype(np.float32))       # f32(weight[t] * x_w[t])
        for k in range(1, P + 1):
            lag = k - 1 if mutant == "lag" else k
            r[k - 1] = Fraction(int(np.dot(a[P - lag:n - lag], b[P:n])), 1 << (sa + sb))
        t0, t1 = (P, n) if mutant == "time" else (P - 1, n - 1)   # t in [t0, t1)
        for j in range(P):
            c, sc = exact_ints((w[t0 + 1:t1 + 1] * xw[t0 - j:t1 - j]).astype(np.float32))
            for i in range(j + 1):
                G[i][j] = G[j][i] = Fraction(int(np.dot(a[t0 - i:t1 - i], c)), 1 << (sa + sc))
    return G, r


def float_solution(G, r, lam=0):
    """The f64 solution of (G + lam I) a = r by numpy, from the rounded matrix: what a mutant's solver would answer."""
    P = len(r)
    m = np.array([[float(G[i][j]) for j in range(P)] for i in range(P)]) + float(lam) * np.eye(P)
    return np.linalg.solve(m, np.array([float(v) for v in r]))


def backward_error(G, r, a, lam):
    """|| (G + lam I) a - r ||_inf / (|| G + lam I ||_inf || a ||_inf + || r ||_inf) in exact arithmetic -> float (0 / 0 = 0)."""
    P = len(r)
    av = [Fraction(float(v)) for v in a]
    lam = Fraction(lam)
    res = mat = Fraction(0)
    for i in range(P):
        row = list(G[i])
        row[i] += lam
        res = max(res, abs(sum((row[j] * av[j] for j in range(P)), Fraction(0)) - r[i]))
        mat = max(mat, sum((abs(v) for v in row), Fraction(0)))
    den = mat * max([abs(v) for v in av] + [Fraction(0)]) + max([abs(v) for v in r] + [Fraction(0)])
    return float(res / den) if den else (0.0 if res == 0 else float("inf"))


# ---- the case table ----
Case = namedtuple("Case", "name n order steps bps window entry layout rows claim")
# entry:  "qlpc" (mono rows, flacenc_hip_qlpc_batch[_async]), "stereo_qlpc", "stereo_frames" (encode_stereo_frames),
#         "frames3" (encode_frames with 3 channels), "oracle" (no kernel can be reached: see the module docstring)
# layout: "host" (staged at a padded stride: aligned) or a device layout: "stride+1", "stride+3", "offset1" (a stride of
#         whole quads, the base one word behind a 16-byte boundary), "canary" (an odd stride of n + 5 or n + 6)
# rows:   a tuple of row specs "material[:bits[:seed]]" (mono) or "pair[:bits[:seed]]" (stereo frames) or
#         "a|b|c" (a 3-channel frame)
# claim:  the name of the form it reaches
DEVICE_LAYOUTS = ("stride+1", "stride+3", "offset1", "canary")


def layout_stride(layout, n):
    """(stride in words, offset of the first row in words behind a 16-byte aligned allocation)."""
    if layout == "stride+1":
        return n + 1, 0
    if layout == "stride+3":
        return n + 3, 0
    if layout == "offset1":
        return (n + 3 + 4) & ~3, 1
    if layout == "canary":
        return (n + 5) | 1, 0
    raise KeyError(layout)


def is_aligned(case):
    if case.layout == "host":
        return True
    stride, off = layout_stride(case.layout, case.n)
    return off % 4 == 0 and stride % 4 == 0


def is_stereo(case):
    return case.entry in ("stereo_qlpc", "stereo_frames")


def case_form(case):
    return form(case.n, case.order, case.steps, is_aligned(case), is_stereo(case))


def _row(spec, n, bps):
    parts = spec.split(":")
    bits = int(parts[1]) if len(parts) > 1 and parts[1] else bps
    seed = int(parts[2]) if len(parts) > 2 else 0
    return parts[0], bits, seed


def case_rows(case):
    """The samples of a case: int32 [rows, n] for "qlpc" / "oracle", [frames, 2, n] for the stereo entries, [frames, 3, n]
    for "frames3"."""
    out = []
    for spec in case.rows:
        if case.entry in ("qlpc", "oracle"):
            name, bits, seed = _row(spec, case.n, case.bps)
            out.append(material(name, case.n, bits, seed))
        elif is_stereo(case):
            name, bits, seed = _row(spec, case.n, case.bps)
            out.append(stereo_pair(name, case.n, bits, seed))
        else:
            chans = [_row(s, case.n, case.bps) for s in spec.split("|")]
            out.append(np.stack([material(nm, case.n, b, sd) for nm, b, sd in chans]))
    return np.ascontiguousarray(np.stack(out), np.int32)


def case_bps(case):
    """Per-row bits per sample of a mono case (a row may carry its own width)."""
    return np.array([_row(s, case.n, case.bps)[1] for s in case.rows], np.uint8)


def mono_rows(case):
    """Every subframe signal a case analyses, with its width: [(int32 [n], bps)] -- the rows of a mono case, L R M S of a
    stereo frame, the channels of a 3-channel frame."""
    x = case_rows(case)
    if case.entry in ("qlpc", "oracle"):
        return list(zip(x, (int(b) for b in case_bps(case))))
    out = []
    for f in x:
        if is_stereo(case):
            l, r = f[0].astype(np.int64), f[1].astype(np.int64)
            out += [(f[0], case.bps), (f[1], case.bps), (((l + r) >> 1).astype(np.int32), case.bps),
                    ((l - r).astype(np.int32), case.bps + 1)]
        else:
            out += [(c, case.bps) for c in f]
    return out


RECT = "rectangle"
TUKEY = ("tukey", 0.4)
ORDERS = (1, 3, 4, 7, 8, 11, 12, 15, 16, 31, 32)
IRLS_ORDERS = (7, 11, 12, 31, 32)
FORM_ORDERS = (7, 12, 32)                 # one order of each aligned form: small, tiles, blocks
CHAIN_LENGTHS = (1, 2, 511, 512, 513, 1024, 1025)
IRLS_BLOCKS = (1023, 1024, 1025, 2049)
SOLVE_ORDERS = (8, 12, 16, 24, 32)        # LW = 64, 32, 16, 8, 4
FOUR = ("alternation::0", "noise::1", "music::2", "ramp::0")


def _seam_rows(count, lw):
    """`count` different rows; on either side of every workgroup seam of the batched solve an extreme row and a music row:
    (extreme, music) at odd seams, (music, extreme) at even ones."""
    rows = []
    for k in range(count):
        rows.append("music::%d" % k if k % 2 else "noise::%d" % k)
    ext = ("alternation", "const_lo", "square", "impulse")
    for s, at in enumerate(range(lw, count, lw)):
        a, b = (ext[s % 4] + "::0", "music::%d" % (1000 + s))
        if s % 2:
            a, b = b, a
        rows[at - 1], rows[at] = a, b
    return tuple(rows)


def _build():
    cases = []

    def add(name, n, order, steps, bps, rows, entry="qlpc", layout="host", window=RECT, claim=None):
        c = Case(name, n, order, steps, bps, window, entry, layout, tuple(rows), claim)
        cases.append(c._replace(claim=claim or case_form(c)["name"]))

    # every order edge on every extreme, widths rotating; n = 601: odd, more than one window piece
    for k, order in enumerate(ORDERS):
        bps = (16, 24, 8)[k % 3]
        add("order %d" % order, 601, order, 0, bps, EXTREMES)
        if order in IRLS_ORDERS:
            for steps in (1, 3):
                add("order %d irls %d" % (order, steps), 601, order, steps, (24, 16)[steps == 3], EXTREMES)
    add("order 8 tukey", 601, 8, 0, 16, EXTREMES, window=TUKEY)
    add("order 12 tukey irls 1", 601, 12, 1, 24, EXTREMES, window=TUKEY)
    add("side25", 1152, 8, 0, 25, ("side25", "noise:25:3", "const_lo:25"))
    add("side25 irls", 1152, 12, 2, 25, ("side25", "noise:25:3", "const_lo:25"))
    # the sliding window's edges: n - P steps
    for order in FORM_ORDERS:
        for length in CHAIN_LENGTHS:
            n = order + length
            if n < 64:
                add("steps %d order %d" % (length, order), n, order, 0, 24, FOUR, entry="oracle")
                add("steps %d order %d irls" % (length, order), n, order, 1, 24, FOUR, entry="oracle")
            else:
                add("steps %d order %d" % (length, order), n, order, 0, 24, FOUR)
                add("steps %d order %d irls" % (length, order), n, order, 1, 16, FOUR)
    # the error pass's window
    for order in FORM_ORDERS:
        for n in IRLS_BLOCKS:
            add("irls block %d order %d" % (n, order), n, order, 2, 16, FOUR)
    # n <= P: nothing to estimate from
    for n in (8, 5):
        add("short %d order 8" % n, n, 8, 0, 16, ("noise::1", "const_hi::0"), entry="oracle")
        add("short %d order 8 irls" % n, n, 8, 1, 16, ("noise::1", "const_hi::0"), entry="oracle")
    # the batched solve across workgroups, ragged last one
    for order in SOLVE_ORDERS:
        lw = solve_lanes(order)
        for count in (lw + 1, 2 * lw + 3):
            for steps in (0, 2):
                add("solve %d x order %d steps %d" % (count, order, steps), 256, order, steps, 16, _seam_rows(count, lw))
    add("solve stereo order 16", 256, 16, 2, 16, ["%s::%d" % (PAIRS[k % 4], k) for k in range(9)], entry="stereo_qlpc")
    # stereo forms on aligned rows
    for order in FORM_ORDERS:
        for steps in (0, 1):
            add("stereo order %d steps %d" % (order, steps), 1152, order, steps, 24, PAIRS, entry="stereo_qlpc")
    # unaligned device rows: the one-kernel form
    add("one-kernel mono", 1000, 8, 0, 16, EXTREMES, layout="stride+1")
    add("one-kernel mono irls", 1000, 8, 1, 24, EXTREMES, layout="stride+1")
    add("one-kernel mono order 12", 1025, 12, 1, 16, FOUR, layout="canary")
    add("one-kernel mono order 16", 2049, 16, 0, 24, FOUR, layout="offset1")
    add("one-kernel mono order 32", 1023, 32, 1, 24, FOUR, layout="stride+3")
    add("one-kernel mono order 7 tukey", 4096, 7, 2, 16, FOUR, layout="offset1", window=TUKEY)
    add("one-kernel stereo", 1152, 8, 0, 24, PAIRS, entry="stereo_qlpc", layout="stride+3")
    add("one-kernel stereo irls", 1152, 12, 2, 24, PAIRS, entry="stereo_qlpc", layout="stride+3")
    add("one-kernel stereo frames", 1152, 8, 1, 16, PAIRS + ("square_noise::5",), entry="stereo_frames", layout="offset1")
    add("one-kernel stereo frames order 32", 4096, 32, 0, 24, PAIRS, entry="stereo_frames", layout="offset1")
    add("one-kernel 3 channels", 1152, 12, 0, 16,
        ("music::1|alternation|noise::2", "ramp|zero|clipped", "const_hi|music::3|square"), entry="frames3",
        layout="canary")
    add("one-kernel 3 channels irls", 1000, 8, 1, 24,
        ("music::1|alternation|noise::2", "impulse|sine|const_lo"), entry="frames3", layout="canary")
    add("one-kernel wg mono", WG_ABOVE + 1, 8, 1, 16, ("music::0", "noise::1"), layout="stride+1")
    add("one-kernel wg stereo", WG_ABOVE + 4, 8, 1, 16, ("silent::2",), entry="stereo_qlpc", layout="stride+1")
    # frame level on aligned rows: the extremes at 1152 and 4096
    for n in (1152, 4096):
        add("frames %d" % n, n, 8, 0, 24, PAIRS + ("square_noise::1",), entry="stereo_frames")
        add("frames %d irls" % n, n, 12, 1, 16, PAIRS + ("square_noise::1",), entry="stereo_frames")
    return cases


CASES = _build()
GPU_CASES = [c for c in CASES if c.entry != "oracle"]


def by_name(name):
    return next(c for c in CASES if c.name == name)
