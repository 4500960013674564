"""Worst-case material shared by the parity, order-search and window-search suites, the record check of the flagged
candidate batch against tests/order_model.py or tests/window_model.py, and predicates saying which branch of
order_search_kernel every candidate of a subframe reaches (computed from the model on the CPU, so a case can assert that
it reaches its branch, and in which candidate)."""
import numpy as np

import order_model as om

MAX_P_TO_BITS = (1 << 27) - 1  # rice.rs:51
LDS_BUDGET = 160 * 1024  # order_search_kernel keeps the residual rows in LDS while its image fits this


def extreme_frames(rng, n, bps):
    """Stereo frames built from worst-case material: full-scale alternation and square waves,
    impulses, full-range ramps, clipped sines, one channel silent / constant / inverted."""
    lo, hi = -(1 << (bps - 1)), (1 << (bps - 1)) - 1
    t = np.arange(n)

    def one():
        k = int(rng.integers(0, 8))
        if k == 0:
            return np.where(t % 2 == 0, hi, lo)
        if k == 1:
            return np.where((t // int(rng.integers(1, 200))) % 2 == 0, hi, lo)
        if k == 2:
            x = np.zeros(n, np.int64)
            x[rng.integers(0, n, int(rng.integers(1, 6)))] = rng.choice([lo, hi])
            return x
        if k == 3:
            return np.linspace(lo, hi, n).astype(np.int64)
        if k == 4:
            return np.clip(np.sin(t / float(rng.uniform(1.5, 300.0))) * hi * float(rng.uniform(1.0, 4.0)), lo, hi).astype(np.int64)
        if k == 5:
            return np.full(n, int(rng.integers(lo, hi + 1)))
        if k == 6:
            return rng.integers(lo, hi + 1, n)
        return (rng.integers(-3, 4, n)).cumsum().clip(lo, hi)

    frames = []
    for _ in range(6):
        l, r = one(), one()
        m = int(rng.integers(0, 5))
        if m == 0:
            r = l.copy()
        elif m == 1:
            r = np.clip(-l, lo, hi)
        elif m == 2:
            r = np.clip(l + rng.integers(-2, 3, n), lo, hi)
        frames.append(np.stack([l, r]))
    return np.stack(frames).astype(np.int32)


def params_record(p):
    """A status-0 flacenc_hip_subframe_params record as the models' record functions state one."""
    return {"order": int(p["order"]), "shift": int(p["shift"]), "precision": int(p["precision"]),
            "coefs": [int(c) for c in p["coefs"]], "rice_order": int(p["rice_order"]),
            "rice_params": [int(c) for c in p["rice_params"][:1 << int(p["rice_order"])]], "status": 0,
            "code_bits": int(p["code_bits"]), "subframe_bits": int(p["subframe_bits"]),
            "sum_quotients": int(p["sum_quotients"])}


def check_rows(params, residual, R, A, x, bps, cfg, where, record=om.record):
    """Status, R[], unquantised coefficients, record fields and residual rows of a flagged candidate batch == the
    model's, row by row.  record(x, bps, cfg) -> (record fields, residual row, autocorr [33], lpc_coefs [32]):
    order_model.record, or window_record(extras, orders) for FLACENC_HIP_FLAG_WINDOW_SEARCH, whose autocorr is the winning
    window's R_j."""
    for i in range(len(x)):
        rec, resid, ac, lc = record(x[i], int(bps[i]) if np.ndim(bps) else bps, cfg)
        p = params[i]
        assert int(p["status"]) == rec["status"], (where, i)
        assert np.array_equal(R[i], ac), (where, i)
        assert np.array_equal(A[i], lc), (where, i)
        if rec["status"] != 0:
            continue
        got = params_record(p)
        assert got == rec, (where, i, got, rec)
        assert np.array_equal(residual[i], resid), (where, i)


def window_record(extras, orders):
    """check_rows' record function for one extra-window list (tests/window_model.py) and the orders switch."""
    import window_model as wm
    return lambda x, bps, cfg: wm.record(x, bps, cfg, extras, orders)


# ---- material ----
def full_scale(bits):
    return -(1 << (bits - 1)), (1 << (bits - 1)) - 1


def alternation(n, bits):
    """Full-scale alternation (the seed-2616 pattern): at orders 24 and 32 the residual wraps i32."""
    lo, hi = full_scale(bits)
    return np.where(np.arange(n) % 2 == 0, hi, lo).astype(np.int64)


def noise(n, bits, seed):
    lo, hi = full_scale(bits)
    return np.random.default_rng(seed).integers(lo, hi + 1, n)


def music(n, bits, seed=0, start=0):
    """The golden fixtures, tiled; above 16 bits shifted up with random low bits."""
    import util
    names = ("ras103", "ras22", "sus109", "sus6")
    x = np.concatenate([util.test_signal(nm, c) for nm in names for c in (0, 1)]).astype(np.int64)
    x = np.tile(x, (start + n) // len(x) + 1)[start:start + n]
    if bits < 16:
        return x >> (16 - bits)
    if bits > 16:
        x = (x << (bits - 16)) | np.random.default_rng(seed + n).integers(0, 1 << (bits - 16), n)
    return x


# ---- the kernel's branches, from the model ----
def finest_order(n):
    """finest_partition_order(n, 64) (rice.rs:157-165)."""
    lg = 0
    while (2 << lg) <= n // 64:
        lg += 1
    tz = 0
    while ((n >> tz) & 1) == 0 and tz < 15:
        tz += 1
    return min(lg, tz, 8)


def search_lds_bytes(n, lds_u=True):
    """order_search_kernel's LDS image: the samples, the zig-zag rows with lds_u, the tables and 1744 bytes."""
    r16 = lambda v: (v + 15) & ~15  # noqa: E731
    return r16(4 * n) * (2 if lds_u else 1) + r16((1 << finest_order(n)) * 31 * 4) + 1744


def lds_edge():
    """(the largest block whose order_search_kernel image, residual rows included, fits the LDS budget, and the two
    blocks after it, which do not).  The image is not monotone in n: a block with many trailing zero bits has more
    finest partitions, so 16384 (256 partitions) already leaves LDS while most blocks up to this edge stay in it."""
    n = max(m for m in range(64, 32768) if search_lds_bytes(m) <= LDS_BUDGET)
    assert search_lds_bytes(n + 1) > LDS_BUDGET and search_lds_bytes(n + 2) > LDS_BUDGET
    return n, n + 1, n + 2


def zigzag(e):
    e = np.asarray(e, np.int64)
    return np.where(e < 0, -2 * e - 1, 2 * e).astype(np.uint64)


def candidate_branches(c, x, bps):
    """The branch set of one candidate (order_model.candidate's dict) of subframe x: see branches."""
    if c["status"] != om.STATUS_OK:
        return {"status"}
    n = len(x)
    fo = finest_order(n)
    psize = n >> fo
    maxabs = int(np.max(np.abs(np.asarray(x, np.int64)))) if n else 0
    out = set()
    qp = c["qp"]
    sumabs = int(np.sum(np.abs(np.asarray(qp.coefs[:32], np.int64))))
    out.add("i24" if maxabs * sumabs < 0x7FFFFFFF and maxabs < (1 << 23) else "i64")
    u = zigzag(c["residual"])
    u[:qp.order] = 0
    wide = int(u.max()) >= (1 << 27)
    if wide:
        out.add("wide")
    elif max(int(u[i * psize:(i + 1) * psize].sum()) for i in range(1 << fo)) >= (1 << 32):
        out.add("ksat")
    params = [int(p) for p in c["rice_params"]]
    if max(params) > 14:
        out.add("rice2")
    nb = 1 << c["rice_order"]
    narrow = 8 + bps * qp.order + 9 + qp.precision * qp.order + 6 + c["code_bits"] + (nb if max(params) > 14 else 0)
    if not wide and narrow != c["subframe_bits"]:
        out.add("clamp")
    return out


def branches_by_candidate(x, bps, cfg, extras, orders):
    """Which branches order_search_kernel takes on every candidate of window_model.search, in kernel order
    (c = j * Pc + ...): a list of sets of 'i24' (v_mad_i32_i24 residuals), 'i64' (64-bit residuals), 'wide' (zig-zag
    codes of 2^27 and more), 'ksat' (a finest partition's sum of codes reaches 2^32, codes below 2^27), 'clamp' (the
    chosen level's table sum differs from the exact bits: a saturated entry), 'rice2' (a chosen parameter above 14),
    'status' (a non-zero status)."""
    import window_model as wm
    x = np.ascontiguousarray(x, np.int32)
    _, cands = wm.search(x, bps, cfg, extras, orders)
    return [candidate_branches(c, x, bps) for c in cands]


def regime(b):
    """One letter per candidate's key regime: W wide, K kSat alone, C clamp, . an ordinary candidate."""
    return "W" if "wide" in b else "C" if "clamp" in b else "K" if "ksat" in b else "."


def regimes(x, bps, cfg, extras, orders):
    return "".join(regime(b) for b in branches_by_candidate(x, bps, cfg, extras, orders))


def branches(x, bps, cfg):
    """The union of branches_by_candidate over the one-window case with every order: what the order search alone
    reaches on one subframe."""
    return set().union(*branches_by_candidate(x, bps, cfg, (), True))
