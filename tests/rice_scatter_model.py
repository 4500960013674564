"""The fused 4096 kernel's partitioned-Rice search as index arithmetic over its 64 lanes (numpy, batched over blocks).

Lane l holds the 64-sample finest partition l of a 4096-sample residual block; lane 0's first `warm` slots are warm-up
samples and are not coded.  `search()` mirrors phase 4 of qlpc_wave_kernel_impl.h: the parameter window from the lane
means, the path predicate, the reduce-scatter search of the common case (tagged entries  E_j = (W_j << 8) + j,  two
scatter steps inside the quad, the group's table on its first quad from level 3 on) and the clamped search everything
else takes.  It returns, per block, the chosen partition order, the group leaders' parameters and PrcParameter::code_bits
-- what oracle.find_partitioned_rice_parameter returns -- plus the classification the tests assert on."""
import numpy as np

MAX_P_TO_BITS = (1 << 27) - 1
W_MAX = MAX_P_TO_BITS - 4
LANES = 64
SPL = 64
NP = 4  # entries of the one group the fast path evaluates


def zigzag(e):
    e = np.asarray(e, np.int64)
    return np.where(e >= 0, 2 * e, -2 * e - 1).astype(np.uint32)


def _floor_log2(q):
    q = np.asarray(q, np.uint64)
    out = np.zeros(q.shape, np.int64)
    for b in (32, 16, 8, 4, 2, 1):
        big = q >= (np.uint64(1) << np.uint64(b))
        out += np.where(big, b, 0)
        q = np.where(big, q >> np.uint64(b), q)
    return out


def window(u, warm, max_rice_parameter):
    """u: (B, 64, 64) zig-zag codes (warm-up slots 0).  -> dict of per-block window quantities, as the kernel has them."""
    s0 = u.sum(axis=2, dtype=np.uint64)  # (B, 64)
    maxu = u.reshape(u.shape[0], -1).max(axis=1).astype(np.uint64)
    bitlen = np.where(maxu > 0, _floor_log2(np.maximum(maxu, 1)) + 1, 0)
    max_p = np.minimum(max_rice_parameter, bitlen)
    small_bits = max_rice_parameter >= bitlen
    q0 = (s0 >> np.uint64(6)) + np.uint64(1)
    p0min = _floor_log2(q0).min(axis=1)
    q0hi = q0.copy()
    q0hi[:, 0] += (s0[:, 0] >> np.uint64(8)) + np.uint64(1)
    p0max = _floor_log2(q0hi).max(axis=1)
    p_lo = np.minimum(np.maximum(p0min - 1, 0), max_p)
    p_hi = np.minimum(p0max + 1, max_p)
    fast = small_bits & (p0max - p0min <= 1) & (maxu < (1 << 26))
    return dict(s0=s0, maxu=maxu, bitlen=bitlen, max_p=max_p, small_bits=small_bits, p0min=p0min, p0max=p0max,
                p_lo=p_lo, p_hi=p_hi, fast=fast)


def _lane_sums(u, p):
    """sum over a lane's samples of (u >> p), p per block: (B, 64)."""
    return (u >> p.astype(np.uint32)[:, None, None]).sum(axis=2, dtype=np.uint64)


def fast_path(u, warm, p_lo):
    """The reduce-scatter search.  -> (pk (B, 7, 64) minima per level and lane, totals (B, 7), bound_ok, the lanes'
    untagged entries W (B, 64, 4))."""
    B = u.shape[0]
    lane = np.arange(LANES)
    len0 = np.full(LANES, SPL, np.uint64)
    len0[0] = SPL - warm
    E = np.zeros((B, LANES, NP), np.uint64)
    for j in range(NP):
        p = p_lo + j
        W = _lane_sums(u, p) + len0[None, :] * (p[:, None].astype(np.uint64) + np.uint64(1))
        E[:, :, j] = (W << np.uint64(8)) + np.uint64(j)
    bound_ok = bool((E < (1 << 20)).all())  # per lane: W < 512 + 64 * 32
    pk = np.zeros((B, 7, LANES), np.uint64)
    pk[:, 0] = E.min(axis=2)
    # level 1: the lanes of a pair trade halves; even lanes keep entries {0, 1}, odd lanes {2, 3}
    odd = (lane & 1) != 0
    keep = np.where(odd[None, :, None], E[:, :, 2:4], E[:, :, 0:2])
    send = np.where(odd[None, :, None], E[:, :, 0:2], E[:, :, 2:4])
    a = keep + send[:, lane ^ 1, :]  # (B, 64, 2)
    m = a.min(axis=2)
    pk[:, 1] = np.minimum(m, m[:, lane ^ 1])
    # level 2: the pairs of a quad trade; every lane keeps one entry, number 2 (lane & 1) + ((lane >> 1) & 1)
    second = (lane & 2) != 0
    keep1 = np.where(second[None, :], a[:, :, 1], a[:, :, 0])
    send1 = np.where(second[None, :], a[:, :, 0], a[:, :, 1])
    t = keep1 + send1[:, lane ^ 2]
    entry = 2 * (lane & 1) + ((lane >> 1) & 1)

    def quad_min(v):
        v = np.minimum(v, v[:, lane ^ 1])
        return np.minimum(v, v[:, lane ^ 2])

    pk[:, 2] = quad_min(t)
    for K, S in ((3, 4), (4, 8), (5, 16), (6, 32)):
        t = t + t[:, (lane + S) % LANES]  # meaningful on the first quad of every group of 2 S lanes
        pk[:, K] = quad_min(t)
    # the tag of entry j at level K is j 2^K: check it on the lanes that hold a valid table
    assert ((t[:, :4] & np.uint64(255)) == (entry[:4] << 6).astype(np.uint64)[None, :]).all()
    tot = np.zeros((B, 7), np.uint64)
    for K in range(7):
        tot[:, K] = ((pk[:, K, ::1 << K] >> np.uint64(8)) + np.uint64(4)).sum(axis=1)
    return pk, tot, bound_ok, (E >> np.uint64(8))


def clamped_path(u, warm, p_lo, p_hi, max_p):
    """rice_search<true> over [p_lo, p_hi] with the reference's clamps; full range again if a minimum saturated.
    -> (pk (B, 7, 64) packed minima (W << 5 | p), totals (B, 7))."""
    B = u.shape[0]
    len0 = np.full(LANES, SPL, np.uint64)
    len0[0] = SPL - warm

    def run(lo, hi):
        pk = np.full((B, 7, LANES), np.iinfo(np.uint64).max, np.uint64)
        for p in range(int(lo.min()), int(hi.max()) + 1):
            inwin = (p >= lo) & (p <= hi)
            s = np.minimum((u >> np.uint32(p)).sum(axis=2, dtype=np.uint64), MAX_P_TO_BITS)
            W = np.minimum(s + len0[None, :] * np.uint64(p + 1), W_MAX)
            W = np.where((p <= max_p)[:, None], W, W_MAX)
            for K in range(7):
                if K > 0:
                    W = np.minimum(W[:, 0::2] + W[:, 1::2], W_MAX)
                c = (W << np.uint64(5)) | np.uint64(p)
                c = np.where(inwin[:, None], c, np.iinfo(np.uint64).max)
                pk[:, K, ::1 << K] = np.minimum(pk[:, K, ::1 << K], c)
        return pk

    pk = run(p_lo, p_hi)
    sat = np.zeros(B, bool)
    for K in range(7):
        sat |= (((pk[:, K, ::1 << K] >> np.uint64(5)) + np.uint64(4)) >= MAX_P_TO_BITS).any(axis=1)
    redo = sat & (p_lo != 0)
    if redo.any():
        sub = clamped_path(u[redo], warm, np.zeros(int(redo.sum()), np.int64), max_p[redo], max_p[redo])
        pk[redo] = sub[0]
    tot = np.zeros((B, 7), np.uint64)
    for K in range(7):
        tot[:, K] = ((pk[:, K, ::1 << K] >> np.uint64(5)) + np.uint64(4)).sum(axis=1)
    return pk, tot


def search(blocks, warm, max_rice_parameter=30):
    """blocks: (B, 4096) int32 residuals, slots [0, warm) zero.  -> list of dicts, one per block."""
    blocks = np.asarray(blocks, np.int32)
    B = blocks.shape[0]
    u = zigzag(blocks).reshape(B, LANES, SPL)
    u[:, 0, :warm] = 0
    w = window(u, warm, max_rice_parameter)
    out = [None] * B
    for fast in (True, False):
        idx = np.nonzero(w["fast"] == fast)[0]
        if len(idx) == 0:
            continue
        if fast:
            pk, tot, ok, W = fast_path(u[idx], warm, w["p_lo"][idx])
            assert ok
            shift, mask = 8, 255
        else:
            pk, tot = clamped_path(u[idx], warm, w["p_lo"][idx], w["p_hi"][idx], w["max_p"][idx])
            shift, mask = 5, 31
        for n, b in enumerate(idx):
            bestk = int(np.argmin(tot[n]))  # first minimum: ties keep the finer order
            lead = pk[n, bestk, ::1 << bestk]
            if fast:
                params = int(w["p_lo"][b]) + ((lead & np.uint64(mask)) >> np.uint64(bestk))
            else:
                params = lead & np.uint64(mask)
            best = int(tot[n, bestk])
            param_tie = False
            if fast:  # two parameters with the same, minimal, entry in a group's table of the chosen order
                g = np.sort(W[n].reshape(LANES >> bestk, 1 << bestk, NP).sum(axis=1), axis=1)
                param_tie = bool((g[:, 0] == g[:, 1]).any())
            out[b] = dict(
                order=6 - bestk, params=params.astype(np.uint8), code_bits=best, fast=fast,
                width=int(w["p_hi"][b] - w["p_lo"][b] + 1), p0min=int(w["p0min"][b]), p0max=int(w["p0max"][b]),
                param_tie=param_tie, order_tie=int((tot[n] == np.uint64(best)).sum()) > 1, pk=pk[n], bestk=bestk, p_lo=int(w["p_lo"][b]))
    return out


def is_fast(blocks, warm, max_rice_parameter=30):
    """The path predicate alone (the data-dependent part: the kernel adds !FIXED, 64 samples per lane, !finest_only)."""
    blocks = np.asarray(blocks, np.int32)
    u = zigzag(blocks).reshape(blocks.shape[0], LANES, SPL)
    u[:, 0, :warm] = 0
    return window(u, warm, max_rice_parameter)["fast"]
