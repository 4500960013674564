"""A model of FLACENC_HIP_FLAG_WASTED_BITS on top of the oracle: per subframe signal x of width w, Constant (k = 0) when
use_constant and x is constant, else k = the trailing zero bits of the OR of x (0 when that OR is 0) and the subframe is
oracle.encode_subframe(x >> k, w - k) at count_bits + k; try_stereo_coding compares those counts.  Frames are written
with flac_write (the oracle's writer has no wasted bits).  flac_parse asserts that frames carry no wasted bits, so these
frames are read back with the decoder instead."""
import numpy as np

import flac_write
from oracle import oracle

STEREO_TAGS = {0: 1, 1: 8, 2: 9, 3: 10}  # channel assignment -> header channel code (bitrepr.rs:329-356)
STEREO_ROLES = {0: (0, 1), 1: (0, 3), 2: (3, 1), 3: (2, 3)}  # select_channels, datatype.rs:1173-1185


def frame_config(order=8, use_fixed=True, use_constant=True, stereo=True, **qlpc):
    """The oracle's frame config (its sums are the stable build's: FLACENC_HIP_FLAG_REFERENCE_SUM_ORDER's integers, and
    the unflagged ones on the shapes the GPU tests use); `qlpc`: more oracle.make_config keywords."""
    return oracle.make_frame_config(oracle.make_config(lpc_order=order, **qlpc), use_constant=use_constant,
                                    use_fixed=use_fixed, use_leftside=stereo, use_rightside=stereo, use_midside=stereo)


def wasted_of(x, fc) -> int:
    x = np.asarray(x, np.int64)
    if fc.use_constant and len(x) and np.all(x == x[0]):
        return 0
    o = int(np.bitwise_or.reduce(x)) if len(x) else 0
    if o == 0:
        return 0
    return (o & -o).bit_length() - 1


def subframe(x, w, fc, wasted=True) -> dict:
    """encode_subframe under the flag (wasted=False: today's) -> {"bits", "k", "enc", "w"}."""
    x = np.ascontiguousarray(x, np.int32)
    k = wasted_of(x, fc) if wasted else 0
    enc = oracle.encode_subframe(x >> k, w - k, fc)
    return {"bits": enc["bits"] + k, "k": k, "enc": enc, "w": w, "x": x}


def roles(l, r):
    l = np.asarray(l, np.int64)
    r = np.asarray(r, np.int64)
    return [l, r, (l + r) >> 1, l - r]


def stereo_decision(l, r, bps, fc, wasted=True):
    """-> (assignment, [subframe of L, R, M, S])"""
    subs = [subframe(x, bps + (1 if i == 3 else 0), fc, wasted) for i, x in enumerate(roles(l, r))]
    b = [s["bits"] for s in subs]
    best, assignment = b[0] + b[1], 0
    if fc.use_leftside and b[0] + b[3] < best:
        best, assignment = b[0] + b[3], 1
    if fc.use_rightside and b[1] + b[3] < best:
        best, assignment = b[1] + b[3], 2
    if fc.use_midside and b[2] + b[3] < best:
        best, assignment = b[2] + b[3], 3
    return assignment, subs


def stereo_bits(l, r, bps, fc, wasted=True) -> int:
    """Sum of the two chosen subframes' bits."""
    a, subs = stereo_decision(l, r, bps, fc, wasted)
    return sum(subs[i]["bits"] for i in STEREO_ROLES[a])


def _write_args(s) -> dict:
    """flac_write.write_subframe keywords for one modelled subframe."""
    enc, k = s["enc"], s["k"]
    kind = enc["kind"]
    if kind == 0:
        return {"kind": "constant", "wasted": k}
    if kind == 1:
        return {"kind": "verbatim", "wasted": k}
    if kind == 2:
        order, porder = int(enc["fixed"].order), int(enc["fixed"].rice_order)
        extra = {"kind": "fixed", "order": order}
    else:
        qp = enc["lpc"].qp
        order, porder = int(qp.order), int(enc["lpc"].rice_order)
        extra = {"kind": "lpc", "order": order, "coefs": [int(c) for c in qp.coefs[:order]],
                 "precision": int(qp.precision), "shift": int(qp.shift)}
    params = [int(p) for p in enc["rice_params"][:1 << porder]]
    extra.update(wasted=k, porder=porder, params=params, method=1 if max(params) > 14 else 0)
    return extra


def stereo_frame_bytes(l, r, bps, fc, number=0) -> bytes:
    a, subs = stereo_decision(l, r, bps, fc)
    return flac_write.frame([l, r], STEREO_TAGS[a], bps, [_write_args(subs[i]) for i in STEREO_ROLES[a]], number=number)


def channel_frame_bytes(xs, bps, fc, number=0) -> bytes:
    """An Independent(len(xs)) frame."""
    subs = [subframe(x, bps, fc) for x in xs]
    return flac_write.frame(xs, len(xs) - 1, bps, [_write_args(s) for s in subs], number=number)
