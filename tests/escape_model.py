"""FLACENC_HIP_FLAG_RICE_ESCAPE stated in Python (include/flacenc_hip.h has the definition).

The Rice side is the oracle's: orc_prc_bit_table_from_errors at the finest level, orc_prc_merge below it,
orc_prc_minimizer for every partition, orc_finest_partition_order for the level to start from.  This module adds the raw
width of a partition, the escape cost, the strict choice, the walk over the levels on sum_q min(R, E), the exact bit
count and a way from a record to bytes through tests/flac_write.py, which writes ("esc", width) partitions.

search(e, order, ..., escape=False) is the reference's search restated on the same calls: tests/test_rice_escape_cpu.py
holds it to orc_find_partitioned_rice_parameter before anything else is believed."""
import numpy as np

import flac_write as fw
from oracle import oracle as orc

MARK = 0x80
MAX_WIDTH = 31


def zigzag(e):
    e = np.asarray(e, np.int64)
    return np.where(e < 0, -2 * e - 1, 2 * e).astype(np.uint32)


def raw_width(e):
    """The smallest w with -2^(w-1) <= v < 2^(w-1) for every v; 0 for all zeros or no samples."""
    e = np.asarray(e, np.int64)
    if e.size == 0 or not e.any():
        return 0
    lo, hi = int(e.min()), int(e.max())
    w = 1
    while not (-(1 << (w - 1)) <= lo and hi < (1 << (w - 1))):
        w += 1
    return w


def escape_cost(cnt, w):
    return 4 + 5 + cnt * w if w <= MAX_WIDTH else None


def bounds(n, order, level):
    size = n >> level
    return [(max(q * size, order), (q + 1) * size) for q in range(1 << level)]


def search(e, order, max_p=30, escape=True, finest_only=False):
    """-> dict(rice_order, params: per partition an int or ("esc", w), code_bits, sum_quotients, residual_bits,
    escaped: how many partitions of the chosen level are escaped)."""
    e = np.asarray(e, np.int64)
    n = len(e)
    z = zigzag(e)
    level = orc.finest_partition_order(n, max(64, order))
    tables = [orc.prc_bit_table_from_errors(z[a:b], 4) for a, b in bounds(n, order, level)]
    widths = [raw_width(e[a:b]) for a, b in bounds(n, order, level)]
    best = None
    while True:
        cost, params = 0, []
        for q, (a, b) in enumerate(bounds(n, order, level)):
            k, r = orc.prc_minimizer(tables[q], max_p)
            ec = escape_cost(b - a, widths[q]) if escape else None
            if ec is not None and ec < r:                         # strictly: a tie stays Rice
                cost += ec
                params.append(("esc", widths[q]))
            else:
                cost += r
                params.append(int(k))
        if best is None or cost < best[0]:
            best = (cost, level, params)
        if level == 0 or finest_only:
            break
        tables = [orc.prc_merge(tables[2 * q], tables[2 * q + 1], 4) for q in range(len(tables) // 2)]
        widths = [max(widths[2 * q], widths[2 * q + 1]) for q in range(len(widths) // 2)]
        level -= 1
    cost, level, params = best
    out = dict(rice_order=level, params=params, code_bits=cost)
    out["sum_quotients"], out["residual_bits"] = count(e, order, level, params)
    out["escaped"] = sum(isinstance(p, tuple) for p in params)
    return out


def count(e, order, level, params):
    """(sum of z >> k over the non-escaped partitions, the residual's exact bits in Residual::write)."""
    e = np.asarray(e, np.int64)
    z = zigzag(e).astype(np.int64)
    pb = 5 if any(not isinstance(p, tuple) and p > 14 for p in params) else 4
    bits, sq = 2 + 4, 0
    for (a, b), p in zip(bounds(len(e), order, level), params):
        if isinstance(p, tuple):
            bits += pb + 5 + (b - a) * p[1]
        else:
            s = int((z[a:b] >> p).sum())
            sq += s
            bits += pb + s + (b - a) * (p + 1)
    return sq, bits


def head_bits(kind, bps, order, precision):
    """Everything of FixedLpc::count_bits / Lpc::count_bits in front of the residual."""
    return 8 + order * bps + (4 + 5 + order * precision if kind == "lpc" else 0)


def param_bytes(params):
    """rice_params[256] of the record: 0x80 | w for an escaped partition, zeros behind the last one."""
    out = np.zeros(256, np.uint8)
    for q, p in enumerate(params):
        out[q] = (MARK | p[1]) if isinstance(p, tuple) else p
    return out


def params_from_bytes(raw, level):
    return [("esc", int(b) & 31) if int(b) & MARK else int(b) for b in np.asarray(raw)[:1 << level]]


def flagged_record(rec, e, kind, bps, max_p=30, finest_only=False):
    """The record the flag makes of a candidate record `rec` (a PARAMS_DTYPE scalar with status 0, as the unflagged
    call returns it) and its residual row: a copy with the five fields rewritten when a partition escapes, `rec` itself
    otherwise.  -> (record, the search's dict)."""
    out = rec.copy()
    if int(rec["status"]) != 0:
        return out, None
    order = int(rec["order"])
    m = search(e, order, max_p, True, finest_only)
    if m["escaped"]:
        out["rice_order"] = m["rice_order"]
        out["rice_params"] = param_bytes(m["params"])
        out["code_bits"] = m["code_bits"]
        out["sum_quotients"] = m["sum_quotients"]
        out["subframe_bits"] = head_bits(kind, bps, order, int(rec["precision"])) + m["residual_bits"]
    return out, m


def residual_bytes(e, order, level, params):
    """The residual as tests/flac_write.py writes it, padded to a byte (RICE2 iff a non-escaped parameter > 14)."""
    method = 1 if any(not isinstance(p, tuple) and p > 14 for p in params) else 0
    w = fw.BitWriter()
    fw.write_residual(w, np.asarray(e, np.int64), order, len(e), method, level, list(params))
    nbits = len(w.bits)
    w.align()
    return w.bytes(), nbits


# ---------------------------------------------------------------- encode_subframe / try_stereo_coding under the flag
STEREO_TAGS = {0: 1, 1: 8, 2: 9, 3: 10}
STEREO_ROLES = {0: (0, 1), 1: (0, 3), 2: (3, 1), 3: (2, 3)}      # select_channels, datatype.rs:1173-1185
FINEST_ONLY = 0x100                                               # oracle.RICE_FINEST_ONLY inside max_rice_parameter


def _candidate(kind, w, order, precision, residual, rice_order, rice_params, code_bits, sum_quotients, subframe_bits,
               max_p, escape, **more):
    """One candidate of encode_subframe (the oracle's, unflagged) -> the same with the escape search's fields."""
    c = dict(kind=kind, order=order, precision=precision, residual=np.asarray(residual, np.int64), rice_order=rice_order,
             params=[int(p) for p in rice_params[:1 << rice_order]], code_bits=code_bits, sum_quotients=sum_quotients,
             bits=subframe_bits, escaped=0, **more)
    if escape:
        m = search(c["residual"], order, max_p & 0xFF, True, bool(max_p & FINEST_ONLY))
        if m["escaped"]:
            c.update(rice_order=m["rice_order"], params=m["params"], code_bits=m["code_bits"],
                     sum_quotients=m["sum_quotients"], escaped=m["escaped"],
                     bits=head_bits(kind, w, order, precision) + m["residual_bits"])
    return c


def subframe(x, w, fc, escape=True, analyse=None):
    """encode_subframe (coding.rs:384-418) on the oracle's candidates with the flag's bit counts: Constant first, the
    LPC candidate if it beats min(fixed, verbatim), the fixed candidate if its selector key and its count are below
    Verbatim, else Verbatim.  -> dict(kind 0..3, bits, cand: the kept candidate or None, x, w, status: the LPC
    analysis's).  `analyse(x, w, qlpc config)`: what states the LPC candidate in place of oracle.estimated_qlpc, with
    its keys (a search flag's winner, chosen unescaped: the escape pass runs on the winner alone)."""
    x = np.ascontiguousarray(x, np.int32)
    n = len(x)
    verbatim = orc.verbatim_count_bits(n, w)
    out = dict(x=x, w=w, cand=None, status=0)
    max_p = fc.qlpc.max_rice_parameter
    lpc = fixed = None
    if n >= 64 and fc.use_lpc:
        r = (analyse or orc.estimated_qlpc)(x, w, fc.qlpc)
        out["status"] = int(r["status"])
        if r["status"] == 0:
            lpc = _candidate("lpc", w, int(r["order"]), int(r["precision"]), r["residual"], int(r["rice_order"]),
                             r["rice_params"], r["code_bits"], r["sum_quotients"], r["subframe_bits"], max_p, escape,
                             coefs=[int(c) for c in r["coefs"]], shift=int(r["shift"]))
    if fc.use_constant and np.all(x == x[0]):
        return dict(out, kind=0, bits=8 + w)
    if n >= 64 and fc.use_fixed:
        r = orc.fixed_lpc(x, w, verbatim, fc.fixed, max_p)
        if r["selected"]:                                         # the selector's key < Verbatim, as without the flag
            fixed = _candidate("fixed", w, r["order"], 0, r["residual"], r["rice_order"], r["rice_params"],
                               r["code_bits"], r["sum_quotients"], r["subframe_bits"], max_p, escape)
    fixed_bits = fixed["bits"] if fixed else 1 << 64
    if lpc and lpc["bits"] < min(fixed_bits, verbatim):
        return dict(out, kind=3, bits=lpc["bits"], cand=lpc)
    if fixed and fixed_bits < verbatim:
        return dict(out, kind=2, bits=fixed_bits, cand=fixed)
    return dict(out, kind=1, bits=verbatim)


def roles(l, r):
    l = np.asarray(l, np.int64)
    r = np.asarray(r, np.int64)
    return [l, r, (l + r) >> 1, l - r]


def stereo_decision(l, r, bps, fc, escape=True, analyse=None):
    """-> (assignment, [subframe of L, R, M, S])"""
    subs = [subframe(x, bps + (1 if i == 3 else 0), fc, escape, analyse) for i, x in enumerate(roles(l, r))]
    b = [s["bits"] for s in subs]
    best, assignment = b[0] + b[1], 0
    if fc.use_leftside and b[0] + b[3] < best:
        best, assignment = b[0] + b[3], 1
    if fc.use_rightside and b[1] + b[3] < best:
        best, assignment = b[1] + b[3], 2
    if fc.use_midside and b[2] + b[3] < best:
        best, assignment = b[2] + b[3], 3
    return assignment, subs


def write_args(s, wasted=0):
    """flac_write.write_subframe keywords of a modelled subframe."""
    if s["kind"] == 0:
        return {"kind": "constant", "wasted": wasted}
    if s["kind"] == 1:
        return {"kind": "verbatim", "wasted": wasted}
    c = s["cand"]
    kw = dict(kind=c["kind"], order=c["order"], porder=c["rice_order"], params=list(c["params"]), wasted=wasted,
              method=1 if any(not isinstance(p, tuple) and p > 14 for p in c["params"]) else 0)
    if c["kind"] == "lpc":
        kw.update(coefs=c["coefs"], precision=c["precision"], shift=c["shift"])
    return kw


def stereo_frame_bytes(l, r, bps, fc, number=0, escape=True, analyse=None):
    a, subs = stereo_decision(l, r, bps, fc, escape, analyse)
    return fw.frame([l, r], STEREO_TAGS[a], bps, [write_args(subs[i]) for i in STEREO_ROLES[a]], number=number)


def channel_frame_bytes(xs, bps, fc, number=0, escape=True, analyse=None):
    subs = [subframe(x, bps, fc, escape, analyse) for x in xs]
    return fw.frame(xs, len(xs) - 1, bps, [write_args(s) for s in subs], number=number)


def check_record(rec, s, where):
    """A predictor record of a frame-level result (PARAMS_DTYPE scalar) against the modelled subframe's candidate."""
    c = s["cand"]
    got = (int(rec["order"]), int(rec["precision"]), int(rec["rice_order"]), list(rec["rice_params"]),
           int(rec["code_bits"]), int(rec["subframe_bits"]), int(rec["sum_quotients"]), int(rec["status"]))
    want = (c["order"], c["precision"], c["rice_order"], list(param_bytes(c["params"])), c["code_bits"], c["bits"],
            c["sum_quotients"], 0)
    assert got == want, (where, got[:3], want[:3], got[4:], want[4:])
    if c["kind"] == "lpc":
        assert [int(v) for v in rec["coefs"][:c["order"]]] == c["coefs"] and int(rec["shift"]) == c["shift"], where
