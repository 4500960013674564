"""A model of FLACENC_HIP_FLAG_ORDER_SEARCH built from oracle calls: per LPC candidate subframe with lpc_order = P, R[0..P]
is the stable build's autocorrelation (estimated_qlpc's `autocorr` under ACORR_REFERENCE, or ACORR_NIGHTLY), and for every
o = 1..P the candidate is the Levinson recursion on R[0..o], quantize_parameters, compute_error and the exhaustive Rice
search; the one with status 0 and the smallest Lpc::count_bits wins (ties: the lower order), else the order-P record.
Frames apply encode_subframe's rules with that LPC candidate and try_stereo_coding, and are written by the oracle's
writer."""
import numpy as np

from oracle import oracle

STATUS_OK, STATUS_NONFINITE, STATUS_NEG_ENERGY = 0, 1, 2


def config(order=8, nightly=False, **kw):
    return oracle.make_config(lpc_order=order, acorr=oracle.ACORR_NIGHTLY if nightly else oracle.ACORR_REFERENCE, **kw)


def _max_p(cfg) -> int:
    return cfg.max_rice_parameter  # (oracle.RICE_FINEST_ONLY included)


def _levinson_status(R) -> int:
    """levinson_quantize's status checks on R[0..o] (lpc.rs:646-655, 786-791)."""
    if not np.all(np.isfinite(R)):
        return STATUS_NONFINITE
    if not R[0] >= 0.0:
        return STATUS_NEG_ENERGY
    if R[0] == 0.0 and np.any(R != 0.0):
        return STATUS_NEG_ENERGY
    return STATUS_OK


def candidate(x, bps, R, o, cfg) -> dict:
    """The order-o candidate from R[0..o]: status, o, coefs (unquantised) and, with status 0, qp, residual, rice_order,
    rice_params, code_bits, sum_quotients, subframe_bits (the exact Lpc::count_bits)."""
    Ro = np.ascontiguousarray(R[: o + 1], np.float64)
    st = _levinson_status(Ro)
    coefs = np.zeros(o, np.float64)
    if st == STATUS_OK and Ro[0] != 0.0:
        coefs, _ = oracle.symmetric_levinson_recursion(Ro[:o], Ro[1:o + 1])
        if not np.all(np.isfinite(coefs)):
            st = STATUS_NONFINITE
    out = {"status": st, "o": o, "coefs": coefs if st == STATUS_OK else np.zeros(o)}
    if st != STATUS_OK:
        return out
    qp = oracle.quantize_parameters(coefs, cfg.quant_precision)
    err = oracle.compute_error(qp, x)
    res = oracle.encode_residual(err, qp.order, _max_p(cfg))
    rbits = oracle.residual_count_bits(len(x), qp.order, res["partition_order"], res["rice_params"],
                                       res["sum_quotients"], res["sum_rice_params"])
    out.update(qp=qp, residual=err, rice_order=int(res["partition_order"]), rice_params=res["rice_params"],
               code_bits=int(res["code_bits"]), sum_quotients=int(res["sum_quotients"]),
               subframe_bits=oracle.lpc_count_bits(bps, qp.order, qp.precision, rbits))
    return out


def autocorr(x, bps, cfg) -> np.ndarray:
    """R[0..P] in the configured summation order (estimated_qlpc's own)."""
    return np.asarray(oracle.estimated_qlpc(np.ascontiguousarray(x, np.int32), bps, cfg)["autocorr"], np.float64)


def search(x, bps, cfg):
    """-> (the flagged LPC candidate, R[0..P], keys {o: subframe_bits, None where the status is not 0})."""
    x = np.ascontiguousarray(x, np.int32)
    R = autocorr(x, bps, cfg)
    cands = [candidate(x, bps, R, o, cfg) for o in range(1, cfg.lpc_order + 1)]
    keys = {c["o"]: (c["subframe_bits"] if c["status"] == STATUS_OK else None) for c in cands}
    ok = [c for c in cands if c["status"] == STATUS_OK]
    best = min(ok, key=lambda c: (c["subframe_bits"], c["o"])) if ok else cands[-1]
    return best, R, keys


def record(x, bps, cfg):
    """The candidate batch's outputs for one subframe: (record fields, residual row, autocorr [33], lpc_coefs [32])."""
    best, R, _ = search(x, bps, cfg)
    ac = np.zeros(33)
    ac[: len(R)] = R
    lc = np.zeros(32)
    if best["status"] != STATUS_OK:
        return {"status": int(best["status"])}, np.zeros(len(x), np.int32), ac, lc
    lc[: best["o"]] = best["coefs"]
    qp = best["qp"]
    rec = {"order": int(qp.order), "shift": int(qp.shift), "precision": int(qp.precision),
           "coefs": [int(c) for c in qp.coefs[:32]], "rice_order": best["rice_order"],
           "rice_params": [int(p) for p in best["rice_params"]], "status": 0, "code_bits": best["code_bits"],
           "subframe_bits": best["subframe_bits"], "sum_quotients": best["sum_quotients"]}
    return rec, best["residual"], ac, lc


def encode_subframe(x, bps, fc):
    """encode_subframe (coding.rs:384-418) with the flagged LPC candidate -> (kind, bits, oracle writer keywords)."""
    x = np.ascontiguousarray(x, np.int32)
    n = len(x)
    # Constant / FixedLpc / Verbatim as the oracle decides them without the LPC candidate
    rest = oracle.make_frame_config(fc.qlpc, use_constant=fc.use_constant, use_fixed=fc.use_fixed, use_lpc=False,
                                    fixed=fc.fixed)
    enc = oracle.encode_subframe(x, bps, rest)
    kind, bits = enc["kind"], enc["bits"]
    if kind == 0:
        return 0, bits, {"kind": 0, "bps": bps, "dc_offset": int(x[0])}
    verbatim = oracle.verbatim_count_bits(n, bps)
    if n >= 64 and fc.use_lpc:
        best, _, _ = search(x, bps, fc.qlpc)
        baseline = bits if kind == 2 else verbatim  # min(verbatim, fixed): a fixed candidate >= verbatim is not kind 2
        # est_lpc.or(fixed).filter(|sf| sf.count_bits() < verbatim_bits)
        if best["status"] == STATUS_OK and best["subframe_bits"] < baseline:
            qp = best["qp"]
            return 3, best["subframe_bits"], {
                "kind": 3, "bps": bps, "samples": x, "order": int(qp.order), "shift": int(qp.shift),
                "precision": int(qp.precision), "coefs": np.array(qp.coefs[:32], np.int16),
                "rice_order": best["rice_order"], "rice_params": best["rice_params"], "residual": best["residual"]}
    if kind == 2:
        f = enc["fixed"]
        return 2, bits, {"kind": 2, "bps": bps, "samples": x, "order": int(f.order), "rice_order": int(f.rice_order),
                         "rice_params": enc["rice_params"][:1 << int(f.rice_order)].copy(), "residual": enc["residual"]}
    return 1, bits, {"kind": 1, "bps": bps, "samples": x}


STEREO_ROLES = {0: (0, 1), 1: (0, 3), 2: (3, 1), 3: (2, 3)}  # select_channels, datatype.rs:1173-1185


def stereo_frame(l, r, bps, fc):
    """encode_frame for a 2-channel frame -> (assignment, [(kind, bits, writer keywords) of L, R, M, S])."""
    l = np.ascontiguousarray(l, np.int32)
    r = np.ascontiguousarray(r, np.int32)
    m, s = oracle.stereo_to_midside(l, r)
    subs = [encode_subframe(x, bps + (1 if k == 3 else 0), fc) for k, x in enumerate((l, r, m, s))]
    b = [x[1] for x in subs]
    best, a = b[0] + b[1], 0
    if fc.use_leftside and b[0] + b[3] < best:
        best, a = b[0] + b[3], 1
    if fc.use_rightside and b[1] + b[3] < best:
        best, a = b[1] + b[3], 2
    if fc.use_midside and b[2] + b[3] < best:
        best, a = b[2] + b[3], 3
    return a, subs


def stereo_bits(l, r, bps, fc) -> int:
    a, subs = stereo_frame(l, r, bps, fc)
    return sum(subs[k][1] for k in STEREO_ROLES[a])


def stereo_frame_bytes(l, r, bps, fc, number=0, sample_rate=44100) -> bytes:
    a, subs = stereo_frame(l, r, bps, fc)
    return oracle.write_frame(len(l), a, bps, sample_rate, number, [subs[k][2] for k in STEREO_ROLES[a]])


def channel_frame_bytes(xs, bps, fc, number=0, sample_rate=44100) -> bytes:
    """An Independent(len(xs)) frame."""
    subs = [encode_subframe(x, bps, fc)[2] for x in xs]
    return oracle.write_frame(len(xs[0]), 0, bps, sample_rate, number, subs)


# ---- composed with FLACENC_HIP_FLAG_WASTED_BITS (tests/wasted_model.py) ----
def wasted_subframe(x, w, fc) -> dict:
    """encode_subframe under both flags: k = wasted_model.wasted_of(x), then encode_subframe(x >> k, w - k) with the
    flagged LPC candidate, at its bits + k."""
    import wasted_model
    x = np.ascontiguousarray(x, np.int32)
    k = wasted_model.wasted_of(x, fc)
    kind, bits, kw = encode_subframe(x >> k, w - k, fc)
    return {"kind": kind, "bits": bits + k, "k": k, "kw": kw}


def _flac_write_args(s) -> dict:
    """flac_write.write_subframe keywords for one composed subframe."""
    kind, kw, k = s["kind"], s["kw"], s["k"]
    if kind == 0:
        return {"kind": "constant", "wasted": k}
    if kind == 1:
        return {"kind": "verbatim", "wasted": k}
    porder = int(kw["rice_order"])
    params = [int(p) for p in kw["rice_params"][:1 << porder]]
    out = {"kind": "fixed" if kind == 2 else "lpc", "order": int(kw["order"]), "wasted": k, "porder": porder,
           "params": params, "method": 1 if max(params) > 14 else 0}
    if kind == 3:
        out.update(coefs=[int(c) for c in kw["coefs"][:int(kw["order"])]], precision=int(kw["precision"]),
                   shift=int(kw["shift"]))
    return out


def wasted_stereo_frame_bytes(l, r, bps, fc, number=0) -> bytes:
    """A 2-channel frame under both flags, written by flac_write (the oracle's writer has no wasted bits)."""
    import flac_write
    import wasted_model
    subs = [wasted_subframe(x, bps + (1 if k == 3 else 0), fc) for k, x in enumerate(wasted_model.roles(l, r))]
    b = [s["bits"] for s in subs]
    best, a = b[0] + b[1], 0
    if fc.use_leftside and b[0] + b[3] < best:
        best, a = b[0] + b[3], 1
    if fc.use_rightside and b[1] + b[3] < best:
        best, a = b[1] + b[3], 2
    if fc.use_midside and b[2] + b[3] < best:
        best, a = b[2] + b[3], 3
    return flac_write.frame([l, r], wasted_model.STEREO_TAGS[a], bps, [_flac_write_args(subs[k]) for k in STEREO_ROLES[a]],
                            number=number)


def wasted_channel_frame_bytes(xs, bps, fc, number=0) -> bytes:
    """An Independent(len(xs)) frame under both flags."""
    import flac_write
    subs = [wasted_subframe(x, bps, fc) for x in xs]
    return flac_write.frame(xs, len(xs) - 1, bps, [_flac_write_args(s) for s in subs], number=number)
