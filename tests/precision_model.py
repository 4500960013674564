"""A model of FLACENC_HIP_FLAG_PRECISION_SEARCH built from oracle calls (include/flacenc_hip.h states the rule): per LPC
candidate subframe with lpc_order = P and quant_precision = q0, the (window j, order o) list is window_model's -- with
FLACENC_HIP_FLAG_ORDER_GUESS guess_model's, whose guesses keep q = q0 in their cost -- and every (j, o) is coded by
order_model.candidate at each precision q_i = q0 - i, i = 0 .. Q-1 (Q = q0 - F + 1 for a floor F < q0, else 1) under a
copy of the config with quant_precision = q_i.  The candidate with status 0 and the smallest Lpc::count_bits wins, ties to
the lower window, then the lower order, then the higher precision; with none it is (0, P, q0).  Frames and wasted bits are
window_model's."""
import numpy as np

import guess_model as gm
import order_model as om
import window_model as wm
from oracle import oracle

DEFAULT_FLOOR = 5


def precisions(q0, floor=DEFAULT_FLOOR) -> list:
    """q_0 .. q_(Q-1), descending."""
    return list(range(q0, floor - 1, -1)) if floor < q0 else [q0]


def at_precision(cfg, q):
    """A copy of an oracle config with quant_precision = q."""
    return oracle.QlpcConfig(cfg.lpc_order, q, cfg.window_type, cfg.tukey_alpha, cfg.max_rice_parameter, cfg.acorr_order)


def search(x, bps, cfg, floor=DEFAULT_FLOOR, extras=(), orders=False, K=0):
    """-> (the flagged LPC candidate with "j", "R" and "q", every coded candidate in kernel order).  extras / orders:
    FLACENC_HIP_FLAG_WINDOW_SEARCH's list / FLACENC_HIP_FLAG_ORDER_SEARCH as well; K > 0: FLACENC_HIP_FLAG_ORDER_GUESS
    with K guesses per window (then `orders` is not read)."""
    x = np.ascontiguousarray(x, np.int32)
    P, q0 = cfg.lpc_order, cfg.quant_precision
    grid = gm.search(x, bps, cfg, K, extras)[1] if K else wm.search(x, bps, cfg, extras, orders)[1]
    cands = []
    for c in grid:  # the candidates at q0, in (j, o) order
        c["q"] = q0
        cands.append(c)
        for q in precisions(q0, floor)[1:]:
            d = om.candidate(x, bps, c["R"], c["o"], at_precision(cfg, q))
            d.update(j=c["j"], R=c["R"], q=q)
            cands.append(d)
    ok = [c for c in cands if c["status"] == om.STATUS_OK]
    fallback = next(c for c in cands if c["j"] == 0 and c["o"] == P and c["q"] == q0)
    best = min(ok, key=lambda c: (c["subframe_bits"], c["j"], c["o"], -c["q"])) if ok else fallback
    return best, cands


def record(x, bps, cfg, floor=DEFAULT_FLOOR, extras=(), orders=False, K=0):
    """The candidate batch's outputs for one subframe: (record fields, residual row, autocorr [33], lpc_coefs [32])."""
    best, _ = search(x, bps, cfg, floor, extras, orders, K)
    ac = np.zeros(33)
    ac[: cfg.lpc_order + 1] = best["R"]
    lc = np.zeros(32)
    if best["status"] != om.STATUS_OK:
        return {"status": int(best["status"])}, np.zeros(len(x), np.int32), ac, lc
    lc[: best["o"]] = best["coefs"]
    qp = best["qp"]
    assert int(qp.precision) == best["q"]
    rec = {"order": int(qp.order), "shift": int(qp.shift), "precision": int(qp.precision),
           "coefs": [int(c) for c in qp.coefs[:32]], "rice_order": best["rice_order"],
           "rice_params": [int(p) for p in best["rice_params"]], "status": 0, "code_bits": best["code_bits"],
           "subframe_bits": best["subframe_bits"], "sum_quotients": best["sum_quotients"]}
    return rec, best["residual"], ac, lc


def record_fn(floor=DEFAULT_FLOOR, extras=(), orders=False, K=0):
    """extreme_signals.check_rows' record function for one floor and one set of the other search flags."""
    return lambda x, bps, cfg: record(x, bps, cfg, floor, extras, orders, K)


class Model(wm.Model):
    """encode_subframe / encode_frame with the flagged LPC candidate: window_model.Model's frames, assignment and wasted
    bits around this module's search."""

    def __init__(self, floor=DEFAULT_FLOOR, extras=(), orders=False, K=0):
        super().__init__(extras, orders)
        self.floor, self.K = floor, K

    def encode_subframe(self, x, bps, fc):
        x = np.ascontiguousarray(x, np.int32)
        n = len(x)
        rest = oracle.make_frame_config(fc.qlpc, use_constant=fc.use_constant, use_fixed=fc.use_fixed, use_lpc=False,
                                        fixed=fc.fixed)
        enc = oracle.encode_subframe(x, bps, rest)
        kind, bits = enc["kind"], enc["bits"]
        if kind == 0:
            return 0, bits, {"kind": 0, "bps": bps, "dc_offset": int(x[0])}
        verbatim = oracle.verbatim_count_bits(n, bps)
        if n >= 64 and fc.use_lpc:
            best, _ = search(x, bps, fc.qlpc, self.floor, self.extras, self.orders, self.K)
            baseline = bits if kind == 2 else verbatim
            if best["status"] == om.STATUS_OK and best["subframe_bits"] < baseline:
                qp = best["qp"]
                return 3, best["subframe_bits"], {
                    "kind": 3, "bps": bps, "samples": x, "order": int(qp.order), "shift": int(qp.shift),
                    "precision": int(qp.precision), "coefs": np.array(qp.coefs[:32], np.int16),
                    "rice_order": best["rice_order"], "rice_params": best["rice_params"], "residual": best["residual"]}
        if kind == 2:
            f = enc["fixed"]
            return 2, bits, {"kind": 2, "bps": bps, "samples": x, "order": int(f.order), "rice_order": int(f.rice_order),
                             "rice_params": enc["rice_params"][:1 << int(f.rice_order)].copy(),
                             "residual": enc["residual"]}
        return 1, bits, {"kind": 1, "bps": bps, "samples": x}

    wasted_channel_frame_bytes = gm.Model.wasted_channel_frame_bytes
