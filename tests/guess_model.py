"""A model of FLACENC_HIP_FLAG_ORDER_GUESS built from oracle calls and numpy (include/flacenc_hip.h states the rule): per
LPC candidate subframe with lpc_order = P and per window j, the Levinson error chain e_o = e_(o-1) (1 - k_o^2) over the
order-o candidates of order_model.candidate on R_j[0..o], the estimated bits b_o = max(0, 0.5 log2f(e_o / 2n)), the cost
b_o (n - o) + o (q + w), and the K eligible orders of the smallest (cost, order) as the window's guesses.  The coded
candidates are (0, P) and every guess, each order_model.candidate; the one with status 0 and the smallest Lpc::count_bits
wins (ties: the lower window, then the lower order), else (0, P).  Windows, frames and wasted bits are window_model's."""
import numpy as np

import order_model as om
import window_model as wm
from oracle import oracle


def levinson(R, o):
    """(status, k_o) of order_model.candidate(.., R, o, ..) -- its status checks and its unquantised coefficient number
    o - 1 -- without its residual and Rice search (tests/test_order_guess_cpu.py holds the two together)."""
    Ro = np.ascontiguousarray(R[: o + 1], np.float64)
    st = om._levinson_status(Ro)
    if st != om.STATUS_OK or Ro[0] == 0.0:
        return st, 0.0
    coefs, _ = oracle.symmetric_levinson_recursion(Ro[:o], Ro[1:o + 1])
    if not np.all(np.isfinite(coefs)):
        return om.STATUS_NONFINITE, 0.0
    return om.STATUS_OK, float(coefs[o - 1])


def bits_per_sample(e, n) -> np.float32:
    """b_o of prediction error e over n samples."""
    with np.errstate(over="ignore", under="ignore"):
        x = np.float32(float(e) * (0.5 / float(n)))
    if not x > 0:
        return np.float32(0.0)
    b = np.float32(0.5) * np.float32(oracle.log2f(x))
    return b if b > 0 else np.float32(0.0)


def cost(b, n, o, q, w) -> float:
    return float(b) * float(n - o) + float(o * (q + w))


def chain(R0, ks, statuses, n, w, q):
    """The eligible orders' (e_o, x-free b_o, cost_o) from k_1.. and the candidates' statuses: -> (eligible count, e[],
    b[], cost[]), entry o - 1 for order o."""
    es, bs, costs = [], [], []
    e = float(R0)
    if not e >= 0.0:
        return 0, es, bs, costs
    for o, (k, st) in enumerate(zip(ks, statuses), 1):
        if st != om.STATUS_OK:
            break
        e = e * (1.0 - float(k) * float(k))
        if not e >= 0.0:
            break
        b = bits_per_sample(e, n)
        es.append(e)
        bs.append(b)
        costs.append(cost(b, n, o, q, w))
    return len(es), es, bs, costs


def pick(costs, K):
    """The K orders of the smallest (cost, order) among orders 1..len(costs), ascending."""
    ranked = sorted(range(1, len(costs) + 1), key=lambda o: (costs[o - 1], o))
    return sorted(ranked[:K])


def guesses_from_R(R, P, n, w, q, K):
    """One window's guesses from R[0..P] -> {"eligible", "e", "b", "cost", "guesses"}."""
    lev = [levinson(R, o) for o in range(1, P + 1)]
    m, es, bs, costs = chain(R[0], [k for _, k in lev], [st for st, _ in lev], n, w, q)
    return {"eligible": m, "e": es, "b": bs, "cost": costs, "guesses": pick(costs, K)}


def windows(cfg, n, extras):
    return [wm.config_window(cfg, n)] + [wm.weights(e, n) for e in extras]


def search(x, bps, cfg, K=1, extras=()):
    """-> (the flagged LPC candidate with "j" and "R", the coded candidates in kernel order, the per-window guess
    records).  extras = () is the call without FLACENC_HIP_FLAG_WINDOW_SEARCH."""
    x = np.ascontiguousarray(x, np.int32)
    n, P, q = len(x), cfg.lpc_order, cfg.quant_precision
    cands, per_window = [], []
    for j, wts in enumerate(windows(cfg, n, extras)):
        R = wm.autocorr(x, wts, cfg)
        g = guesses_from_R(R, P, n, bps, q, K)
        per_window.append(g)
        orders = set(g["guesses"]) | ({P} if j == 0 else set())
        for o in sorted(orders):
            c = om.candidate(x, bps, R, o, cfg)
            c.update(j=j, R=R)
            cands.append(c)
    ok = [c for c in cands if c["status"] == om.STATUS_OK]
    fallback = next(c for c in cands if c["j"] == 0 and c["o"] == P)
    best = min(ok, key=lambda c: (c["subframe_bits"], c["j"], c["o"])) if ok else fallback
    return best, cands, per_window


def record(x, bps, cfg, K=1, extras=()):
    """The candidate batch's outputs for one subframe: (record fields, residual row, autocorr [33], lpc_coefs [32])."""
    best, _, _ = search(x, bps, cfg, K, extras)
    ac = np.zeros(33)
    ac[: cfg.lpc_order + 1] = best["R"]
    lc = np.zeros(32)
    if best["status"] != om.STATUS_OK:
        return {"status": int(best["status"])}, np.zeros(len(x), np.int32), ac, lc
    lc[: best["o"]] = best["coefs"]
    qp = best["qp"]
    rec = {"order": int(qp.order), "shift": int(qp.shift), "precision": int(qp.precision),
           "coefs": [int(c) for c in qp.coefs[:32]], "rice_order": best["rice_order"],
           "rice_params": [int(p) for p in best["rice_params"]], "status": 0, "code_bits": best["code_bits"],
           "subframe_bits": best["subframe_bits"], "sum_quotients": best["sum_quotients"]}
    return rec, best["residual"], ac, lc


class Model(wm.Model):
    """encode_subframe / encode_frame with the guessed LPC candidate: window_model.Model's frames, assignment and wasted
    bits around this module's search."""

    def __init__(self, K=1, extras=()):
        super().__init__(extras, False)
        self.K = K

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
            best, _, _ = search(x, bps, fc.qlpc, self.K, self.extras)
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

    def wasted_channel_frame_bytes(self, xs, bps, fc, number=0) -> bytes:
        """An Independent(len(xs)) frame under FLACENC_HIP_FLAG_WASTED_BITS as well (order_model.wasted_channel_frame_bytes)."""
        import flac_write
        import wasted_model
        subs = []
        for x in xs:
            x = np.ascontiguousarray(x, np.int32)
            k = wasted_model.wasted_of(x, fc)
            kind, bits, kw = self.encode_subframe(x >> k, bps - k, fc)
            subs.append({"kind": kind, "bits": bits + k, "k": k, "kw": kw})
        return flac_write.frame(xs, len(xs) - 1, bps, [om._flac_write_args(s) for s in subs], number=number)
