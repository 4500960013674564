"""A model of FLACENC_HIP_FLAG_WINDOW_SEARCH built from oracle calls: per LPC candidate subframe with lpc_order = P, window 0
is the config's and windows 1 .. W-1 the extra entries (type, alpha, start, end); R_j[0..P] is the stable build's
autocorrelation of fill_windowed_signal(x, w_j) (the simd-nightly build's under ACORR_NIGHTLY).  The candidates are (j, P)
for every window, or (j, o) for every window and o = 1..P with the order search, each built by order_model.candidate; the
one with status 0 and the smallest Lpc::count_bits wins (ties: the lower window, then the lower order), else (0, P).
Frames apply encode_subframe's rules with that LPC candidate and try_stereo_coding, and are written by the oracle's
writer (by flac_write under wasted bits), as order_model does."""
import numpy as np

import order_model as om
from oracle import oracle

RECTANGLE, TUKEY, PARTIAL_TUKEY, PUNCHOUT_TUKEY = 0, 1, 2, 3
UNIT = 65536
# the extra windows of a fresh handle (the contract's table)
DEFAULT = ((PARTIAL_TUKEY, 0.2, 0, 36044), (PARTIAL_TUKEY, 0.2, 29492, 65536), (PUNCHOUT_TUKEY, 0.2, 0, 21845),
           (PUNCHOUT_TUKEY, 0.2, 21845, 43690), (PUNCHOUT_TUKEY, 0.2, 43690, 65536))
STEREO_ROLES = om.STEREO_ROLES


def tukey(alpha, m) -> np.ndarray:
    """T(m): the reference's Tukey weights of length m; all zeros below 2 samples."""
    if m < 2:
        return np.zeros(m, np.float32)
    return oracle.window_weights(("tukey", float(np.float32(alpha))), m)


def piece(start, end, n):
    """(s, e) of an entry over n samples, integers only."""
    return (int(start) * n) >> 16, (int(end) * n) >> 16


def weights(entry, n) -> np.ndarray:
    """The weights of an extra-window entry (type, alpha, start, end) over n samples."""
    t, alpha, start, end = entry
    if t == RECTANGLE:
        return np.ones(n, np.float32)
    if t == TUKEY:
        return tukey(alpha, n)
    s, e = piece(start, end, n)
    w = np.zeros(n, np.float32)
    if t == PARTIAL_TUKEY:
        w[s:e] = tukey(alpha, e - s)
    elif t == PUNCHOUT_TUKEY:
        w[:s] = tukey(alpha, s)
        w[e:] = tukey(alpha, n - e)
    else:
        raise ValueError(t)
    return w


ALPHAS = (0.0, 0.1, 0.2, 0.5, 1.0)


def unit_of(sample, n) -> int:
    """The smallest start / end value whose piece boundary over n samples is `sample` (0 <= sample <= n)."""
    return -((-sample << 16) // n)


def random_extras(rng, n) -> tuple:
    """A valid extra-window list for blocks of n samples: 0 to 7 entries of all four types, alphas from ALPHAS, and
    among the pieces some that are empty or one sample long on n (a partial window's piece, a punch-out's head or
    tail).  Every entry passes flacenc_hip_set_lpc_windows' validation: 0 <= start < end <= 65536 for the two piece
    types."""
    out = []
    for _ in range(int(rng.integers(0, 8))):
        t = int(rng.integers(0, 4))
        alpha = float(rng.choice(ALPHAS))
        start = end = 0
        if t >= PARTIAL_TUKEY:
            m = int(rng.integers(0, 2))  # the degenerate length
            shape = int(rng.integers(0, 3))
            if shape > 0:
                start = int(rng.integers(0, UNIT))
                end = int(rng.integers(start + 1, UNIT + 1))
            elif t == PARTIAL_TUKEY:
                s = int(rng.integers(0, n - m + 1 if m else n))
                start = unit_of(s, n)
                end = unit_of(s + m, n) if m else start + 1
                assert piece(start, end, n) == (s, s + m)
            elif rng.random() < 0.5:  # a head of m samples
                start = unit_of(m, n) if m else 0
                end = int(rng.integers(start + 1, UNIT + 1))
                assert piece(start, end, n)[0] == m
            else:  # a tail of m samples
                end = unit_of(n - m, n)
                start = int(rng.integers(0, end))
                assert n - piece(start, end, n)[1] == m
            assert 0 <= start < end <= UNIT
        out.append((t, alpha, start, end))
    return tuple(out)


def config_window(cfg, n) -> np.ndarray:
    """Window 0: the config's own (window_type, tukey_alpha)."""
    if cfg.window_type == RECTANGLE:
        return np.ones(n, np.float32)
    return oracle.window_weights(("tukey", cfg.tukey_alpha), n)


def autocorr(x, w, cfg) -> np.ndarray:
    """R[0..P] of x under window w in the configured summation order."""
    xw = oracle.fill_windowed_signal(x, w)
    P = cfg.lpc_order
    if cfg.acorr_order == oracle.ACORR_NIGHTLY:
        return oracle.auto_correlation_nightly(P + 1, xw)
    return oracle.auto_correlation(P + 1, xw)


def search(x, bps, cfg, extras=DEFAULT, orders=False):
    """-> (the flagged LPC candidate with "j" and "R", every candidate).  orders: FLACENC_HIP_FLAG_ORDER_SEARCH as well."""
    x = np.ascontiguousarray(x, np.int32)
    n, P = len(x), cfg.lpc_order
    wins = [config_window(cfg, n)] + [weights(e, n) for e in extras]
    cands = []
    for j, w in enumerate(wins):
        R = autocorr(x, w, cfg)
        for o in (range(1, P + 1) if orders else (P,)):
            c = om.candidate(x, bps, R, o, cfg)
            c.update(j=j, R=R)
            cands.append(c)
    ok = [c for c in cands if c["status"] == om.STATUS_OK]
    fallback = next(c for c in cands if c["j"] == 0 and c["o"] == P)
    best = min(ok, key=lambda c: (c["subframe_bits"], c["j"], c["o"])) if ok else fallback
    return best, cands


def record(x, bps, cfg, extras=DEFAULT, orders=False):
    """The candidate batch's outputs for one subframe: (record fields, residual row, autocorr [33], lpc_coefs [32])."""
    best, _ = search(x, bps, cfg, extras, orders)
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


class Model:
    """encode_subframe / encode_frame with the flagged LPC candidate of one extra-window list."""

    def __init__(self, extras=DEFAULT, orders=False):
        self.extras, self.orders = tuple(extras), orders

    def encode_subframe(self, x, bps, fc):
        """encode_subframe (coding.rs:384-418) -> (kind, bits, oracle writer keywords), as order_model.encode_subframe."""
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
            best, _ = search(x, bps, fc.qlpc, self.extras, self.orders)
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

    @staticmethod
    def _assign(b, fc):
        best, a = b[0] + b[1], 0
        if fc.use_leftside and b[0] + b[3] < best:
            best, a = b[0] + b[3], 1
        if fc.use_rightside and b[1] + b[3] < best:
            best, a = b[1] + b[3], 2
        if fc.use_midside and b[2] + b[3] < best:
            best, a = b[2] + b[3], 3
        return a

    def stereo_frame_bytes(self, l, r, bps, fc, number=0, sample_rate=44100) -> bytes:
        l = np.ascontiguousarray(l, np.int32)
        r = np.ascontiguousarray(r, np.int32)
        m, s = oracle.stereo_to_midside(l, r)
        subs = [self.encode_subframe(x, bps + (1 if k == 3 else 0), fc) for k, x in enumerate((l, r, m, s))]
        a = self._assign([x[1] for x in subs], fc)
        return oracle.write_frame(len(l), a, bps, sample_rate, number, [subs[k][2] for k in STEREO_ROLES[a]])

    def channel_frame_bytes(self, xs, bps, fc, number=0, sample_rate=44100) -> bytes:
        """An Independent(len(xs)) frame."""
        subs = [self.encode_subframe(x, bps, fc)[2] for x in xs]
        return oracle.write_frame(len(xs[0]), 0, bps, sample_rate, number, subs)

    def wasted_stereo_frame_bytes(self, l, r, bps, fc, number=0) -> bytes:
        """A 2-channel frame under FLACENC_HIP_FLAG_WASTED_BITS as well (order_model.wasted_stereo_frame_bytes)."""
        import flac_write
        import wasted_model
        subs = []
        for k, x in enumerate(wasted_model.roles(l, r)):
            x = np.ascontiguousarray(x, np.int32)
            w = bps + (1 if k == 3 else 0)
            kw_ = wasted_model.wasted_of(x, fc)
            kind, bits, kw = self.encode_subframe(x >> kw_, w - kw_, fc)
            subs.append({"kind": kind, "bits": bits + kw_, "k": kw_, "kw": kw})
        a = self._assign([s_["bits"] for s_ in subs], fc)
        return flac_write.frame([l, r], wasted_model.STEREO_TAGS[a], bps,
                                [om._flac_write_args(subs[k]) for k in STEREO_ROLES[a]], number=number)
