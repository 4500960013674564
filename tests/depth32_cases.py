"""32-bit FLAC frames and streams for the depth-32 decoder tests, CPU and GPU (flacenc_hip_set_max_bits_per_sample).

Ground truth is independent of the code under test: every frame is written by flac_write (the RFC-derived writer, in
Python integers) from the samples it must decode to, and the builder asserts two conditions on its own inputs:
  * every residual lies in (-2^31, 2^31) -- RFC 9639 section 9.2.7.3; flac_write does not check it;
  * flac_parse (the RFC-derived parser, Python integers) reads the frame back to the samples it was written from.
Signals are chosen so that the first holds: Verbatim and Constant subframes carry the extremes, and the predictors run
on a full-scale sinusoid plus a few bits of noise (full-scale white noise does not qualify: its order-2 fixed residual
reaches 2^33), or, where the shift is 0, on a near-full-scale level with a few bits of noise.  Residuals of this size are
coded with RICE2 parameters (up to 30): under the 4-bit method's limit of 14 a sample would take 2^17 unary bits."""
import numpy as np

import flac_parse
import flac_write as fw

HI, LO = (1 << 31) - 1, -(1 << 31)
LPC_ORDERS = (1, 4, 5, 8, 9, 16, 17, 32)  # the decoder's order buckets are <= 4, <= 8, <= 16, <= 32


def _side_index(ch_tag):
    return {8: 1, 9: 0, 10: 1}.get(ch_tag, -1)


def _coded(x, ch_tag):
    if ch_tag == 8:
        return [x[0], x[0] - x[1]]
    if ch_tag == 9:
        return [x[0] - x[1], x[1]]
    if ch_tag == 10:
        return [(x[0] + x[1]) >> 1, x[0] - x[1]]
    return [x[c] for c in range(x.shape[0])]


def _assert_residuals_fit(x, ch_tag, subframes):
    for c, (sig, sf) in enumerate(zip(_coded(x, ch_tag), subframes)):
        if sf["kind"] not in ("fixed", "lpc"):
            continue
        sig = np.asarray(sig, np.int64) >> sf.get("wasted", 0)
        order = sf.get("order", 0)
        coefs, shift = (fw.FIXED_COEFS[order], 0) if sf["kind"] == "fixed" else (sf["coefs"], sf["shift"])
        # (int64 is exact here: |c| < 2^15, |x| < 2^33, at most 32 terms)
        e = fw.residuals(sig, coefs, shift, order)[order:]
        assert e.size == 0 or (int(e.min()) > -(1 << 31) and int(e.max()) < (1 << 31)), (c, int(e.min()), int(e.max()))


def make_case(name, x, ch_tag, subframes, bps=32, ss_code=7, **hdr):
    """-> dict(name, data, channels, bps, x int64 [nch, n], number); asserts the two conditions of the module."""
    x = np.asarray(x, np.int64)
    lo, hi = -(1 << (bps - 1)), (1 << (bps - 1)) - 1
    assert x.ndim == 2 and int(x.min()) >= lo and int(x.max()) <= hi, name
    _assert_residuals_fit(x, ch_tag, subframes)
    data = fw.frame(x, ch_tag, bps, subframes, ss_code=ss_code, **hdr)
    back = flac_parse.parse_frame(data, stream_bps=bps, wasted_ok=True)
    assert back["bps"] == bps and back["length"] == len(data) and np.array_equal(back["channels"], x), name
    return dict(name=name, data=data, channels=x.shape[0], bps=bps, x=x, number=hdr.get("number", 0))


def sinusoid(rng, n, scale=1.0, period=None, noise_bits=3, bps=32):
    """A sinusoid of `scale` times full scale plus `noise_bits` bits of noise, clipped to the open range."""
    hi = (1 << (bps - 1)) - 1
    period = period or rng.uniform(60, 200)
    t = np.arange(n) + rng.uniform(0, period)
    s = np.round(scale * hi * np.sin(2 * np.pi * t / period)).astype(np.int64)
    s += rng.integers(-(1 << noise_bits), (1 << noise_bits) + 1, n)
    return np.clip(s, -hi, hi)


def level(rng, n, at, noise_bits=2):
    """A level `at` with a few bits of noise (inside the 32-bit range)."""
    return np.clip(at + rng.integers(-(1 << noise_bits), (1 << noise_bits) + 1, n), LO, HI).astype(np.int64)


def opposed_pair(rng, n):
    """Left a full-scale sinusoid, right its negative (plus noise): the side channel needs 33 bits, and an odd side
    sample occurs (asserted), so mid/side exercises the parity bit."""
    left = sinusoid(rng, n)
    right = np.clip(-left + rng.integers(-8, 9, n), -HI, HI)
    x = np.stack([left, right])
    side = x[0] - x[1]
    assert int(np.abs(side).max()) > 1 << 31 and (side & 1).any()  # more than 32 bits; an odd sample
    return x


def skewed_pair(rng, n):
    """Left a full-scale sinusoid, right minus half of it (plus noise): the side channel, 1.5 times left, needs 33 bits
    (asserted), and the mid, a quarter of left, is large too -- every coded channel of every stereo code is."""
    left = sinusoid(rng, n)
    right = np.clip(-(left >> 1) + rng.integers(-8, 9, n), -HI, HI)
    x = np.stack([left, right])
    side = x[0] - x[1]
    assert int(np.abs(side).max()) > 1 << 31 and (side & 1).any()
    return x


def presums(sig, coefs, order):
    """The pre-shift prediction sums of a coded channel, sum_j c_j x[t-1-j] for t >= order (int64 is exact: |c| < 2^15,
    |x| < 2^33, at most 32 terms)."""
    sig = np.asarray(sig, np.int64)
    acc = np.zeros(len(sig) - order, np.int64)
    for j, c in enumerate(coefs):
        acc += int(c) * sig[order - 1 - j:len(sig) - 1 - j]
    return acc


def lpc_shift14(order):
    """Precision 15, shift 14: c0 = 16383 predicts the previous sample, the rest are small.  The pre-shift sum is about
    2^14 times the sample: above 2^40 on every coded channel (asserted by the builder below on the true sums)."""
    return [16383] + [(-1) ** j * (1 + j % 3) for j in range(1, order)]


def lpc_shift0(order):
    """Precision 15, shift 0 on a level: 16000 x[t-1] - 15999 x[t-2] = x[t-1] + 15999 (x[t-1] - x[t-2]).  With shift 0 the
    sum itself is the prediction and must stay near the sample, so it cannot exceed 2^40 in a valid stream; its two
    products do (about 2^45 on a near-full-scale level).  Both are asserted by the builder below."""
    return [1] if order == 1 else [16000, -15999] + [0] * (order - 2)


def frame_cases():
    rng = np.random.default_rng(0xD32)
    out = []
    V, K = dict(kind="verbatim"), dict(kind="constant")

    # ---- independent channels: codes 0, 1, 7; both sample-size codes; block sizes 16 and 17 ----
    alt = np.where(np.arange(16) % 2 == 0, HI, LO)
    out.append(make_case("mono verbatim extremes n=16", alt[None], 0, [V]))
    out.append(make_case("mono verbatim extremes n=17 code 0", np.append(-alt - 1, HI)[None], 0, [V], ss_code=0))
    out.append(make_case("2 ch constant extremes n=17", np.stack([np.full(17, HI), np.full(17, LO)]), 1, [K, K]))
    x8 = np.stack([sinusoid(rng, 64) for _ in range(8)])
    sf8 = [dict(kind="fixed", order=o, method=1) for o in range(5)] + [V, dict(kind="fixed", order=2, method=1), V]
    out.append(make_case("8 ch fixed 0..4", x8, 7, sf8))
    out.append(make_case("8 ch fixed 0..4 code 0", x8[::-1], 7, sf8, ss_code=0))

    # ---- the 33-bit extremes on every stereo code: side = +-(2^32 - 1), verbatim and constant ----
    for tag in (8, 9, 10):
        xa = np.stack([alt, -alt - 1])  # left 2^31 - 1 against right -2^31, and the reverse, alternating
        out.append(make_case(f"code {tag} verbatim extremes n=16", xa, tag, [V, V]))
        out.append(make_case(f"code {tag} verbatim extremes n=17 code 0", np.stack([np.append(-alt - 1, HI),
                                                                                  np.append(alt, LO)]), tag, [V, V], ss_code=0))
        out.append(make_case(f"code {tag} constant side +", np.stack([np.full(16, HI), np.full(16, LO)]), tag, [K, K]))
        out.append(make_case(f"code {tag} constant side -", np.stack([np.full(17, LO), np.full(17, HI)]), tag, [K, K]))
    odd = np.stack([level(rng, 32, HI - 40), level(rng, 32, LO + 41)])
    odd[0, 0], odd[1, 0] = HI, LO + 2  # side 2^32 - 3: odd, and mid << 1 | 1 plus side needs 34 bits
    out.append(make_case("code 10 odd side, 34-bit sum", odd, 10, [V, V]))

    # ---- fixed predictors on a 33-bit side ----
    for o in range(1, 5):
        tag = (8, 9, 10)[o % 3]
        sfs = [dict(kind="fixed", order=o, method=1), dict(kind="fixed", order=o, method=1)]
        out.append(make_case(f"code {tag} fixed {o}", opposed_pair(rng, 64), tag, sfs))
    near = np.stack([sinusoid(rng, 48), np.zeros(48, np.int64)])
    near[1] = np.clip(near[0] + rng.integers(-100, 101, 48), -HI, HI)
    out.append(make_case("code 10 fixed 0 on a small side", near, 10, [dict(kind="fixed", order=1, method=1), dict(kind="fixed", order=0)]))

    # ---- LPC at the order-bucket edges, precision 15, shifts 14 and 0 ----
    for i, order in enumerate(LPC_ORDERS):
        n = 64 if order <= 16 else 96
        tag = (8, 9, 10, 0)[i % 4]
        c14 = lpc_shift14(order)
        sf = dict(kind="lpc", order=order, coefs=c14, precision=15, shift=14, method=1)
        x = sinusoid(rng, n, period=rng.uniform(150, 300))[None] if tag == 0 else skewed_pair(rng, n)
        for sig in _coded(x, tag):  # the true pre-shift sum of every coded channel, the mid included
            assert int(np.abs(presums(sig, c14, order)).max()) > 1 << 40
        out.append(make_case(f"code {tag} lpc {order} shift 14", x, tag, [sf] * x.shape[0]))
        c0 = lpc_shift0(order)
        sf = dict(kind="lpc", order=order, coefs=c0, precision=15, shift=0, method=1)
        tag = (10, 8, 9, 0)[i % 4]
        x = level(rng, n, HI - 1000)[None] if tag == 0 else np.stack([level(rng, n, HI - 1000), level(rng, n, LO + 1000)])
        for c, sig in enumerate(_coded(x, tag)):
            # with shift 0 the sum IS the prediction: it stays near the sample (33 bits), its products do not -- except
            # on the mid of opposed levels, which is a few bits of noise
            assert int(np.abs(presums(sig, c0, order)).max()) < 1 << 33
            if order > 1 and not (tag == 10 and c == 0):
                assert c0[0] * int(np.abs(sig).max()) > 1 << 40
        out.append(make_case(f"code {tag} lpc {order} shift 0", x, tag, [sf] * x.shape[0]))

    # ---- wasted bits: 1, 8 and 31 on a 32-bit channel, 32 on a 33-bit side ----
    for wasted in (1, 8):
        x = (sinusoid(rng, 32, bps=32 - wasted) << wasted)[None]
        out.append(make_case(f"mono wasted {wasted}", x, 0, [dict(kind="fixed", order=1, method=1, wasted=wasted)]))
    x31 = (rng.integers(-1, 1, 24) << 31)[None]
    assert x31.min() == LO and x31.max() == 0
    out.append(make_case("mono wasted 31", x31, 0, [dict(kind="verbatim", wasted=31)]))
    # (a 33-bit side with 32 wasted bits has one bit left: 0 or -2^32, and only 0 is a difference of two 32-bit samples)
    same = sinusoid(rng, 24)
    out.append(make_case("code 8 side wasted 32", np.stack([same, same]), 8,
                         [dict(kind="fixed", order=2, method=1), dict(kind="verbatim", wasted=32)]))
    out.append(make_case("code 10 side wasted 32", np.stack([same, same]), 10,
                         [dict(kind="fixed", order=2, method=1), dict(kind="constant", wasted=32)]))

    # ---- residual forms: RICE2 parameter 30, an escaped partition of width 31 ----
    wide = rng.integers(-HI, HI + 1, 32)[None]
    out.append(make_case("mono rice2 parameter 30", wide, 0, [dict(kind="fixed", order=0, method=1, params=[30])]))
    half = rng.integers(-(1 << 30), 1 << 30, 32)[None]
    out.append(make_case("mono escape width 31", half, 0,
                         [dict(kind="fixed", order=0, method=1, porder=1, params=[("esc", 31), 30])]))

    # ---- a variable-blocking header with a 36-bit sample number ----
    out.append(make_case("code 10 variable, 36-bit number", opposed_pair(rng, 40), 10,
                         [dict(kind="fixed", order=2, method=1), dict(kind="fixed", order=3, method=1)], number=0xFFFFFFFFF, variable=True))
    return out


def broken_copies(cases, seed=0xB0B):
    """Per case a bit-flipped and a truncated copy: (name, bytes, channels, bps)."""
    rng = np.random.default_rng(seed)
    out = []
    for c in cases:
        b = bytearray(c["data"])
        i = int(rng.integers(len(b) * 8))
        b[i // 8] ^= 0x80 >> (i % 8)
        out.append((c["name"] + " / bit flip", bytes(b), c["channels"], c["bps"]))
        out.append((c["name"] + " / truncated", c["data"][: int(rng.integers(1, len(c["data"])))], c["channels"], c["bps"]))
    return out


def by_shape(cases):
    """The cases grouped by (channels, bps): one decode call each."""
    groups = {}
    for c in cases:
        groups.setdefault((c["channels"], c["bps"]), []).append(c)
    return groups


def mixed_streams():
    """16-bit, 24-bit and 32-bit streams side by side, a few frames each: dict(bps, channels, n, frames [bytes],
    x [int64 [nch, n]])."""
    rng = np.random.default_rng(0x3117)
    out = []

    def stream(bps, tag, n, n_frames, make_x, sfs, ss_code=None):
        frames, xs = [], []
        for f in range(n_frames):
            ss = ss_code if ss_code is not None else (7 if bps == 32 else fw.SS_CODES[bps])
            c = make_case(f"stream {bps}/{tag} frame {f}", make_x(), tag, sfs, bps=bps, number=f, ss_code=ss)
            frames.append(c["data"])
            xs.append(c["x"])
        out.append(dict(bps=bps, channels=xs[0].shape[0], n=n, frames=frames, x=xs))

    f2, f1 = dict(kind="fixed", order=2, method=1), dict(kind="fixed", order=1, method=1)
    stream(16, 0, 192, 3, lambda: sinusoid(rng, 192, bps=16)[None], [f2])
    stream(32, 10, 192, 4, lambda: opposed_pair(rng, 192), [f2, f1])
    stream(24, 8, 192, 3, lambda: np.stack([sinusoid(rng, 192, bps=24), sinusoid(rng, 192, 0.5, bps=24)]), [f2, f2])
    stream(32, 0, 64, 3, lambda: sinusoid(rng, 64)[None], [dict(kind="lpc", order=9, coefs=lpc_shift14(9), precision=15,
                                                              shift=14, method=1)], ss_code=0)
    stream(16, 9, 192, 3, lambda: np.stack([sinusoid(rng, 192, bps=16), sinusoid(rng, 192, bps=16)]), [f1, f2])
    stream(32, 8, 192, 3, lambda: opposed_pair(rng, 192), [f2, dict(kind="fixed", order=3, method=1)])
    return out


def streaminfo(bps, channels, max_block, total_samples, md5, rate=44100):
    """"fLaC" and one STREAMINFO block (the last metadata block)."""
    w = fw.BitWriter()
    w.u(1, 1)
    w.u(0, 7)
    w.u(34, 24)
    w.u(max_block, 16)
    w.u(max_block, 16)
    w.u(0, 24)
    w.u(0, 24)
    w.u(rate, 20)
    w.u(channels - 1, 3)
    w.u(bps - 1, 5)
    w.u(total_samples, 36)
    return b"fLaC" + w.bytes() + bytes(md5)


# ---- invalid streams that pass both CRCs: the wide decoder's value rule ----
def _wrap64(v):
    v &= (1 << 64) - 1
    return v - (1 << 64) if v >> 63 else v


def _low32(v):
    return ((v & 0xFFFFFFFF) ^ 0x80000000) - 0x80000000


def wide_rule_lpc(warm, coefs, shift, e, n):
    """The rule of flac_decode_core.h in Python integers: sums, products and the final add wrap at 64 bits, the shift is
    arithmetic.  -> (the n values, whether a sum left 64 bits before it was wrapped)."""
    x, wrapped = [int(v) for v in warm], False
    for t in range(len(warm), n):
        full = sum(int(c) * x[t - 1 - j] for j, c in enumerate(coefs))
        pred = _wrap64(full)
        wrapped |= pred != full
        x.append(_wrap64(int(e[t]) + (pred >> shift)))
    return x, wrapped


def wide_rule_stereo(ch_tag, a, b):
    if ch_tag == 8:
        return a, _wrap64(a - b)
    if ch_tag == 9:
        return _wrap64(a + b), b
    m = _wrap64((a << 1) | (b & 1))
    return _wrap64(m + b) >> 1, _wrap64(m - b) >> 1


def _raw_lpc_subframe(w, sbps, warm, coefs, shift, e, n):
    """An LPC subframe (precision 15, one RICE2 partition of parameter 30) from its fields, not from samples."""
    order = len(coefs)
    w.u(0, 1)
    w.u(31 + order, 6)
    w.u(0, 1)
    for v in warm:
        w.s(v, sbps)
    w.u(14, 4)
    w.s(shift, 5)
    for c in coefs:
        w.s(c, 15)
    fw.write_residual(w, e, order, n, 1, 0, [30])


def invalid_cases():
    """32-bit frames no encoder writes -- reconstructed values leave 32 bits, and in the LPC cases 64 -- with valid
    CRCs: dict(name, data, channels, bps, want int64 [nch, n] = the low 32 bits the value rule gives)."""
    rng = np.random.default_rng(0x1BAD)
    out = []

    def finish(name, ch_tag, n, write_subframes, coded):
        w = fw.BitWriter()
        w.bits = list(np.unpackbits(np.frombuffer(fw.header(n, ch_tag, 32, 0, ss_code=7), np.uint8)))
        write_subframes(w)
        w.align()
        b = w.bytes()
        data = b + flac_parse.crc16(b).to_bytes(2, "big")
        if ch_tag >= 8:
            pairs = [wide_rule_stereo(ch_tag, a, b_) for a, b_ in zip(*coded)]
            coded = [[p[0] for p in pairs], [p[1] for p in pairs]]
        assert any(v != _low32(v) for row in coded for v in row), name  # something leaves 32 bits
        want = np.array([[_low32(v) for v in row] for row in coded], np.int64)
        out.append(dict(name=name, data=data, channels=len(coded), bps=32, want=want))

    n = 24
    for shift, coefs in ((0, [16383, 16383]), (3, [16383, -16384, 16383])):
        e = rng.integers(-HI, HI + 1, n)
        x, wrapped = wide_rule_lpc([HI, LO, HI][: len(coefs)], coefs, shift, e, n)
        assert wrapped
        finish(f"mono lpc shift {shift} wraps at 64 bits", 0, n,
               lambda w: _raw_lpc_subframe(w, 32, [HI, LO, HI][: len(coefs)], coefs, shift, e, n), [x])
    for tag in (8, 9, 10):
        e0, e1 = rng.integers(-HI, HI + 1, n), rng.integers(-HI, HI + 1, n)
        sb = [32 + (c == _side_index(tag)) for c in range(2)]
        warm = [[(1 << (sb[c] - 1)) - 1, -(1 << (sb[c] - 1))] for c in range(2)]
        coefs = [16383, 16000]
        x0, w0 = wide_rule_lpc(warm[0], coefs, 1, e0, n)
        x1, w1 = wide_rule_lpc(warm[1], coefs, 1, e1, n)
        assert w0 and w1

        def both(w, sb=sb, warm=warm, e0=e0, e1=e1):
            _raw_lpc_subframe(w, sb[0], warm[0], coefs, 1, e0, n)
            _raw_lpc_subframe(w, sb[1], warm[1], coefs, 1, e1, n)
        finish(f"code {tag} lpc wraps at 64 bits", tag, n, both, [x0, x1])
    # verbatim: nothing wraps at 64 bits, the other channel of a left/side or right/side pair leaves 32
    side = np.where(np.arange(16) % 2 == 0, -((1 << 32) - 1), (1 << 32) - 1)
    main = np.where(np.arange(16) % 2 == 0, HI, LO)
    for tag in (8, 9, 10):
        coded = [main, side] if tag != 9 else [-side, main]  # (right/side adds, the others subtract)

        def verb(w, coded=coded, tag=tag):
            for c in range(2):
                fw.write_subframe(w, coded[c], 32 + (c == _side_index(tag)), "verbatim")
        finish(f"code {tag} verbatim leaves 32 bits", tag, 16, verb, [[int(v) for v in coded[0]], [int(v) for v in coded[1]]])
    return out
