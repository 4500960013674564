"""A small FLAC frame writer for the decoder tests, written from RFC 9639.  It writes what the oracle's writer
(Frame::write) never does: wasted bits, escaped partitions, RICE2 parameters above 14, variable-blocking headers with
multi-byte sample numbers and every block-size / sample-rate code.  Frames are built from a description and the
samples they must decode to; predictions use the decoder's arithmetic (64-bit sum, arithmetic shift, i32 wrap)."""
import numpy as np

from flac_parse import crc8, crc16

FIXED_COEFS = [[], [1], [2, -1], [3, -3, 1], [4, -6, 4, -1]]
BS_CODES = {192: 1, 576: 2, 1152: 3, 2304: 4, 4608: 5, 256: 8, 512: 9, 1024: 10, 2048: 11, 4096: 12, 8192: 13,
            16384: 14, 32768: 15}
SS_CODES = {8: 1, 12: 2, 16: 4, 20: 5, 24: 6}


class BitWriter:
    def __init__(self):
        self.bits = []

    def u(self, v, n):
        for i in range(n - 1, -1, -1):
            self.bits.append((int(v) >> i) & 1)

    def s(self, v, n):
        self.u(int(v) & ((1 << n) - 1), n)

    def unary(self, q):
        self.bits.extend([0] * q)
        self.bits.append(1)

    def align(self):
        while len(self.bits) % 8:
            self.bits.append(0)

    def bytes(self):
        assert len(self.bits) % 8 == 0
        return np.packbits(np.array(self.bits, np.uint8)).tobytes()


def utf8_number(v):
    if v < 0x80:
        return bytes([v])
    n = 2
    while v >= 1 << (5 * n + 1):
        n += 1
    assert n <= 7
    out = []
    for _ in range(n - 1):
        out.append(0x80 | (v & 0x3F))
        v >>= 6
    first = ((0xFF00 >> n) & 0xFF) | v
    return bytes([first] + out[::-1])


def header(block_size, ch_tag, bps, number, variable=False, bs_code=None, sr_code=9, ss_code=None, sr_value=0):
    if bs_code is None:
        bs_code = BS_CODES.get(block_size, 6 if block_size <= 256 else 7)
    if ss_code is None:
        ss_code = SS_CODES.get(bps, 0)
    w = BitWriter()
    w.u(0x3FFE, 14)
    w.u(0, 1)
    w.u(1 if variable else 0, 1)
    w.u(bs_code, 4)
    w.u(sr_code, 4)
    w.u(ch_tag, 4)
    w.u(ss_code, 3)
    w.u(0, 1)
    b = w.bytes() + utf8_number(number)
    if bs_code == 6:
        b += bytes([block_size - 1])
    elif bs_code == 7:
        b += (block_size - 1).to_bytes(2, "big")
    if sr_code == 12:
        b += bytes([sr_value])
    elif sr_code in (13, 14):
        b += int(sr_value).to_bytes(2, "big")
    return b + bytes([crc8(b)])


def residuals(x, coefs, shift, order):
    """e[t] = x[t] - (sum c_j x[t-1-j] >> shift) in the decoder's arithmetic (inverse of the reconstruction)."""
    x = np.asarray(x, np.int64)
    n = len(x)
    e = np.zeros(n, np.int64)
    if order >= n:
        return e
    # one int64 pass per coefficient: |c| < 2^15, |x| < 2^25 and at most 32 terms stay far below 2^63
    assert len(coefs) <= order
    pred = np.zeros(n - order, np.int64)
    for j, c in enumerate(coefs):
        pred += int(c) * x[order - 1 - j:n - 1 - j]
    e[order:] = x[order:] - (pred >> max(shift, 0))
    return e


def write_residual(w, e, order, n, method=0, porder=0, params=None):
    """params: per partition an int Rice parameter, or ("esc", width)."""
    w.u(method, 2)
    w.u(porder, 4)
    nparts = 1 << porder
    psize = n >> porder
    t = order
    for q in range(nparts):
        count = psize - (order if q == 0 else 0)
        p = params[q] if params is not None else best_param(e[t:t + count], method)
        if isinstance(p, tuple):
            w.u(15 if method == 0 else 31, 4 if method == 0 else 5)
            width = p[1]
            w.u(width, 5)
            for v in e[t:t + count]:
                assert width > 0 or v == 0
                if width:
                    assert -(1 << (width - 1)) <= v < (1 << (width - 1))
                    w.s(v, width)
        else:
            w.u(p, 4 if method == 0 else 5)
            for v in e[t:t + count]:
                u = (-2 * int(v) - 1) if v < 0 else 2 * int(v)
                w.unary(u >> p)
                w.u(u & ((1 << p) - 1), p)
        t += count


def best_param(e, method):
    limit = 14 if method == 0 else 30
    if len(e) == 0:
        return 0
    m = float(np.mean(np.abs(np.asarray(e, np.float64)))) + 1.0
    return int(min(limit, max(0, int(np.log2(m)))))


def write_subframe(w, x, sbps, kind, order=0, coefs=None, precision=0, shift=0, wasted=0, method=0, porder=0,
                   params=None):
    """x: the samples this subframe decodes to (already the side channel where it is one)."""
    x = np.asarray(x, np.int64)
    n = len(x)
    if wasted:
        assert np.all(x % (1 << wasted) == 0)
        x = x >> wasted
    ebps = sbps - wasted
    w.u(0, 1)
    typ = {"constant": 0, "verbatim": 1}.get(kind)
    if kind == "fixed":
        typ = 8 + order
    elif kind == "lpc":
        typ = 31 + order
    w.u(typ, 6)
    if wasted:
        w.u(1, 1)
        w.unary(wasted - 1)
    else:
        w.u(0, 1)
    if kind == "constant":
        assert np.all(x == x[0])
        w.s(x[0], ebps)
        return
    if kind == "verbatim":
        for v in x:
            w.s(v, ebps)
        return
    for v in x[:order]:
        w.s(v, ebps)
    if kind == "fixed":
        coefs, shift = FIXED_COEFS[order], 0
    else:
        w.u(precision - 1, 4)
        w.s(shift, 5)
        for c in coefs:
            w.s(c, precision)
    write_residual(w, residuals(x, coefs, shift, order), order, n, method, porder, params)


def frame(channels_x, ch_tag, bps, subframes, number=0, variable=False, **hdr):
    """channels_x: the decoded channels [nch, n]; subframes: per channel a dict of write_subframe keywords."""
    x = np.asarray(channels_x, np.int64)
    n = x.shape[1]
    coded = [x[c] for c in range(x.shape[0])]
    if ch_tag == 8:
        coded = [x[0], x[0] - x[1]]
    elif ch_tag == 9:
        coded = [x[0] - x[1], x[1]]
    elif ch_tag == 10:
        coded = [(x[0] + x[1]) >> 1, x[0] - x[1]]
    w = BitWriter()
    w.bits = list(np.unpackbits(np.frombuffer(header(n, ch_tag, bps, number, variable, **hdr), np.uint8)))
    for c, sf in enumerate(subframes):
        side = (ch_tag == 8 and c == 1) or (ch_tag == 9 and c == 0) or (ch_tag == 10 and c == 1)
        write_subframe(w, coded[c], bps + (1 if side else 0), **sf)
    w.align()
    b = w.bytes()
    return b + crc16(b).to_bytes(2, "big")
