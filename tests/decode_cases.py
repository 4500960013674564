"""The deterministic corpus of the batched decoder suites (tests/test_gpu_decode_batched.py on the GPU,
tests/test_decode_cases_cpu.py on the host core and tests/flac_parse.py alone).  Frames come from tests/flac_write.py
(independent of the product), from test_decode_core_cpu.oracle_corpus() / crafted_corpus(), and from a byte-level
assembler of mono Verbatim frames below.  Every case carries the samples it was written from: that array is the
reference, the host core is only a second witness for statuses.

groups() sorts the cases by (channels, bits_per_sample) -- one launch has one stream format -- and the layout functions
turn a group into a launch.  The module also states, from the frame list alone, which subframes share a wave of
subframe_kernel (wave_table) and which single-bit flips must be detected (damage_points); the CPU test asserts those
claims, so a GPU case reaches what it names before it compares a sample."""
import collections
import functools

import numpy as np

import flac_write as fw
import test_decode_core_cpu as corpora

# name, frame bytes, channels, bits per sample, samples int64 [channels, n], coded number, per channel (kind, order) or
# None where the case came from a corpus that does not say, and a note on how the case was checked
Case = collections.namedtuple("Case", "name data channels bps x number subs note")

BUCKETS = (4, 8, 16, 32)


def bucket(order):
    return 4 if order <= 4 else 8 if order <= 8 else 16 if order <= 16 else 32


# ---------------------------------------------------------------- CRCs by table (flac_parse has the bitwise forms)
def _table(poly, bits):
    top, mask = 1 << (bits - 1), (1 << bits) - 1
    t = []
    for i in range(256):
        c = i << (bits - 8)
        for _ in range(8):
            c = ((c << 1) ^ poly) & mask if c & top else (c << 1) & mask
        t.append(c)
    return t


_T8, _T16 = _table(0x07, 8), _table(0x8005, 16)


def crc8(data):
    c = 0
    for b in data:
        c = _T8[c ^ b]
    return c


def crc16(data):
    c = 0
    for b in data:
        c = ((c << 8) & 0xFFFF) ^ _T16[(c >> 8) ^ b]
    return c


# ---------------------------------------------------------------- mono Verbatim / Constant frames, byte by byte
def verbatim_frame(x, bps, number=0, variable=False):
    """A mono Verbatim frame of 8- or 16-bit samples: the header, the subframe header 0b0_000001_0, the samples as they
    are, the CRC-16.  Block sizes to 65536."""
    x = np.asarray(x, np.int64)
    assert bps in (8, 16) and x.ndim == 1
    body = x.astype(">i2" if bps == 16 else "i1").tobytes()
    b = fw.header(len(x), 0, bps, number, variable) + b"\x02" + body
    return b + crc16(b).to_bytes(2, "big")


def constant_frame(value, n, bps, number=0, variable=False):
    b = fw.header(n, 0, bps, number, variable) + b"\x00" + int(value).to_bytes(bps // 8, "big", signed=True)
    return b + crc16(b).to_bytes(2, "big")


def mono8_frame_of_length(total, number, rng, variable=False):
    """-> (bytes, samples, number) of a mono 8-bit Verbatim frame of exactly `total` bytes (total >= 11).  Where the
    block-size field grows from 8 to 16 bits no block size gives the length with a one-byte number; a longer coded
    number (number + 128, number + 2048) then fills the byte or two."""
    for num in (number, number + 128, number + 2048):
        for n in range(max(1, total - 16), total):
            if len(fw.header(n, 0, 8, num, variable)) + 1 + n + 2 == total:
                x = rng.integers(-128, 128, n).astype(np.int64)
                return verbatim_frame(x, 8, num, variable), x, num
    raise AssertionError(("no mono 8-bit Verbatim frame of this length", total, number))


def signal(rng, n, bps, kind="smooth"):
    return corpora.signal(rng, n, bps, kind)


# ---------------------------------------------------------------- arithmetic corners
def full_scale(rng, n, bps, pattern):
    """Samples at the two ends of the range, signed so that sum c_j x[t-1-j] is as large as the pattern allows on about
    half of the positions, with a few values from the middle of the range."""
    lo, hi = -(1 << (bps - 1)), (1 << (bps - 1)) - 1
    t = np.arange(n)
    if pattern == "alt":
        x = np.where(t % 2 == 0, hi, lo)
    elif pattern == "neg":
        x = np.where((t // 40) % 2 == 0, lo, hi)
    else:
        x = np.where((t // 40) % 2 == 0, hi, lo)
    x = x.astype(np.int64)
    mid = rng.integers(0, n, n // 8)
    x[mid] = rng.integers(lo, hi + 1, len(mid))
    return x


def pattern_coefs(pattern, m, order=32):
    """`pos`: every coefficient m; `neg`: every coefficient -m - 1; `alt`: m, -m - 1, m, ... (m = 16383 gives the ends
    of the 15-bit range)."""
    if pattern == "pos":
        return [m] * order
    if pattern == "neg":
        return [-m - 1] * order
    return [m if j % 2 == 0 else -m - 1 for j in range(order)]


def residual_fits(x, coefs, shift):
    e = fw.residuals(x, coefs, shift, len(coefs))
    return -(1 << 31) <= int(e.min()) and int(e.max()) < (1 << 31), e


def largest_magnitude(x, pattern, shift):
    """The largest m in 0..16383 for which the residual of x under pattern_coefs(pattern, m) >> shift fits an int32
    (RFC 9639 section 9.2.7), by bisection on the residual computed in Python integers; the CPU test asserts the fit at
    m and the misfit at m + 1."""
    if residual_fits(x, pattern_coefs(pattern, 16383), shift)[0]:
        return 16383
    lo, hi = 0, 16383  # fits at lo, not at hi
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if residual_fits(x, pattern_coefs(pattern, mid), shift)[0]:
            lo = mid
        else:
            hi = mid
    return lo


def corner_subframe(x, pattern, shift):
    m = largest_magnitude(x, pattern, shift)
    coefs = pattern_coefs(pattern, m)
    ok, e = residual_fits(x, coefs, shift)
    assert ok
    note = "order 32 precision 15 %s m=%d shift=%d: residual in [%d, %d], bisected" % (pattern, m, shift, e.min(),
                                                                                       e.max())
    return dict(kind="lpc", order=32, coefs=coefs, precision=15, shift=shift, method=1), note


@functools.lru_cache(None)
def corner_cases():
    """LPC order 32, precision 15, the three coefficient patterns at shifts 0..15 on full-scale 24-bit samples (mono),
    and on a 24-bit left/side frame whose side channel needs all 25 bits."""
    rng = np.random.default_rng(0xC0121E12)
    out = []
    for i, shift in enumerate(range(16)):
        pattern = ("pos", "neg", "alt")[i % 3]
        for pat in (pattern, ("pos", "neg", "alt")[(i + 1) % 3]) if shift in (0, 14, 15) else (pattern,):
            n = (72, 80, 97)[i % 3]
            x = full_scale(rng, n, 24, pat)
            sf, note = corner_subframe(x, pat, shift)
            out.append(Case("corner24 %s shift %d" % (pat, shift), fw.frame(x[None], 0, 24, [sf], number=shift), 1, 24,
                            x[None], shift, (("lpc", 32),), note))
    for i, shift in enumerate((0, 7, 13, 14, 15)):
        pat = ("alt", "pos", "neg")[i % 3]
        n = 96 + i
        left = full_scale(rng, n, 24, pat)
        right = -1 - left                      # the other end of the range: side = left - right = 2 left + 1
        right[::7] = left[::7]
        x = np.stack([left, right])
        side = left - right
        assert side.max() == (1 << 24) - 1 and side.min() == -(1 << 24) + 1
        sf0, note0 = corner_subframe(left, pat, shift)
        sf1, note1 = corner_subframe(side, pat, shift)
        out.append(Case("corner25 %s shift %d" % (pat, shift), fw.frame(x, 8, 24, [sf0, sf1], number=shift), 2, 24, x,
                        shift, (("lpc", 32), ("lpc", 32)), note0 + "; side: " + note1))
    return out


@functools.lru_cache(None)
def side_cases():
    """All three side assignments (and independent) at 8, 16 and 24 bits: l, r at opposite ends of the range, odd and
    even l + r, then noise."""
    rng = np.random.default_rng(0x51DE)
    out = []
    for bps in (8, 16, 24):
        lo, hi = -(1 << (bps - 1)), (1 << (bps - 1)) - 1
        for tag, rep in [(t, k) for k in (0, 1) for t in (8, 9, 10, 1)]:
            n = 40 + bps + tag + 13 * rep
            l = signal(rng, n, bps, "noise")
            r = signal(rng, n, bps, "noise")
            l[:10] = [hi, lo, hi, lo, hi, lo, 0, -1, 1, 3]
            r[:10] = [lo, hi, hi, lo, hi - 1, lo + 1, -1, 0, 2, -4]
            assert {int(v) & 1 for v in (l + r)[:10]} == {0, 1}
            x = np.stack([l, r])
            sfs = [dict(kind="fixed", order=1 + rep, method=1), dict(kind="verbatim")]
            if (tag == 9) != (rep == 1):
                sfs = sfs[::-1]
            subs = tuple((s["kind"], s.get("order", 0)) for s in sfs)
            out.append(Case("side tag %d bps %d %d" % (tag, bps, rep), fw.frame(x, tag, bps, sfs, number=tag), 2, bps,
                            x, tag, subs, "l, r at opposite ends; odd and even l + r"))
    return out


# ---------------------------------------------------------------- frame lengths for the CRC-16
SWEEP = range(8, 801)  # every value of (frame length - 2) that the sweep holds


@functools.lru_cache(None)
def crc_sweep_cases():
    """Mono 8-bit frames whose length - 2 takes every value of SWEEP: all 256 residues of crc16_kernel's 256-byte
    rounds, across 256, 512 and 768.  Length 10 (length - 2 = 8) is the shortest frame the writer can make: a 6-byte
    header (block size from the table, a one-byte number), a Constant subframe of one header byte and one sample, the
    CRC."""
    rng = np.random.default_rng(0xC2C16)
    out = [Case("crc len 10", constant_frame(-77, 192, 8, 5), 1, 8, np.full((1, 192), -77, np.int64), 5,
                (("constant", 0),), "the minimum length")]
    for lm2 in SWEEP[1:]:
        total = lm2 + 2
        if total == 11:
            data, x, number = constant_frame(19, 17, 8, 3), np.full(17, 19, np.int64), 3   # 7-byte header
        else:
            data, x, number = mono8_frame_of_length(total, lm2 % 128, rng)
        assert len(data) == total
        kind = "constant" if total == 11 else "verbatim"
        out.append(Case("crc len %d" % total, data, 1, 8, x[None], number, ((kind, 0),), ""))
    return out


@functools.lru_cache(None)
def big_frame_case():
    """One frame above 64 KiB: mono 16-bit Verbatim, 32768 samples."""
    rng = np.random.default_rng(0xB16)
    x = signal(rng, 32768, 16, "noise")
    data = verbatim_frame(x, 16, 9)
    assert len(data) > 65536
    return Case("big verbatim 32768", data, 1, 16, x[None], 9, (("verbatim", 0),), "above 64 KiB")


# ---------------------------------------------------------------- subframes in company: one wave per register bucket
def _small_subframe(rng, kind, order, n):
    """-> (samples, write_subframe keywords) of a short mono 16-bit subframe."""
    if kind == "constant":
        return np.full(n, int(rng.integers(-30000, 30000)), np.int64), dict(kind="constant")
    x = signal(rng, n, 16, "noise" if kind == "verbatim" else "smooth")
    if kind == "verbatim":
        return x, dict(kind="verbatim")
    if kind == "fixed":
        return x, dict(kind="fixed", order=order)
    coefs, shift = corpora.lpc_coefs(rng, order, 12)
    return x, dict(kind="lpc", order=order, coefs=[int(c) for c in coefs], precision=12, shift=shift,
                   method=int(order) & 1)


@functools.lru_cache(None)
def company_cases():
    """256 mono 16-bit frames = the four waves of one subframe_kernel workgroup when they lead a launch: wave b's
    largest order lies in bucket BUCKETS[b], and it also holds smaller orders.  Wave 3 mixes block sizes 1..32768 with
    Constant, Verbatim, Fixed and LPC subframes."""
    rng = np.random.default_rng(0xC0111)
    out = []
    for w, top in enumerate(BUCKETS):
        for i in range(64):
            n = int(rng.integers(top + 1, 100))
            kind = ("fixed", "lpc", "constant", "verbatim", "lpc", "fixed", "lpc", "lpc")[i % 8]
            if kind == "lpc":
                lowest = 1 if i % 16 != 1 else top // 2 + (1 if top > 4 else 0)
                order = int(rng.integers(lowest, top + 1)) if i > 1 else top
            elif kind == "fixed":
                order = i % 5
            else:
                order = 0
            if w == 3 and i in (7, 18, 29, 40, 51):
                n = {7: 1, 18: 32768, 29: 4097, 40: 16, 51: 16384}[i]
                kind, order = {7: ("verbatim", 0), 18: ("constant", 0), 29: ("fixed", 2), 40: ("lpc", 16),
                               51: ("verbatim", 0)}[i]
            number = w * 64 + i
            if kind == "verbatim" and n >= 4096:
                x = signal(rng, n, 16, "noise")
                data = verbatim_frame(x, 16, number)
            else:
                x, sf = _small_subframe(rng, kind, order, n)
                data = fw.frame(x[None], 0, 16, [sf], number=number)
            out.append(Case("company %d/%d %s %d n=%d" % (w, i, kind, order, n), data, 1, 16, x[None], number,
                            ((kind, order),), ""))
    return out


def wave_table(cases, channels):
    """Which subframes share a wave: lane lf * channels + c of a workgroup of 256 // channels frames holds subframe c of
    the workgroup's frame lf, and a wave is 64 lanes.  -> per wave (in launch order) a list of (kind, order, block
    size); every case must say its subframes."""
    per = 256 // channels
    waves = []
    for g in range(0, len(cases), per):
        lanes = [(k, o, c.x.shape[1]) for c in cases[g:g + per] for k, o in c.subs]
        waves += [lanes[i:i + 64] for i in range(0, len(lanes), 64)]
    return waves


def bucket_claims(waves):
    """-> {bucket: the indices of the waves whose largest order lies in it and that also hold an order from a smaller
    bucket (bucket 4: at least two different orders)}"""
    out = {b: [] for b in BUCKETS}
    for i, lanes in enumerate(waves):
        bs = [bucket(o) for _, o, _ in lanes]
        top = max(bs)
        if (top == 4 and len({o for _, o, _ in lanes}) > 1) or (top > 4 and min(bs) < top):
            out[top].append(i)
    return out


# ---------------------------------------------------------------- the groups
def _imported():
    out = []
    for i, (data, nch, bps, x) in enumerate(corpora.oracle_corpus()):
        out.append(Case("oracle %d" % i, data, nch, bps, np.asarray(x, np.int64), None, None, ""))
    for i, (data, nch, bps, x, number) in enumerate(corpora.crafted_corpus()):
        out.append(Case("crafted %d" % i, data, nch, bps, np.asarray(x, np.int64), number, None, ""))
    return out


@functools.lru_cache(None)
def groups():
    """{(channels, bps): [Case]} in a fixed order; the company leads the mono 16-bit group."""
    cases = company_cases() + [big_frame_case()] + _imported() + corner_cases() + side_cases() + crc_sweep_cases()
    out = collections.OrderedDict()
    for c in cases:
        out.setdefault((c.channels, c.bps), []).append(c)
    return out


def max_block_size(cases):
    return max(c.x.shape[1] for c in cases)


# ---------------------------------------------------------------- damage with a known verdict
def header_bytes(data):
    """The length of a frame's header, CRC-8 included (RFC 9639 section 9.1)."""
    n = 4
    first = data[4]
    ones = 0
    while (first >> (7 - ones)) & 1:
        ones += 1
    n += max(1, ones)
    bs_code, sr_code = data[2] >> 4, data[2] & 15
    n += 1 if bs_code == 6 else 2 if bs_code == 7 else 0
    n += 1 if sr_code == 12 else 2 if sr_code in (13, 14) else 0
    return n + 1


def damage_points(data):
    """(label, bit index from the frame's first bit) of the single-bit flips with a required verdict: a CRC-16 detects
    every single-bit error and the header checks come first, so each must give a non-zero status."""
    h, n = header_bytes(data), len(data)
    pts = [("sync", 3), ("sync low", 13), ("reserved", 14), ("blocking", 15), ("block size", 17), ("sample rate", 22),
           ("channels", 25), ("sample size", 29), ("reserved 2", 31), ("number", 8 * 4 + 6), ("crc8", 8 * (h - 1) + 2),
           ("body first", 8 * h + 1), ("body last", 8 * (n - 3) + 7), ("crc16 hi", 8 * (n - 2) + 4),
           ("crc16 lo", 8 * (n - 1))]
    if n > 65536:  # one flip per position class of crc16_kernel's 256-byte rounds
        rounds = (n - 2 + 255) // 256
        pad = rounds * 256 - (n - 2)
        for label, r in (("first round", 0), ("middle round", rounds // 2), ("last round", rounds - 1)):
            for lane in (0, 31, 63):
                q = max(r * 256 + 4 * lane - pad, h + 1)
                pts.append(("%s lane %d" % (label, lane), 8 * q + lane % 8))
    return pts


def flip(data, bit):
    b = bytearray(data)
    b[bit // 8] ^= 0x80 >> (bit % 8)
    return bytes(b)


def damage_bases(cases):
    """The frames of a group that get damaged copies: the first, one from the middle, the last, and every frame above
    64 KiB."""
    idx = sorted({0, len(cases) // 2, len(cases) - 1} | {i for i, c in enumerate(cases) if len(c.data) > 65536})
    return idx


# ---------------------------------------------------------------- launch layouts
# A launch is (buffer uint8, offsets uint64, lengths uint32, entries); entry f is (Case, None) for a valid frame and
# (Case, label) for a damaged copy of it.
def _launch(blobs, entries):
    lengths = np.array([len(b) for b in blobs], np.uint32)
    offsets = np.concatenate([[0], np.cumsum(lengths[:-1], dtype=np.uint64)]).astype(np.uint64)
    return np.frombuffer(b"".join(blobs), np.uint8).copy(), offsets, lengths, entries


def back_to_back(cases):
    return _launch([c.data for c in cases], [(c, None) for c in cases])


def shuffled(cases, seed=0x5AFE):
    order = np.random.default_rng(seed).permutation(len(cases))
    return back_to_back([cases[i] for i in order])


def interleaved(cases):
    """Every valid frame in order; after each damage base, its single-bit-damaged copies."""
    bases = set(damage_bases(cases))
    blobs, entries = [], []
    for i, c in enumerate(cases):
        blobs.append(c.data)
        entries.append((c, None))
        if i in bases:
            for label, bit in damage_points(c.data):
                blobs.append(flip(c.data, bit))
                entries.append((c, label))
    return _launch(blobs, entries)


def expected_rows(entries, channels, mbs, stride=None):
    """The ground truth of a launch: int32 [n, channels, stride], zero beyond each block and on damaged frames."""
    out = np.zeros((len(entries), channels, stride or mbs), np.int32)
    for f, (c, label) in enumerate(entries):
        if label is None:
            out[f, :, :c.x.shape[1]] = c.x
    return out


# ---------------------------------------------------------------- multichannel and stereo launches
@functools.lru_cache(None)
def channel_cases(channels):
    """Short frames (blocks of 64..192 samples) of `channels` independent channels, or of stereo cycling the four
    assignments: enough for more than three workgroups of 256 // channels frames, and no multiple of that."""
    rng = np.random.default_rng(0xC4A00 + channels)
    per = 256 // channels
    count = 301 if channels == 2 else 3 * per + max(1, per // 3)
    assert count % per and (count > 3 * per or channels == 2)
    out = []
    for f in range(count):
        n = int(rng.integers(64, 193))
        x = np.stack([signal(rng, n, 16, "smooth" if (f + c) % 3 else "noise") for c in range(channels)])
        tag = (0 if channels == 1 else channels - 1) if channels != 2 else (1, 8, 9, 10)[f % 4]
        sfs, subs = [], []
        for c in range(channels):
            kind, order = (("fixed", (f + c) % 5), ("verbatim", 0), ("lpc", 1 + (f * 5 + c * 3) % 12),
                           ("constant", 0), ("lpc", 1 + (f + c) % 32))[(f + 2 * c) % 5]
            if kind == "constant":
                if channels == 2 and tag != 1:
                    kind, order = "fixed", 0      # a coded side channel is rarely constant
                else:
                    x[c] = x[c, 0]
            if kind == "lpc":
                coefs, shift = corpora.lpc_coefs(rng, order, 10)
                sfs.append(dict(kind="lpc", order=order, coefs=[int(v) for v in coefs], precision=10, shift=shift))
            elif kind == "fixed":
                sfs.append(dict(kind="fixed", order=order))
            else:
                sfs.append(dict(kind=kind))
            subs.append((kind, order))
        out.append(Case("ch%d frame %d" % (channels, f), fw.frame(x, tag, 16, sfs, number=f), channels, 16, x, f,
                        tuple(subs), "tag %d" % tag))
    return out


# ---------------------------------------------------------------- index streams
# An index stream is (name, bytes, offsets uint64, lengths uint32, channels, bps).
def _stream(name, frames, channels, bps, front=b""):
    lengths = np.array([len(b) for b in frames], np.uint32)
    offsets = (np.concatenate([[0], np.cumsum(lengths[:-1], dtype=np.uint64)]) + len(front)).astype(np.uint64) \
        if len(frames) else np.zeros(0, np.uint64)
    return name, front + b"".join(frames), offsets, lengths, channels, bps


@functools.lru_cache(None)
def tiny_stream(variable=False, n_frames=3000):
    """Mono 8-bit frames of 10..40 bytes (Constant and tiny Verbatim blocks): a lane of streams_cand_kernel's 16 positions
    holds up to two of them, a workgroup's 4096 positions more than a hundred."""
    rng = np.random.default_rng(0x7177 + variable)
    frames, at = [], 0
    for f in range(n_frames):
        number = at if variable else f
        if f % 3 == 0:
            n = (192, 576, 256, 17)[(f // 3) % 4]
            frames.append(constant_frame(int(rng.integers(-128, 128)), n, 8, number, variable))
        else:
            n = int(rng.integers(1, 28))
            frames.append(verbatim_frame(rng.integers(-128, 128, n), 8, number, variable))
        at += n
    assert 8 <= min(map(len, frames)) and max(map(len, frames)) <= 40
    return _stream("tiny variable" if variable else "tiny fixed", frames, 1, 8)


SEAM_STARTS = (15, 32, 4095, 8192, 12289, 16384)  # 15 and 0 mod 16; 4095, 0 and 1 mod 4096; a workgroup's first again


@functools.lru_cache(None)
def seam_stream():
    """Mono 8-bit Verbatim frames of mixed sizes (11 to some 800 bytes, variable blocking) with a true frame starting at
    each of SEAM_STARTS: the last position of a lane of the candidate kernels, the first of the next, and the last,
    first and second position of a workgroup."""
    rng = np.random.default_rng(0x5EA)
    frames, at = [], 0
    for t in SEAM_STARTS + (16395, 16424, 21000):
        while at < t:
            gap = t - at
            size = gap if gap <= 800 else int(rng.integers(300, 700))
            if 0 < gap - size < 11:
                size -= 11
            frames.append(mono8_frame_of_length(size, len(frames) % 128, rng, variable=True)[0])
            at += size
    s = _stream("seams", frames, 1, 8)
    assert set(SEAM_STARTS) <= set(int(o) for o in s[2])
    return s


def one_frame_stream():
    return _stream("one frame", [constant_frame(3, 192, 8, 0)], 1, 8)


def empty_stream():
    return _stream("empty", [], 1, 8)


def candidate_capacity(max_frames):
    """index_candidate_capacity of stream_index.cpp, as the header states it."""
    return max_frames + max_frames // 4 + 4096


def planted_field_stream(n_planted):
    """Three mono 16-bit Verbatim frames of 32768, 1152 and 1152 samples; the first one's samples spell n_planted valid
    6-byte headers back to back, so the buffer holds n_planted + 3 candidate headers."""
    rng = np.random.default_rng(0xF1E1D)
    xs = [np.abs(signal(rng, n, 16)) // 2 for n in (32768, 1152, 1152)]   # no byte 0xFF outside the headers
    fake = b"".join(fw.header(1152, 0, 16, k % 128) for k in range(n_planted))
    spelled = np.frombuffer(fake, ">i2").astype(np.int64)
    assert 3 * n_planted == len(spelled) <= 32768 - 64
    xs[0][32:32 + len(spelled)] = spelled
    frames = [verbatim_frame(x, 16, f) for f, x in enumerate(xs)]
    return _stream("planted %d" % n_planted, frames, 1, 16)


def is_candidate(data, p, channels, bps):
    """stream_index.cpp's is_candidate, from RFC 9639 section 9.1: a header valid for the stream, CRC-8 included."""
    d = data[p:p + 16]
    if len(d) < 2 or d[0] != 0xFF or (d[1] & 0xFE) != 0xF8:
        return False
    try:
        bs_code, sr_code, ch_code, ss_code = d[2] >> 4, d[2] & 15, d[3] >> 4, (d[3] >> 1) & 7
        if d[3] & 1 or bs_code == 0 or sr_code == 15 or ch_code > 10 or ss_code == 3:
            return False
        ones = 0
        while ones < 8 and (d[4] >> (7 - ones)) & 1:
            ones += 1
        if ones in (1, 8) or any((b >> 6) != 2 for b in d[5:4 + max(1, ones)]):
            return False
        n = 4 + max(1, ones) + (1 if bs_code == 6 else 2 if bs_code == 7 else 0) + \
            (1 if sr_code == 12 else 2 if sr_code in (13, 14) else 0)
        if crc8(d[:n]) != d[n]:
            return False
    except IndexError:
        return False
    depth = {0: bps, 1: 8, 2: 12, 4: 16, 5: 20, 6: 24, 7: 32}[ss_code]
    return (ch_code + 1 if ch_code < 8 else 2) == channels and depth == bps


def count_candidates(data, channels, bps):
    a = np.frombuffer(data, np.uint8)
    hits = np.flatnonzero((a[:-1] == 0xFF) & ((a[1:] & 0xFE) == 0xF8))
    return sum(is_candidate(data, int(p), channels, bps) for p in hits)
