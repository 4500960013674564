"""What flacenc_hip_encode_streams_planar reads, stated in numpy: the quantiser q of float32 elements, where a stream's
rows lie in `samples`, and the packed PCM P_s the equivalence rule and the digests are stated over.

    q(x) = clamp(rne(x * 2^(bits - 1)), -2^(bits - 1), 2^(bits - 1) - 1), the product in float32, every NaN 0

The model forms the product in float32 (numpy keeps float32 * float32 in float32) and rounds with np.rint (ties to
even); q_exact below is the independent statement in float64 / Python integers the CPU test holds it to."""
import collections
import fractions
import math

import numpy as np

from flacenc_rs_amd import _capi


def q(x, bits):
    """float32 array -> (int32 samples, bool: the element clamped or was a NaN)."""
    x = np.asarray(x, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        v = x * np.float32(2.0 ** (bits - 1))
    assert v.dtype == np.float32
    nan = np.isnan(v)
    r = np.rint(np.where(nan, np.float32(0), v)).astype(np.float64)   # +-inf stays +-inf
    lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
    clipped = nan | (r < lo) | (r > hi)
    return np.clip(r, lo, hi).astype(np.int32), clipped


def q_exact(x, bits):
    """One float (a Python float holding a float32 value) -> (sample, clipped), without float32 arithmetic: the product
    of a float32 and a power of two is exact short of overflow, so it is the rational x * 2^(bits-1); overflow can only
    clamp."""
    lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
    if math.isnan(x):
        return 0, True
    if math.isinf(x):
        return (hi, True) if x > 0 else (lo, True)
    v = fractions.Fraction(x) * (1 << (bits - 1))
    # (a denormal times 2^(bits-1) is exact as a rational; in float32 it may round or flush, but it stays below 2^-100)
    f = v.numerator // v.denominator          # floor
    rest = v - f
    r = f if rest < fractions.Fraction(1, 2) else f + 1 if rest > fractions.Fraction(1, 2) else f + (f & 1)
    return (hi, True) if r > hi else (lo, True) if r < lo else (r, False)


def float_cases(bits):
    """The float32 elements both tests quantise: every tie (k +- 0.5) / 2^(bits-1) for k around both clamp edges and
    around 0, each with its two float neighbours; +-0; denormals; +-1; +-(1 - ulp); +-FLT_MAX; +-inf; quiet and signalling
    NaNs of both signs.  (Where k + 0.5 needs more than 24 bits the cast rounds it: still an element worth asking.)"""
    lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
    ks = [k for c in (lo, 0, hi) for k in range(c - 3, c + 4)]
    ties = np.array([(k + h) / 2.0 ** (bits - 1) for k in ks for h in (-0.5, 0.0, 0.5)], np.float64).astype(np.float32)
    parts = [ties, np.nextafter(ties, np.float32(np.inf)), np.nextafter(ties, np.float32(-np.inf))]
    fmax = np.finfo(np.float32).max
    one_less = np.nextafter(np.float32(1), np.float32(0))
    parts.append(np.array([0.0, -0.0, 1.0, -1.0, one_less, -one_less, fmax, -fmax, np.inf, -np.inf], np.float32))
    bit_patterns = [0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x00400000,      # denormals
                    0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001, 0x7FBFFFFF, 0xFFFFFFFF]   # quiet / signalling NaNs
    parts.append(np.array(bit_patterns, np.uint32).view(np.float32))
    return np.concatenate(parts)


def unscale(v, bits):
    """The decoder's F32 rule: (float32)v * 2^-(bits - 1)."""
    return np.asarray(v, np.int32).astype(np.float32) * np.float32(2.0 ** -(bits - 1))


def pack(x, width):
    """int32 [channels, total] -> P_s: interleaved little-endian bytes, `width` per sample (the low bytes)."""
    flat = np.ascontiguousarray(np.asarray(x, np.int32).T).reshape(-1).astype("<i4")
    return np.ascontiguousarray(flat.view(np.uint8).reshape(-1, 4)[:, :width]).reshape(-1)


Planar = collections.namedtuple("Planar", "samples table out_bytes row_pitch elements")


def layout(rows, descs, row_pitch, residues=(0, 4, 8, 12), fill=0, last_at_end=True, dtype=np.int32):
    """rows[i]: [channels, total] elements of stream i (int32, or float32 viewed as it is); descs[i]: (out_offset,
    out_capacity, bits, width, rate).  -> Planar: `samples` (a 1-D array of 4-byte elements of `dtype`) with stream i's
    rows at pitch row_pitch (0: tight), its first element at a byte offset that is residues[i % len] mod 16, every element
    that is no valid element of a stream (gaps, pitch padding) holding the bit pattern `fill`; the last stream's last
    valid element is the buffer's last element.  `elements`: bool mask of the valid elements."""
    at, offs = 0, []
    for i, r in enumerate(rows):
        c, n = r.shape
        pitch = row_pitch or n
        want = residues[i % len(residues)] // 4
        at += (want - at) % 4 + 4          # at least a gap of four elements, then the residue
        offs.append(at)
        at += (c - 1) * pitch + n if n else 0
    total = max(at, 1)
    buf = np.full(total, fill, np.uint32)
    valid = np.zeros(total, bool)
    table = np.zeros(len(rows), _capi.PCM_STREAM_DESC_DTYPE)
    for i, r in enumerate(rows):
        c, n = r.shape
        pitch = row_pitch or n
        for ch in range(c):
            lo = offs[i] + ch * pitch
            buf[lo:lo + n] = np.ascontiguousarray(r[ch]).view(np.uint32)
            valid[lo:lo + n] = True
        out_offset, cap, bits, width, rate = descs[i]
        table[i] = (offs[i] * 4, n, out_offset, cap, c, bits, width, rate)
    out_bytes = int(max((int(d["out_offset"]) + int(d["out_capacity"]) for d in table), default=0)) + 3
    return Planar(buf.view(dtype), table, out_bytes, row_pitch, valid)


def check_rows(table, sample_format, row_pitch, samples_bytes):
    """The argument rules the planar call adds, in Python integers: True where the call must accept the rows."""
    if sample_format not in (_capi.SAMPLE_I32, _capi.SAMPLE_F32):
        return False
    for d in table:
        off, n, c = int(d["offset"]), int(d["total_samples"]), int(d["channels"])
        if off % 4 or off > samples_bytes or (row_pitch and row_pitch < n):
            return False
        pitch = row_pitch or n
        if n and off + ((c - 1) * pitch + n) * 4 > samples_bytes:
            return False
    return True
