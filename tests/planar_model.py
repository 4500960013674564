"""What flacenc_hip_decode_ranges_planar must give, built from what flacenc_hip_decode_ranges must give
(tests/ranges_model.py) by the header's rule and nothing else: sign-extend and de-interleave the packed samples, scale for
F32, zero-pad every row to n_samples.  Elements are compared as bit patterns (uint32), so +0.0f and the rounding of every
value are part of the comparison.  Also the layout of a planar call over a ranges_cases.RangeBatch: slots in shuffled
order at offsets that are multiples of 4 with chosen residues mod 16 and FILL between them.  No GPU is needed to build
any of it; tests/test_decode_ranges_planar_cpu.py proves the builder, tests/test_gpu_decode_ranges_planar.py uses it."""
import numpy as np

import streams_cases
from flacenc_rs_amd import _capi

FILL = streams_cases.FILL


def values_of(packed, channels, width):
    """Packed interleaved little-endian samples of `width` bytes -> int32 [channels, samples], sign-extended from the
    container's top bit."""
    raw = np.asarray(packed, np.uint8).reshape(-1, channels, width)
    wide = np.zeros(raw.shape[:2] + (4,), np.uint8)
    wide[..., :width] = raw
    wide[..., width:] = np.where(raw[..., width - 1:width] & 0x80, 0xFF, 0)
    return np.ascontiguousarray(wide.reshape(-1, channels * 4).view("<i4").T).astype(np.int32)


def elements_of(values, bps, sample_format):
    """int32 values -> the elements' bit patterns: the value itself, or float32(value) * 2^-(bps - 1)."""
    v = np.asarray(values, np.int32)
    if sample_format == _capi.SAMPLE_I32:
        return v.view(np.uint32).copy()
    scaled = v.astype(np.float32) * np.float32(2.0 ** -(bps - 1))   # int32 -> float32 rounds to nearest even
    return scaled.astype(np.float32).view(np.uint32).copy()


def slot_of(packed, channels, width, bps, n_samples, sample_format):
    """The whole slot of one range, uint32 [channels, n_samples]: the elements of its packed samples, zeros behind."""
    v = values_of(packed, channels, width)
    out = np.zeros((channels, n_samples), np.uint32)
    out[:, :v.shape[1]] = elements_of(v, bps, sample_format)
    return out


def expected_slots(rb, want, sample_format):
    """Per range of a RangeBatch, from ranges_model.expected_batch(rb): (uint32 [channels, n_samples], totals)."""
    out = []
    for (s, first, n), (data, tot) in zip(rb.ranges, want):
        st = rb.streams[s]
        out.append((slot_of(data, st.channels, st.width, st.bps, n, sample_format), tot))
    return out


def odd_streams():
    """Single-frame streams in a 4-byte container whose values need more than the stream's bit depth or reach its ends:
    the order-32 corners and the full-width side channels of tests/decode_cases.py, wasted bits and escaped partitions of
    the crafted corpus, and two frames written here -- residuals far above 16 bits on a 16-bit stream, and a fixed
    predictor whose running sum leaves the int32 range, so that the reconstruction wraps.  -> [streams_cases.Stream]"""
    import decode_cases as dc
    import flac_write as fw
    import test_decode_core_cpu as corpora
    out = []

    def add(name, data, channels, bps, n):
        out.append(streams_cases.Stream(name, data, channels, bps, max(n, 16), None, 4, [(len(data), n)]))

    for c in dc.corner_cases()[::3] + dc.corner_cases()[-5:] + dc.side_cases():
        add(c.name, c.data, c.channels, c.bps, c.x.shape[1])
    for i, (data, nch, bps, x, _) in enumerate(corpora.crafted_corpus()[:15]):
        add("crafted %d" % i, data, nch, bps, x.shape[1])
    rng = np.random.default_rng(0x0DD)
    x = rng.integers(-(1 << 30), 1 << 30, 300).astype(np.int64)
    x[:4] = [(1 << 24) + 1, (1 << 24) + 3, -(1 << 24) - 1, (1 << 30) - 1]   # ties and non-ties of int32 -> float32
    add("over 16 bits", fw.frame(x[None], 0, 16, [dict(kind="fixed", order=0, method=1)]), 1, 16, 300)
    x = 30000 + np.arange(40, dtype=np.int64) * ((1 << 28) + 12345)
    add("wrapping sum", fw.frame(x[None], 0, 16, [dict(kind="fixed", order=1, method=1)]), 1, 16, 40)
    l = rng.integers(-(1 << 29), 1 << 29, 77).astype(np.int64)
    r = rng.integers(-(1 << 29), 1 << 29, 77).astype(np.int64)
    add("over 16 bits left/side", fw.frame(np.stack([l, r]), 8, 16, [dict(kind="fixed", order=0, method=1)] * 2), 2, 16, 77)
    return out


class PlanarLayout:
    """The planar slots of a RangeBatch's ranges in one buffer: shuffled order, every slot at an offset of `residues[k %
    len]` mod 16 behind at least 4 bytes of FILL; rtable is the batch's range table with these offsets."""

    def __init__(self, rb, seed=3, residues=(4, 8, 12, 0)):
        self.rb = rb
        order = np.random.default_rng(seed).permutation(len(rb.ranges))
        self.offsets = [0] * len(rb.ranges)
        self.sizes = [rb.streams[s].channels * n * 4 for s, _, n in rb.ranges]
        at = 0
        for k, r in enumerate(order):
            at += 4
            at += (residues[k % len(residues)] - at) % 16
            self.offsets[r] = at
            at += self.sizes[r]
        self.out_bytes = at + 12
        self.rtable = rb.rtable.copy()
        self.rtable["out_offset"] = self.offsets

    def fresh_out(self):
        return np.full(self.out_bytes, FILL, np.uint8)

    def slot(self, out, r):
        s, _, n = self.rb.ranges[r]
        return out[self.offsets[r]:self.offsets[r] + self.sizes[r]].view(np.uint32).reshape(self.rb.streams[s].channels, n)

    def check(self, out, totals, want_slots):
        """Every slot whole (samples and zeros), every total, FILL everywhere else."""
        mask = np.ones(len(out), bool)
        for r, (slot, tot) in enumerate(want_slots):
            who = (r, self.rb.streams[self.rb.ranges[r][0]].name, self.rb.ranges[r])
            assert [int(v) for v in totals[r]] == tot, who + (totals[r], tot)
            got = self.slot(out, r)
            w = tot[0]
            assert np.array_equal(got[:, :w], slot[:, :w]), who
            assert not got[:, w:].any(), who + ("the tail is not zero",)
            mask[self.offsets[r]:self.offsets[r] + self.sizes[r]] = False
        assert bool((out[mask] == FILL).all()), "bytes outside the slots were written"
