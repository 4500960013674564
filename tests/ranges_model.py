"""What flacenc_hip_decode_ranges must give for one range, from pieces none of which is code under test: what
tests/streams_model.py says flacenc_hip_decode_streams gives for the range's stream with unlimited room (P its PCM, S its
samples, W its stop reason, where it stopped), the chain's frame starts from the host build of the decoder core, and the
slice rule -- range (first, n) gets samples [first, min(first + n, S)) of P; its reason is 0 when all n were written,
else W when W is non-zero, else DECODE_RANGE_END; its seek point is the chain frame that holds `first`, or where the
chain stopped when first >= S."""
import numpy as np

import streams_model
from flacenc_rs_amd import _capi

UNLIMITED = 1 << 62


class Truth:
    """One stream as flacenc_hip_decode_streams sees it with unlimited room."""

    def __init__(self, s):
        self.frame_bytes = s.channels * s.width
        self.pcm, (frames, self.samples, self.consumed, self.why) = streams_model.expected(
            s.data, s.channels, s.bps, s.mbs, s.width, UNLIMITED)
        self.offsets, self.starts = np.zeros(0, np.int64), np.zeros(1, np.int64)
        if frames:
            dec = streams_model.decoder()
            off, ln, _ = dec.index_frames(np.ascontiguousarray(s.data), s.channels, s.bps, len(s.data) // 9 + 1)
            _, bs, _, _ = dec.decode_frames(np.ascontiguousarray(s.data), off, ln, s.channels, s.bps, s.mbs)
            self.offsets = np.asarray(off[:frames], np.int64)
            self.starts = np.concatenate([[0], np.cumsum(np.asarray(bs[:frames], np.int64))])
        assert int(self.starts[-1]) == self.samples

    def expected(self, first, n):
        """-> (the bytes the slot's front must hold, [samples written, stop reason, seek offset, seek position])."""
        S = self.samples
        end = min(first + n, S)
        written = max(0, end - first)
        why = 0 if written == n else (self.why or _capi.DECODE_RANGE_END)
        if first >= S:
            seek = [self.consumed, S]
        else:
            j = int(np.searchsorted(self.starts, first, side="right")) - 1
            seek = [int(self.offsets[j]), int(self.starts[j])]
        fb = self.frame_bytes
        data = self.pcm[first * fb:end * fb] if written else np.zeros(0, np.uint8)
        return data, [written, why] + seek


_truths = {}


def truth(s):
    """Computed once per Stream object and shared."""
    if id(s) not in _truths:
        _truths[id(s)] = (s, Truth(s))
    return _truths[id(s)][1]


def expected_batch(rb):
    """Per range of a ranges_cases.RangeBatch: (bytes, totals)."""
    return [truth(rb.streams[s]).expected(first, n) for s, first, n in rb.ranges]


def check_batch(rb, out, totals, want=None):
    """The output buffer and totals of one call against the model: every slot's front, totals, FILL everywhere else."""
    want = want or expected_batch(rb)
    mask = np.ones(len(out), bool)
    for r, (data, tot) in enumerate(want):
        got = [int(v) for v in totals[r]]
        assert got == tot, (r, rb.streams[rb.ranges[r][0]].name, rb.ranges[r], got, tot)
        at = rb.slot_offsets[r]
        assert np.array_equal(out[at:at + len(data)], data), (r, rb.streams[rb.ranges[r][0]].name, rb.ranges[r])
        mask[at:at + len(data)] = False
    assert bool((out[mask] == rb.FILL).all()), "bytes outside the ranges' samples were written"
    return want
