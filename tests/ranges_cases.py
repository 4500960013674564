"""The corpus of the flacenc_hip_decode_ranges tests: ranges over the streams of tests/streams_cases.py (mixed(), stops(),
garbage()) and the layout of a call -- the byte buffer of a streams_cases.Batch, whose descriptors carry slots the call
must ignore, and one output buffer with the ranges' slots in shuffled order, at odd byte offsets and at offsets of 2 mod
4, with FILL between them.  Ground truth is Stream.pcm; frame starts come from offsets_of and frame_sizes.  No GPU is
needed to build any of it: tests/test_decode_ranges_cpu.py proves the corpus' claims on the host build of the decoder
core, tests/test_gpu_decode_ranges.py takes the same ranges to the device."""
import functools

import numpy as np

import streams_cases as cases
from flacenc_rs_amd import _capi

FILL = cases.FILL


def starts_of(s):
    """Position of every frame the stream was written from, and the number of samples."""
    return np.concatenate([[0], np.cumsum([n for _, n in s.frame_sizes])]).astype(np.int64)


def samples_of(s):
    return int(starts_of(s)[-1])


class RangeBatch:
    """streams: streams_cases.Stream objects; ranges: (stream index, first_sample, n_samples) in the caller's order."""
    FILL = FILL

    def __init__(self, streams, ranges, seed=1, gaps=None):
        self.streams, self.ranges = list(streams), [tuple(int(v) for v in r) for r in ranges]
        self.batch = cases.Batch(self.streams, capacities=[0] * len(self.streams), gaps=gaps)
        self.data = self.batch.data
        self.table = self.batch.table.copy()
        # what flacenc_hip_decode_streams would reject and this call never looks at
        self.table["out_offset"] = 1 << 63
        self.table["out_capacity"] = 1 << 63
        order = np.random.default_rng(seed).permutation(len(self.ranges))
        self.slot_offsets = [0] * len(self.ranges)
        self.slot_bytes = [n * self.streams[s].channels * self.streams[s].width for s, _, n in self.ranges]
        at = 0
        for k, r in enumerate(order):
            at += (1, 2, 3, 5, 6, 9)[k % 6]  # FILL in front; slots land at odd offsets and at offsets of 2 mod 4
            self.slot_offsets[r] = at
            at += self.slot_bytes[r]
        self.out_bytes = at + 7
        self.rtable = np.zeros(len(self.ranges), _capi.RANGE_DESC_DTYPE)
        for r, (s, first, n) in enumerate(self.ranges):
            self.rtable[r] = (first, n, self.slot_offsets[r], s, 0)

    def fresh_out(self):
        return np.full(max(1, self.out_bytes), FILL, np.uint8)

    def max_frames(self):
        """Room for every chain and for every range's frames (a range touches at most all frames of its stream)."""
        return max(self.batch.max_frames(), sum(len(self.streams[s].data) // 9 + 1 for s, _, _ in self.ranges))


def shapes(s):
    """name -> (first_sample, n_samples) for one written stream: the range shapes and the places a range stops."""
    st, S = starts_of(s), samples_of(s)
    bs = [n for _, n in s.frame_sizes]
    out = {}
    if not bs:
        return {"empty: nothing asked": (0, 0), "empty: from 0": (0, 5), "empty: beyond": (3, 2)}
    k = 1 if len(bs) > 1 else 0
    out["inside one frame"] = (int(st[k]) + 3, bs[k] - 8)            # skip = 3 (odd), take < bs
    out["exactly one frame"] = (int(st[k]), bs[k])
    if len(bs) >= 3:
        out["three frames, partial ends"] = (int(st[0]) + 5, int(st[2]) + 3 - 5)   # skip = 5, 3 samples of frame 2
    out["first sample"] = (0, 1)
    out["from 0 into the second frame"] = (0, min(S, bs[0] + 2))
    out["nothing asked"] = (min(10, S - 1), 0)
    out["last sample"] = (S - 1, 1)
    out["past the end"] = (S - 10, 25)
    out["begins at the end"] = (S, 4)
    out["begins beyond the end"] = (S + 100, 4)
    out["nothing asked at the end"] = (S, 0)
    out["ends at the end"] = (S - 13, 13)
    return out


@functools.lru_cache(None)
def wide():
    """The first eight streams of mixed() in a 4-byte container: the same samples, sign-extended."""
    out = []
    for s in cases.mixed()[:8]:
        v = np.zeros((len(s.pcm) // s.width, 4), np.uint8)
        v[:, :s.width] = s.pcm.reshape(-1, s.width)
        v[:, s.width:] = np.where(v[:, s.width - 1:s.width] & 0x80, 0xFF, 0)
        out.append(cases.Stream(s.name + " wide", s.data, s.channels, s.bps, s.mbs, v.reshape(-1), 4, s.frame_sizes))
    return out


@functools.lru_cache(None)
def corpus():
    """Every shape on every stream of mixed() (channels 1, 2, 3 and 8; 8 .. 24 bits; every stereo tag; the variable-
    blocking streams; the LPC-32 stream; the 17-sample tail; the empty stream) and of wide(), in one call."""
    streams = cases.mixed() + wide()
    ranges, names = [], []
    for i, s in enumerate(streams):
        for name, (first, n) in shapes(s).items():
            ranges.append((i, first, n))
            names.append((s.name, name))
    return RangeBatch(streams, ranges, seed=21), names


@functools.lru_cache(None)
def many_on_one():
    """33 ranges on the stereo stream that cycles the four tags, in descending order: overlapping, identical, with odd
    skips; next to them ranges on the empty stream and on a mono neighbour."""
    m = cases.mixed()
    s = m[1]
    S = samples_of(s)
    ranges = [(1, max(0, S - 40 - 45 * k + (k % 3)), 97) for k in range(30)] + [(1, 201, 300)] * 3
    assert len(ranges) == 33 and ranges[0][1] > ranges[29][1]
    ranges += [(2, 0, 4), (2, 0, 0), (0, 250, 20)]
    return RangeBatch([m[0], s, m[10]], ranges, seed=22)


def span_from(s, k):
    """The stream from its frame k on: a span that starts at a seek point."""
    off, st = cases.offsets_of(s), starts_of(s)
    fb = s.channels * s.width
    return cases.Stream("%s from frame %d" % (s.name, k), s.data[int(off[k]):], s.channels, s.bps, s.mbs,
                        s.pcm[int(st[k]) * fb:], s.width, s.frame_sizes[k:])


@functools.lru_cache(None)
def damaged():
    """Every stream of stops() with three ranges -- before, across and behind the damage -- between good neighbours.
    -> (batch, [(name, stream index, samples before the damage, reason)])."""
    stops, base = cases.stops()
    m = cases.mixed()
    streams, ranges, info = [], [], []
    for k, (name, (s, frames, why)) in enumerate(stops.items()):
        good = m[k]
        D = sum(n for _, n in s.frame_sizes[:frames])
        streams += [good, s]
        i = len(streams) - 1
        ranges += [(i - 1, 7, 60), (i, max(0, D - 50), min(50, D)), (i, max(0, D - 10), 30), (i, D + 5, 10)]
        info.append((name, i, D, why))
    return RangeBatch(streams, ranges, seed=23), info


@functools.lru_cache(None)
def with_garbage():
    m = cases.mixed()
    streams, ranges = [], []
    for i, g in enumerate(cases.garbage(8)):
        good = m[(5 * i) % len(m)]
        if not good.frame_sizes:
            good = m[0]
        streams += [g, good]
        ranges += [(2 * i, 0, 16), (2 * i, 100, 7), (2 * i + 1, 9, min(90, samples_of(good) - 9))]
    return RangeBatch(streams, ranges, seed=24)
