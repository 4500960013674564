"""The corpus of the flacenc_hip_decode_streams tests: short streams written frame by frame with tests/flac_write.py
from samples that are kept as ground truth, the damaged and garbage streams, and the layout of a batch (one byte buffer
with gaps between spans, one output buffer with shuffled slots and FILL between them).  No GPU is needed to build any of
it: tests/test_decode_streams_cpu.py proves the corpus' claims on the host build of the decoder core, and
tests/test_gpu_decode_streams.py takes the same streams to the device."""
import functools

import numpy as np

import flac_write as fw
from flacenc_rs_amd import _capi

FILL = 0xEE
GAP = 0xA7  # what the gaps between spans hold unless a test plants something there


class Stream:
    """data: the frames; pcm: the packed PCM the whole stream decodes to (ground truth, from the samples it was written
    from) or None for a stream that has none; mbs: the max_block_size its descriptor states."""

    def __init__(self, name, data, channels, bps, mbs, pcm=None, width=None, frame_sizes=()):
        self.name, self.data = name, np.frombuffer(bytes(data), np.uint8).copy()
        self.channels, self.bps, self.mbs = channels, bps, mbs
        self.width = width or (bps + 7) // 8
        self.pcm = pcm
        self.frame_sizes = tuple(frame_sizes)  # (bytes, block size) of every frame written

    def but(self, name, data=None, mbs=None):
        return Stream(name, self.data if data is None else data, self.channels, self.bps, mbs or self.mbs, None,
                      self.width, self.frame_sizes)


def pack(x, width):
    """int [channels, n] -> interleaved little-endian bytes, the low `width` bytes of every sample."""
    flat = np.ascontiguousarray(np.asarray(x).T).reshape(-1).astype("<i4")
    return np.ascontiguousarray(flat.view(np.uint8).reshape(-1, 4)[:, :width]).reshape(-1)


def signal(rng, n, bps, kind):
    lim = (1 << (bps - 1)) - 1
    if kind == "noise":
        return rng.integers(-lim // 2, lim // 2 + 1, n).astype(np.int64)
    step = max(1, lim // 64)
    return np.clip(np.cumsum(rng.integers(-step, step + 1, n)), -lim // 2, lim // 2).astype(np.int64)


SUBFRAME_KINDS = ("fixed", "lpc4", "verbatim", "lpc8", "constant", "lpc16", "escape", "lpc32", "wasted", "rice2")


def subframe(rng, n, bps, which, side):
    """-> (samples, write_subframe keywords).  `side`: the coded channel may differ from the samples (a stereo tag), so
    kinds that need a special signal (constant, wasted) fall back to fixed."""
    kind = SUBFRAME_KINDS[which % len(SUBFRAME_KINDS)]
    if side and kind in ("constant", "wasted"):
        kind = "fixed"
    if kind == "constant":
        return np.full(n, int(rng.integers(-100, 100)), np.int64), dict(kind="constant")
    if kind == "verbatim":
        return signal(rng, n, bps, "noise"), dict(kind="verbatim")
    x = signal(rng, n, bps, "smooth")
    if kind == "wasted":
        return (x >> 3) << 3, dict(kind="fixed", order=min(2, n), wasted=3)
    if kind == "fixed":
        return x, dict(kind="fixed", order=min(which % 5, n))
    if kind == "escape":
        e = dict(kind="fixed", order=0, params=[("esc", bps + 1)])
        return x, e
    if kind == "rice2":
        return x, dict(kind="fixed", order=min(1, n), method=1)
    top = int(kind[3:])
    order = min(top, n) if which % 3 else min(top // 2 + 1, n)
    coefs = [int(c) for c in rng.integers(-60, 61, order)]
    return x, dict(kind="lpc", order=order, coefs=coefs, precision=12, shift=10)


def written_stream(name, seed, channels, bps, blocks, mbs=None, variable=False, tags=None, kinds=None, silence=False):
    """A stream of len(blocks) frames; frame f has blocks[f] samples.  Stereo cycles the four channel tags.  `kinds`:
    indices into SUBFRAME_KINDS to cycle through; silence: Constant subframes of value 0."""
    rng = np.random.default_rng(seed)
    frames, parts, sizes = [], [], []
    first = 0
    for f, n in enumerate(blocks):
        tag = (0 if channels == 1 else channels - 1)
        if channels == 2:
            tag = (tags or (1, 8, 9, 10))[f % len(tags or (1, 8, 9, 10))]
        xs, sfs = [], []
        for c in range(channels):
            which = (kinds[(f + c) % len(kinds)] if kinds else seed + 3 * f + c)
            x, sf = subframe(rng, n, bps, which, tag >= 8)
            if silence:
                x, sf = np.zeros(n, np.int64), dict(kind="constant")
            xs.append(x)
            sfs.append(sf)
        x = np.stack(xs)
        data = fw.frame(x, tag, bps, sfs, number=first if variable else f, variable=variable)
        frames.append(data)
        parts.append(pack(x, (bps + 7) // 8))
        sizes.append((len(data), n))
        first += n
    pcm = np.concatenate(parts) if parts else np.zeros(0, np.uint8)
    return Stream(name, b"".join(frames), channels, bps, mbs or max(list(blocks) + [16]), pcm, None, sizes)


@functools.lru_cache(None)
def mixed():
    """About two dozen streams: channels 1, 2, 3 and 8; 8, 12, 16, 20 and 24 bits; a short tail under 64 samples;
    variable blocking; every subframe kind of SUBFRAME_KINDS (orders in all four buckets, escapes, wasted bits, RICE2),
    every stereo tag; a run of silence; one empty and one single-frame stream."""
    out = [
        written_stream("mono 16 tail", 1, 1, 16, [256] * 5 + [17]),
        written_stream("stereo 16 tags", 2, 2, 16, [192] * 8 + [40]),
        written_stream("stereo 24", 3, 2, 24, [256, 256, 576, 100]),
        written_stream("3ch 24", 4, 3, 24, [192] * 4 + [33]),
        written_stream("8ch 16", 5, 8, 16, [64] * 6 + [16]),
        written_stream("mono 8", 6, 1, 8, [256] * 7 + [50]),
        written_stream("mono 12", 7, 1, 12, [192] * 3),
        written_stream("stereo 20", 8, 2, 20, [128] * 4 + [63]),
        written_stream("variable stereo", 9, 2, 16, [256, 128, 64, 512, 1152, 16, 333], variable=True),
        written_stream("variable mono", 10, 1, 16, [1152, 16, 700, 35], variable=True),
        written_stream("empty", 11, 2, 16, []),
        written_stream("single frame", 12, 2, 16, [577]),
        written_stream("silence", 13, 2, 16, [1152] * 12, tags=(1,), silence=True),
        written_stream("mono lpc32", 14, 1, 16, [128] * 6, kinds=[7, 5, 3, 1]),
        written_stream("stereo mid/side", 15, 2, 16, [256] * 5, tags=(10,)),
        written_stream("stereo left/side", 16, 2, 16, [256] * 3 + [31], tags=(8,)),
        written_stream("stereo right/side", 17, 2, 8, [256] * 3, tags=(9,)),
        written_stream("wasted mono 24", 18, 1, 24, [192] * 4, kinds=[8]),
        written_stream("escapes 3ch", 19, 3, 16, [64] * 5, kinds=[6, 9]),
        written_stream("8ch 24", 20, 8, 24, [32] * 3),
        written_stream("mono 16 b", 21, 1, 16, [100] * 11),
        written_stream("3ch 8", 22, 3, 8, [256] * 2 + [18]),
        written_stream("stereo 12", 23, 2, 12, [192] * 4),
        written_stream("mono 20", 24, 1, 20, [576, 576, 20]),
    ]
    return out


def offsets_of(s):
    """Start of every frame the stream was written from, and the end."""
    return np.concatenate([[0], np.cumsum([b for b, _ in s.frame_sizes])]).astype(np.int64)


# ---------------------------------------------------------------- stops
def flip(s, name, at):
    bad = s.data.copy()
    bad[at] ^= 0x10
    return s.but(name, bad)


@functools.lru_cache(None)
def stops():
    """name -> (stream, the frames the damage leaves, the stop reason): each decodes up to the damage."""
    base = written_stream("stop base", 31, 2, 16, [192] * 7 + [60])
    off = offsets_of(base)
    k = 3
    out = {
        "crc16 flipped": (flip(base, "crc16 flipped", off[k + 1] - 1), k, _capi.DECODE_CHAIN),
        "crc8 flipped": (flip(base, "crc8 flipped", off[k] + 2), k, _capi.DECODE_CHAIN),
        "cut in last frame": (base.but("cut", base.data[:off[-1] - 9]), len(off) - 2, _capi.DECODE_CHAIN),
        "leading garbage": (base.but("garbage first", np.concatenate(
            [np.random.default_rng(5).integers(0, 256, 300).astype(np.uint8), base.data])), 0, _capi.DECODE_CHAIN),
    }
    big = written_stream("block above max", 32, 1, 16, [128, 128, 256, 128], mbs=128)
    out["block above max"] = (big, 2, _capi.DECODE_UNSUPPORTED)
    return out, base


def garbage(n=32, size=600):
    """Random bytes, and bytes dense with sync codes whose headers often pass the CRC-8 by construction."""
    rng = np.random.default_rng(0x6A2BA6E)
    out = []
    for i in range(n):
        channels, bps = (1, 2, 3, 8)[i % 4], (8, 16, 24)[i % 3]
        raw = rng.integers(0, 256, size + i).astype(np.uint8)
        if i % 2:
            for at in range(0, len(raw) - 8, 7 + i % 5):
                hdr = fw.header((16, 192, 256, 4096)[at % 4], (0 if channels == 1 else channels - 1), bps, at % 100)
                raw[at:at + len(hdr)] = np.frombuffer(hdr, np.uint8)[:len(raw) - at]
        out.append(Stream("garbage %d" % i, raw, channels, bps, 4096))
    return out


# ---------------------------------------------------------------- a batch
class Batch:
    """streams laid into one byte buffer (`gaps[i]` bytes of GAP in front of stream i, `lead` first) and slots laid into
    one output buffer in shuffled order with `spacing` bytes of FILL around them."""

    def __init__(self, streams, capacities=None, gaps=None, spacing=24, seed=1, tail=40):
        """gaps: per stream the number of GAP bytes in front of it, or the bytes themselves (a uint8 array)."""
        self.streams = list(streams)
        n = len(self.streams)
        gaps = gaps if gaps is not None else [(0, 5, 0, 33, 1)[i % 5] for i in range(n)]
        parts, self.offsets = [], []
        at = 0
        for s, g in zip(self.streams, gaps):
            g = np.full(g, GAP, np.uint8) if isinstance(g, (int, np.integer)) else np.asarray(g, np.uint8)
            parts.append(g)
            at += len(g)
            self.offsets.append(at)
            parts.append(s.data)
            at += len(s.data)
        parts.append(np.full(tail, GAP, np.uint8))
        self.data = np.concatenate(parts) if parts else np.zeros(0, np.uint8)
        caps = capacities or [None] * n
        self.capacities = [len(s.pcm) if (c is None and s.pcm is not None) else (c if c is not None else 4096)
                           for s, c in zip(self.streams, caps)]
        order = np.random.default_rng(seed).permutation(n)
        self.out_offsets = [0] * n
        at = spacing
        for i in order:
            self.out_offsets[i] = at
            at += self.capacities[i] + spacing
        self.out_bytes = at
        self.table = np.zeros(n, _capi.STREAM_DESC_DTYPE)
        for i, s in enumerate(self.streams):
            self.table[i] = (self.offsets[i], len(s.data), self.out_offsets[i], self.capacities[i], s.channels, s.bps,
                             s.mbs, s.width)

    def fresh_out(self):
        return np.full(max(1, self.out_bytes), FILL, np.uint8)

    def slot(self, out, i):
        return out[self.out_offsets[i]:self.out_offsets[i] + self.capacities[i]]

    def outside_slots_untouched(self, out, written):
        """Everything but the first written[i] bytes of every slot is still FILL."""
        mask = np.ones(len(out), bool)
        for i, w in enumerate(written):
            mask[self.out_offsets[i]:self.out_offsets[i] + w] = False
        return bool((out[mask] == FILL).all())

    def max_frames(self):
        return sum(len(s.data) // 9 + 1 for s in self.streams)
