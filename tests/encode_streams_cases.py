"""The corpus of tests/test_gpu_encode_streams.py and tests/test_encode_streams_cpu.py: streams of PCM for
flacenc_hip_encode_streams, their layout in one `pcm` buffer (odd byte offsets, gaps) and their slots in one `out`
buffer (shuffled, a fill byte between and around them).

A Stream holds its samples as int32 [channels, total]; material comes from _capi.sigen_frames (tones + noise, with the
full-scale frames of stream_seam_cases.material) and from hand-made rows (a constant channel, silence, the width's two
ends)."""
import collections
import functools

import numpy as np

from flacenc_rs_amd import _capi

FILL = 0xC7          # what every byte of `out` holds before the call; bytes in no slot and behind a stream's bytes keep it
GAP = 0x5A           # the bytes of `pcm` in no span
Stream = collections.namedtuple("Stream", "name x channels bps width rate")


def material(total, channels, bps, seed):
    """int32 [channels, total]: tones + noise in blocks of 256; block 1 alternates between the width's two ends in
    channel 0, block 3 is uniform over the whole width in the last channel (the sign extension of every container)."""
    if total == 0:
        return np.zeros((channels, 0), np.int32)
    n = 256
    F = -(-total // n)
    x = _capi.sigen_frames(F, channels, n, bps, 57.0 + seed % 11, 0.35, 0.03, seed=7000 + seed, nthreads=2)
    lo, hi = -(1 << (bps - 1)), (1 << (bps - 1)) - 1
    if F > 1:
        x[1, 0, 0::2] = lo
        x[1, 0, 1::2] = hi
    if F > 3:
        x[3, channels - 1] = np.random.default_rng(seed).integers(lo, hi + 1, n)
    return np.ascontiguousarray(x.transpose(1, 0, 2).reshape(channels, F * n)[:, :total])


def stream(name, total, channels, bps, width, rate, seed):
    return Stream(name, material(total, channels, bps, seed), channels, bps, width, rate)


@functools.lru_cache(None)
def mixed(block):
    """The equivalence batch at one block size: mono, stereo and 3 channels; 16 bits in 2 bytes, 24 in 3, 16 in 4; rates
    44100, 48000 and 12345 (no code: two header bytes); lengths 0, exactly k blocks, block + 1, + 63, + 64,
    3 blocks + 1000, two pairs of streams with one tail length in one class, and hand-made rows."""
    b = block
    s = [
        stream("mono empty", 0, 1, 16, 2, 44100, 1),
        stream("mono 2 blocks", 2 * b, 1, 16, 2, 44100, 2),
        stream("stereo block+1", b + 1, 2, 16, 2, 44100, 3),
        stream("stereo block+63", b + 63, 2, 16, 2, 44100, 4),
        stream("stereo24 block+64", b + 64, 2, 24, 3, 48000, 5),
        stream("3ch 16in4 3 blocks+1000", 3 * b + 1000, 3, 16, 4, 12345, 6),
        stream("mono block+1000", b + 1000, 1, 16, 2, 44100, 7),
        stream("mono 2 blocks+1000", 2 * b + 1000, 1, 16, 2, 44100, 8),
        stream("stereo block+1 again", b + 1, 2, 16, 2, 44100, 9),
        stream("3ch24 1 block", b, 3, 24, 3, 48000, 10),
        stream("stereo tail only", 63, 2, 16, 2, 44100, 11),
    ]
    # hand-made rows: a constant channel next to silence next to the two ends of the width, one block and a tail of 5
    x = np.zeros((3, b + 5), np.int32)
    x[0] = -1234
    x[2, 0::2] = -(1 << 15)
    x[2, 1::2] = (1 << 15) - 1
    s.append(Stream("3ch hand-made", x, 3, 16, 4, 12345))
    return tuple(s)


def pack(x, width):
    """int32 [channels, total] -> interleaved little-endian bytes, `width` per sample."""
    flat = np.ascontiguousarray(x.T).reshape(-1).astype("<i4")
    return np.ascontiguousarray(flat.view(np.uint8).reshape(-1, 4)[:, :width]).reshape(-1)


def n_frames(s, block):
    return -(-s.x.shape[1] // block)


@functools.lru_cache(None)
def slot_bound(channels, block, bps):
    lib = _capi.load()
    return int(lib.flacenc_hip_stereo_frame_bytes_bound(block, bps) if channels == 2
               else lib.flacenc_hip_frame_bytes_bound(channels, block, bps))


Layout = collections.namedtuple("Layout", "pcm table out_bytes spans")


def layout(streams, block, capacities=None, seed=0, shuffle=True):
    """-> Layout: `pcm` uint8 with every stream's bytes at an odd offset and 1..9 gap bytes between spans (the last span
    ends at the buffer's last byte), the PCM_STREAM_DESC_DTYPE table, the size of `out` and the spans (offset, length).
    Slots are laid out in a shuffled order with 1..7 fill bytes in front of each; a slot's capacity is `capacities[i]`
    where given, else room for every frame at the bound."""
    rng = np.random.default_rng(1000 + seed)
    parts, spans, at = [], [], 0
    for s in streams:
        gap = int(rng.integers(1, 10))
        if (at + gap) % 2 == 0:
            gap += 1
        parts.append(np.full(gap, GAP, np.uint8))
        at += gap
        data = pack(s.x, s.width)
        spans.append((at, data.size))
        parts.append(data)
        at += data.size
    pcm = np.concatenate(parts) if parts else np.zeros(0, np.uint8)
    order = rng.permutation(len(streams)) if shuffle else np.arange(len(streams))
    table = np.zeros(len(streams), _capi.PCM_STREAM_DESC_DTYPE)
    out_at = 0
    for i in order:
        s = streams[i]
        cap = n_frames(s, block) * slot_bound(s.channels, block, s.bps) if capacities is None or capacities[i] is None \
            else capacities[i]
        out_at += int(rng.integers(1, 8))
        table[i] = (spans[i][0], s.x.shape[1], out_at, cap, s.channels, s.bps, s.width, s.rate)
        out_at += cap
    return Layout(pcm, table, out_at + 3, spans)


def slot_map(table, out_bytes):
    """bool [out_bytes]: True for the bytes of `out` that belong to a slot."""
    m = np.zeros(out_bytes, bool)
    for d in table:
        m[int(d["out_offset"]):int(d["out_offset"]) + int(d["out_capacity"])] = True
    return m
