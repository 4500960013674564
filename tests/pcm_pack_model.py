"""A numpy model of flacenc_hip_pack_le_bytes (include/flacenc_hip.h) and the shapes its tests share
(tests/test_pcm_pack_cpu.py on the host build of csrc/pcm_pack_core.h, tests/test_gpu_pack_le_bytes.py and
tests/test_gpu_decode_pcm.py on the device).

The model is the contract restated: clamp the block sizes to the stride, concatenate every frame's first block_size samples
with the channels interleaved, and keep the low bytes_per_sample bytes of every two's-complement value, little-endian."""
import numpy as np

from oracle import oracle as orc

BYTES = (1, 2, 3, 4)
CHANNELS = (1, 2, 3, 8)
# every block size the issue names, empty frames next to full ones, odd sizes in front of the long frames so that their
# starts fall on every byte alignment
MIXED = (0, 1, 2, 3, 5, 16, 63, 64, 255, 256, 257, 4096, 1, 0, 3, 4096, 5)
SENTINEL = 0x5A5A5A5A   # in the rows beyond block_sizes[f]: must never reach the output


def pack_le_bytes(frames, block_sizes, bytes_per_sample):
    """rows int32 [n_frames, channels, stride] -> (bytes uint8, sample offsets uint64 [n_frames + 1], total)."""
    x = np.asarray(frames, np.int32)
    n, ch, stride = x.shape
    bs = np.minimum(np.asarray(block_sizes, np.uint64), stride).astype(np.int64)
    off = np.concatenate([[0], np.cumsum(bs)]).astype(np.uint64)
    parts = [x[f, :, :bs[f]].T for f in range(n) if bs[f]]
    inter = np.concatenate(parts) if parts else np.zeros((0, ch), np.int32)
    raw = np.ascontiguousarray(inter, "<i4").reshape(-1).view(np.uint8).reshape(-1, 4)[:, :bytes_per_sample]
    return np.ascontiguousarray(raw).reshape(-1), off, int(off[-1])


def fill_le_bytes(data, channels, bytes_per_sample, block_size):
    """The oracle's restatement of FrameBuf::fill_le_bytes (le_bytes_to_i32s + deinterleave, src/arrayutils.rs:248-290)
    for a stream of whole frames: bytes -> int32 [n_frames, channels, block_size]."""
    data = bytes(data)
    per = channels * bytes_per_sample * block_size
    assert len(data) % per == 0
    return np.stack([orc.deinterleave(orc.le_bytes_to_i32s(data[f * per:(f + 1) * per], bytes_per_sample), channels,
                                      block_size).reshape(channels, block_size)
                     for f in range(len(data) // per)]) if data else np.zeros((0, channels, block_size), np.int32)


def extremes(bytes_per_sample):
    """The ends of the width, -1, 0, 1 and values that do not fit it (their low bytes are kept)."""
    bits = 8 * bytes_per_sample
    lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
    fit = [lo, hi, -1, 0, 1, lo + 1, hi - 1]
    wide = [] if bytes_per_sample == 4 else [hi + 1, lo - 1, (1 << 31) - 1, -(1 << 31), 0x12345678, -0x12345678]
    return np.array(fit + wide, np.int64).astype(np.int32)


def rows(block_sizes, channels, stride, bytes_per_sample, seed):
    """Rows for a block-size list: random values of the width with the extremes sprinkled in, SENTINEL beyond each block."""
    rng = np.random.default_rng(seed)
    bits = 8 * bytes_per_sample
    n = len(block_sizes)
    x = rng.integers(-(1 << (bits - 1)), 1 << (bits - 1), (n, channels, stride), dtype=np.int64).astype(np.int32)
    ext = extremes(bytes_per_sample)
    where = rng.random(x.shape) < 0.05
    x[where] = ext[rng.integers(0, len(ext), int(where.sum()))]
    mask = (1 << bits) - 1
    x[(x.astype(np.int64) & mask) == (SENTINEL & mask)] = 0   # no sample of a block looks like the sentinel
    for f, b in enumerate(block_sizes):
        x[f, :, min(int(b), stride):] = SENTINEL
    return x


def holds_sentinel(out, bytes_per_sample, channels):
    """Whether a whole sample of `out` is the rows' sentinel (its low bytes): nothing behind a block size was packed."""
    samples = np.asarray(out, np.uint8).reshape(-1, bytes_per_sample)
    return bool((samples == 0x5A).all(axis=1).any())


def frame_start_alignments(block_sizes, channels, bytes_per_sample, stride):
    """The byte alignments (mod 4) of the frames' first bytes in an output that itself starts on a dword.  All four occur
    only where channels * bytes_per_sample is odd; the tests reach the rest by moving the output's first byte."""
    off = np.concatenate([[0], np.cumsum(np.minimum(np.asarray(block_sizes, np.int64), stride))])[:-1]
    return set(int(v) for v in (off * channels * bytes_per_sample) % 4)
