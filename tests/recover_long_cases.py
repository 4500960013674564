"""Batches that take flacenc_hip_recover_streams and the shared batch index (stream_index.cpp) past the fixed sizes
they rest on: 256 frames per workgroup of the segmented max-scan, 256 / channels frames per workgroup of the decode
kernel, 1024 elements per round of the one-workgroup scans (over streams and over chain frames), one jump level per bit
of a frame's index in its chain, and PIECE = 4096 bytes per workgroup of the zero pass.  tests/recover_cases.py stays
below all of them.

Frames are small -- mono, 8 bits, 16 samples, about 11 bytes -- and come out of one pool numbered 0..2999, so that to
lose, repeat or jump is a list operation.  Slot order is channel count ascending, then table order (sort_by_channels is
a stable counting sort): a mono-only batch's frame sequence is its table order, and a stream's head lies at the sum of
the chain frames of the streams in front of it.  No GPU is needed to build any of it: tests/test_recover_long_cpu.py
proves these claims on the model, tests/test_gpu_recover_long.py takes the batches to the device."""
import functools

import numpy as np

import recover_cases as rc
import recover_model as model
import streams_cases as cases

Batch = cases.Batch
BLOCK = 16
POOL = 3000
HEADS = (255, 256, 257, 511, 512, 513, 1023, 1024, 1025)   # sequence positions `seams` puts a stream's head on
SPIKE_HEAD = 1728   # 6 * 256 + 192: its dropped run starts 58 elements in front of a workgroup's first


@functools.lru_cache(None)
def pool():
    """Mono 8-bit frames of 16 samples with the coded numbers 0..2999: Constant, Fixed and Verbatim subframes."""
    return rc.build(200, 1, 8, [BLOCK] * POOL, kinds=[4, 0, 2, 0])


def stream(name, numbers):
    """The pool's frames of these numbers, in this order."""
    p = pool()
    return p.stream(name, [p.frames[k] for k in numbers])


class InOrder(Batch):
    """A Batch whose slots lie in table order, `spacing` bytes apart (a Batch shuffles them)."""

    def __init__(self, streams, capacities, spacing, **kw):
        super().__init__(streams, capacities=capacities, spacing=spacing, **kw)
        at = spacing
        for i in range(len(self.streams)):
            self.out_offsets[i] = at
            self.table[i]["out_offset"] = at
            at += self.capacities[i] + spacing
        assert at == self.out_bytes


# ---------------------------------------------------------------- the streams
def spike_numbers():
    """800 frames with the frame numbered 700 inserted behind the first five: it is placed, and everything up to its
    second appearance -- 696 chain frames -- is dropped against the one maximum it set."""
    n = list(range(800))
    n.insert(5, 700)
    return n


def gap_numbers():
    """Frames 0..2, then 700..1399: one gap of 697 blocks, 703 chain frames."""
    return [0, 1, 2] + list(range(700, 1400))


def restart_numbers():
    """600 frames, then 300..899 again: 300 dropped in one run, 300 placed behind them."""
    return list(range(600)) + list(range(300, 900))


def worn_numbers(n=1150, every=37):
    """Frames 0..n-1 with, in turn at about every 37th, a frame lost, a frame repeated and an old frame again."""
    out = []
    for k in range(n):
        what = (k // every) % 3 if k % every == every - 1 else -1
        if what == 0:
            continue
        out.append(k)
        if what == 1:
            out.append(k)
        if what == 2:
            out.append(k - 9)
    return out


SPIKE_WANT = ([105, 12800, 11120, 696, 0, 0, 0, 0], [(80, 11120)])   # totals and gaps of the spike stream, roomy slot


@functools.lru_cache(None)
def seams_batch():
    """-> (Batch, origins, names).  Mono, origin 0, roomy slots.  Heads on every position of HEADS; the gap stream from
    1025 on; the spike at SPIKE_HEAD; then the long restart, the worn stream and an undamaged stream of 1100 frames.
    The streams in front of position 1024 have gaps of their own (a frame lost)."""
    def lost(n, *gone):
        return [k for k in range(n) if k not in gone]

    items = [("lead 255", list(range(255))), ("one at 255", [0]), ("one at 256", [0]),
             ("254 from 257", lost(255, 100)), ("one at 511", [3]), ("one at 512", [0]),
             ("510 from 513", lost(512, 7, 300)), ("one at 1023", [0]), ("one at 1024", [2]),
             ("gap", gap_numbers()), ("spike", spike_numbers()), ("restart", restart_numbers()),
             ("worn", worn_numbers()), ("undamaged", list(range(1100)))]
    streams = [stream(name, numbers) for name, numbers in items]
    caps = [BLOCK * POOL + 64] * len(streams)
    return Batch(streams, capacities=caps, spacing=17, seed=11), [0] * len(streams), [n for n, _ in items]


def chain_end(numbers, index):
    """The end, in samples from 0, of the pool frame at chain index `index` of a stream of these numbers."""
    return (numbers[index] + 1) * BLOCK


PLATEAU = 701 * BLOCK   # the spike's end: the prefix maximum of its 696 dropped frames


def cut_capacities(what):
    """The slots of cuts_batch(what), in bytes = samples (W = 1).  The spike stream: the plateau exactly, one byte short
    of it and one byte past it; the would-be end of the last frame it drops in front of frame 700's second appearance;
    the end of the dropped frame at chain index 256, far under the plateau; the last frame's end and one sample either
    way.  The gap stream: the ends of the placed frames at chain index 255, 256, 257 and the last, each exactly and one
    sample either way."""
    if what == "spike":
        sp = spike_numbers()
        return [PLATEAU, PLATEAU - 1, PLATEAU + 1, 700 * BLOCK, chain_end(sp, 256)] + \
            [chain_end(sp, -1) + d for d in (-1, 0, 1)]
    gp = gap_numbers()
    return [chain_end(gp, k) + d for k in (255, 256, 257, -1) for d in (-1, 0, 1)]


@functools.lru_cache(None)
def cuts_batch(what):
    """-> (Batch, origins): the spike stream or the gap stream once per capacity of cut_capacities(what) -- one batch
    each, which keeps either under 10 000 chain frames."""
    caps = cut_capacities(what)
    s = stream(what, spike_numbers() if what == "spike" else gap_numbers())
    streams = [s.but("%s in %d" % (what, c)) for c in caps]
    return Batch(streams, capacities=caps, spacing=5, seed=12), [0] * len(streams)


MANY = 1200


def many_streams(damaged=True):
    """1200 streams of 0 to 2 frames.  Damaged: about every 4th starts at a number above 0 (a leading gap), some are junk
    only; undamaged: every stream starts at frame 0 and holds frames only.  Either way every 3rd is an empty span."""
    out = []
    for k in range(MANY):
        count = k % 3
        first = 1 + k % 5 if damaged and k % 4 == 1 else 0
        s = stream("many %d" % k, range(first, first + count))
        if damaged and k % 17 == 5:
            s = s.but("many %d junk" % k, np.frombuffer(rc.junk(k, 20 + k % 9), np.uint8))
        out.append(s)
    return out


@functools.lru_cache(None)
def many_batch():
    """-> (Batch, origins).  Slots of 8 blocks, some of capacity 0."""
    streams = many_streams()
    caps = [0 if k % 13 == 7 else 8 * BLOCK for k in range(MANY)]
    return Batch(streams, capacities=caps, spacing=3, seed=13), [0] * MANY


PIECE = 4096
EXACT_GAPS = (PIECE - 1, PIECE, PIECE + 1, 2 * PIECE)
WIDE_GAP = 1138   # samples of 9 bytes: 10 242 bytes, 2.5 pieces and 2 bytes


@functools.lru_cache(None)
def pieces_batch():
    """-> (InOrder batch, origins).  Slots in table order, 1 byte apart, every capacity a multiple of 16: slot k starts at
    k + 1 mod 16, so the gaps of the first 16 streams -- mono 8-bit, 2.5 pieces each (block 0, then block 641), closed
    by a last frame of one sample, so that the defined prefix is 1 mod 16 bytes and the packed staging of the
    host-memory form walks through the residues as well -- start on every residue mod 16, and with them every piece
    edge.  Then four mono streams with gaps of PIECE - 1, PIECE, PIECE + 1 and 2 * PIECE bytes and six 3-channel 24-bit
    streams (W = 9, variable blocking: the numbers count samples) with gaps of 2.5 pieces.  Only the frames that stay
    are written: the numbers are set."""
    streams, caps = [], []
    for k in range(16):
        b = rc.build(300 + k, 1, 8, [BLOCK, BLOCK, 1], mbs=BLOCK, numbers=[0, 641, 642], kinds=[2, 4, 0])
        streams.append(b.stream("pieces mono %d" % k))
        caps.append(642 * BLOCK + 1 + 15)
    for k, gap in enumerate(EXACT_GAPS):
        b = rc.build(320 + k, 1, 8, [BLOCK] * 3, variable=True, numbers=[0, BLOCK + gap, 2 * BLOCK + gap], kinds=[2, 0])
        streams.append(b.stream("pieces exact %d" % gap))
        caps.append((3 * BLOCK + gap + 15) // 16 * 16)
    for k in range(6):
        gap = WIDE_GAP + k
        b = rc.build(330 + k, 3, 24, [BLOCK] * 3, variable=True, numbers=[0, BLOCK + gap, 2 * BLOCK + gap])
        streams.append(b.stream("pieces 3ch %d" % k))
        caps.append(((3 * BLOCK + gap) * 9 + 15) // 16 * 16)
    return InOrder(streams, caps, 1), [0] * len(streams)


@functools.lru_cache(None)
def wide_batch():
    """-> (Batch, origins).  One 3-channel stream of more than 200 chain frames and one 8-channel stream of more than 70
    -- three decode workgroups of 256 / 8 = 32 frames -- with every 5th frame repeated (dropped: idle lanes between live
    ones) and every 7th lost, as recover_cases.crowd_batch does for stereo."""
    streams, caps = [], []
    for seed, channels, bps, n in ((340, 3, 24, 220), (341, 8, 16, 80)):
        b = rc.build(seed, channels, bps, [BLOCK] * n)
        frames = []
        for j, x in enumerate(b.frames):
            if j % 7 == 3:
                continue
            frames.append(x)
            if j % 5 == 1:
                frames.append(x)
        streams.append(b.stream("wide %dch" % channels, frames))
        caps.append(n * BLOCK * channels * b.width + 32)
    return Batch(streams, capacities=caps, spacing=7, seed=14), [0, 0]


@functools.lru_cache(None)
def undamaged_batch():
    """-> Batch.  An undamaged stream of 1100 frames -- a chain that takes jump level 10 -- in front of and behind the
    undamaged form of `many`: more than 1024 streams and more than 1024 chain frames either side of the scans' seam."""
    long = stream("undamaged", range(1100))
    streams = [long] + many_streams(damaged=False) + [long.but("undamaged again")]
    caps = [1100 * BLOCK] + [2 * BLOCK + 3] * MANY + [1100 * BLOCK]
    return Batch(streams, capacities=caps, spacing=2, seed=15)


def all_batches():
    return {"seams": seams_batch()[:2], "cuts spike": cuts_batch("spike"), "cuts gap": cuts_batch("gap"),
            "many": many_batch(), "pieces": pieces_batch(), "wide": wide_batch()}


NAMES = ("seams", "cuts spike", "cuts gap", "many", "pieces", "wide")


@functools.lru_cache(None)
def wanted(name):
    batch, origins = all_batches()[name]
    return model.expected_batch(batch, origins)


def many_max_gaps():
    """The gap-table sizes `many` runs with: all of its gaps, all but one, and fewer than streams 0..1023 have."""
    want = wanted("many")
    return len(model.gap_records(want)), len(model.gap_records(want)) - 1, len(model.gap_records(want[:1024])) - 7
