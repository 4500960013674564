"""The corpus of the flacenc_hip_recover_streams tests: short streams written frame by frame with tests/flac_write.py
(and one by the oracle's writer, as tests/streams_cases.py has them), the damage applied to their bytes, and the batches
the tests lay them into.  No GPU is needed to build any of it: tests/test_recover_model_cpu.py proves the corpus' claims
on the model (tests/recover_model.py), tests/test_gpu_recover_streams.py takes the same batches to the device.

Blocks of 16 to 192 samples and 3 to 40 frames per stream keep every test at a few seconds."""
import functools

import numpy as np

import flac_write as fw
import streams_cases as cases
from oracle import oracle as orc

Stream, Batch = cases.Stream, cases.Batch


class Built:
    """A stream as its frames: frames[f] the bytes of frame f, numbers[f] its coded number."""

    def __init__(self, channels, bps, mbs, width, variable, frames, blocks, numbers):
        self.channels, self.bps, self.mbs, self.width, self.variable = channels, bps, mbs, width, variable
        self.frames, self.blocks, self.numbers = list(frames), list(blocks), list(numbers)

    def stream(self, name, frames=None, mbs=None, data=None):
        data = b"".join(self.frames if frames is None else frames) if data is None else data
        return Stream(name, data, self.channels, self.bps, mbs or self.mbs, None, self.width)

    def offsets(self):
        return np.concatenate([[0], np.cumsum([len(f) for f in self.frames])]).astype(np.int64)

    def samples(self):
        return int(sum(self.blocks))


def build(seed, channels, bps, blocks, mbs=None, variable=False, start=0, numbers=None, width=None, kinds=None,
          tags=None):
    """Frame f has blocks[f] samples and the coded number numbers[f]: by default start + f under fixed blocking (start
    in frames), start + the samples in front of it under variable blocking (start in samples)."""
    rng = np.random.default_rng(seed)
    mbs = mbs or max(blocks)
    if numbers is None:
        numbers = [start + f for f in range(len(blocks))] if not variable else \
            [start + int(sum(blocks[:f])) for f in range(len(blocks))]
    frames = []
    for f, n in enumerate(blocks):
        tag = 0 if channels == 1 else channels - 1
        if channels == 2:
            tag = (tags or (1, 8, 9, 10))[f % len(tags or (1, 8, 9, 10))]
        xs, sfs = [], []
        for c in range(channels):
            which = kinds[(f + c) % len(kinds)] if kinds else seed + 3 * f + c
            x, sf = cases.subframe(rng, n, bps, which, tag >= 8)
            xs.append(x)
            sfs.append(sf)
        frames.append(fw.frame(np.stack(xs), tag, bps, sfs, number=numbers[f], variable=variable))
    return Built(channels, bps, mbs, width or (bps + 7) // 8, variable, frames, blocks, numbers)


def flipped(frame, at, bit=0x10):
    b = bytearray(frame)
    b[at] ^= bit
    return bytes(b)


def junk(seed, n):
    """Bytes that hold no sync code."""
    raw = np.random.default_rng(seed).integers(0, 255, n).astype(np.uint8)  # never 0xFF
    return raw.tobytes()


@functools.lru_cache(None)
def planted():
    """A mono 8-bit stream whose frame 2 is one Verbatim subframe that holds, byte-aligned, a complete valid frame of the
    same stream parameters (a Constant block of 16 samples with the coded number 9).  -> (Built, the host's index,
    the inner frame's offset inside the host)."""
    inner = fw.frame(np.full((1, 16), 5, np.int64), 0, 8, [dict(kind="constant")], number=9)
    b = build(71, 1, 8, [64] * 5, kinds=[0, 1, 3])
    x = np.random.default_rng(72).integers(-100, 100, 64).astype(np.int64)
    x[10:10 + len(inner)] = np.frombuffer(inner, np.int8)
    host = fw.frame(x[None], 0, 8, [dict(kind="verbatim")], number=2)
    at = host.find(inner)
    assert at > 0
    b.frames[2] = host
    return b, 2, at


def oracle_written(seed=70, frames=6, n=192):
    """A mono 16-bit stream whose frames the oracle's writer (Frame::write) wrote: Verbatim and Constant subframes,
    fixed blocking, numbers from 0."""
    rng = np.random.default_rng(seed)
    out = []
    for f in range(frames):
        if f % 3 == 2:
            sf = dict(kind=orc.KIND_CONSTANT, bps=16, dc_offset=int(rng.integers(-500, 500)))
        else:
            sf = dict(kind=orc.KIND_VERBATIM, bps=16, samples=cases.signal(rng, n, 16, "noise"))
        out.append(bytes(orc.write_frame(n, 0, 16, 44100, f, [sf])))
    return Built(1, 16, n, 2, False, out, [n] * frames, list(range(frames)))


def damage_streams():
    """name -> (Stream, origin): one damage per stream, a few with several, and undamaged streams of every channel
    count between them."""
    out = {}
    mono = build(41, 1, 16, [64] * 7 + [20], kinds=[0, 1, 3, 5, 7])            # every order bucket
    st = build(42, 2, 16, [48] * 8)                                             # every stereo channel code
    st24 = build(43, 2, 24, [96] * 6, width=4)
    three = build(44, 3, 24, [32] * 6)
    eight = build(45, 8, 16, [16] * 5)
    m8 = build(46, 1, 8, [17] * 9)
    for name, b in (("mono", mono), ("stereo", st), ("stereo 24 in 4", st24), ("3ch", three), ("8ch", eight),
                    ("mono 8", m8)):
        out["undamaged " + name] = (b.stream(name), 0)
    f = st.frames
    out["body bit"] = (st.stream("body bit", f[:3] + [flipped(f[3], len(f[3]) // 2)] + f[4:]), 0)
    out["header bit"] = (st.stream("header bit", f[:3] + [flipped(f[3], 2)] + f[4:]), 0)
    out["crc16 bit"] = (st.stream("crc16 bit", f[:3] + [flipped(f[3], len(f[3]) - 1)] + f[4:]), 0)
    out["crc8 bit"] = (mono.stream("crc8 bit", mono.frames[:2] + [flipped(mono.frames[2], 5, 1)] + mono.frames[3:]), 0)
    out["frame removed"] = (three.stream("frame removed", three.frames[:2] + three.frames[3:]), 0)
    for n in (1, 7, 300):
        out["garbage %d" % n] = (eight.stream("garbage %d" % n, eight.frames[:2] + [junk(n, n)] + eight.frames[2:]), 0)
    out["leading garbage"] = (st24.stream("leading garbage", [junk(5, 33)] + st24.frames), 0)
    whole = b"".join(mono.frames)
    out["cut in last frame"] = (mono.stream("cut", data=whole[:-7]), 0)
    out["garbage only"] = (mono.stream("garbage only", data=junk(6, 500)), 0)
    out["random only"] = (st.stream("random only", data=cases.garbage(2, 400)[1].data.tobytes()), 0)
    out["first frame"] = (three.stream("first frame", [flipped(three.frames[0], 9)] + three.frames[1:]), 0)
    g = m8.frames
    out["two neighbours"] = (m8.stream("two neighbours", g[:3] + [flipped(g[3], 7), flipped(g[4], 7)] + g[5:]), 0)
    out["frame repeated"] = (st.stream("frame repeated", f[:4] + [f[3]] + f[4:]), 0)
    out["two swapped"] = (st.stream("two swapped", f[:2] + [f[3], f[2]] + f[4:]), 0)
    again = build(47, 2, 16, [48] * 4)
    out["numbers restart"] = (st.stream("numbers restart", f[:5] + again.frames), 0)
    pl, host, at = planted()
    out["planted, host alive"] = (pl.stream("planted alive"), 0)
    broken = flipped(pl.frames[host], len(pl.frames[host]) - 1)
    out["planted, host broken"] = (pl.stream("planted broken", pl.frames[:host] + [broken] + pl.frames[host + 1:]), 0)
    big = build(48, 1, 16, [64, 64, 128, 64, 64], mbs=64)   # fixed-blocking numbers count blocks of 64
    out["block above max"] = (big.stream("block above max"), 0)
    for k, start in enumerate(((1 << 21) + 5, (1 << 26) + 77, (1 << 31) + 1, (1 << 35) + 123456)):
        v = build(50 + k, (1, 2, 3, 2)[k], 16, [64, 16, 100, 192, 33, 64], variable=True, start=start)
        lost = v.frames[:2] + v.frames[3:] if k % 2 else v.frames
        name = "variable %d (%d-byte numbers)" % (k, len(fw.utf8_number(start)))   # 5, 6, 7 and 7 bytes
        out[name] = (v.stream(name, lost), start)
    o = build(54, 2, 16, [48] * 8, start=1000)
    out["origin at a frame"] = (o.stream("origin", o.frames[:4] + o.frames[5:]), 1000 * 48)
    out["a frame before the origin"] = (o.stream("before origin"), 1002 * 48)
    out["origin inside a frame"] = (o.stream("inside"), 1001 * 48 + 7)
    short = build(55, 1, 8, [16, 20, 16, 30, 16], variable=True, numbers=[0, 16 + 3, 50, 66 + 15, 200])
    out["gaps under 16 bytes"] = (short.stream("short gaps"), 0)
    wide = build(56, 8, 24, [192] * 6)
    out["gap of several KiB"] = (wide.stream("KiB gap", wide.frames[:1] + wide.frames[4:]), 0)
    several = f[:1] + [flipped(f[1], 11), f[2], junk(8, 21), f[4], f[4], f[6], f[5], f[7][:-3]]
    out["several damages"] = (st.stream("several", several), 0)
    out["span of 0 bytes"] = (mono.stream("empty", data=b""), 0)
    ow = oracle_written()
    out["undamaged oracle writer"] = (ow.stream("oracle writer"), 0)
    out["oracle writer, body bit"] = (ow.stream("oracle writer hurt", ow.frames[:3] + [flipped(ow.frames[3], 40)]
                                                + ow.frames[4:]), 0)
    return out


@functools.lru_cache(None)
def damage_batch():
    """-> (Batch, origins, names): every stream of damage_streams in one batch, each slot large enough for its whole
    stream with room to spare -- and one slot of capacity 0."""
    items = damage_streams()
    names = list(items)
    streams = [items[n][0] for n in names] + [items["undamaged stereo"][0].but("capacity 0")]
    origins = [items[n][1] for n in names] + [0]
    caps = [4096 * s.channels * s.width // 2 for s in streams]
    caps[names.index("gap of several KiB")] = 6 * 192 * 24 + 64
    caps[-1] = 0
    return Batch(streams, capacities=caps, spacing=23, seed=3), origins, names + ["capacity 0"]


@functools.lru_cache(None)
def room_batch():
    """One damaged stream (a frame lost in the middle: a gap) in slots that end at every placed frame's end and one
    sample short of it."""
    b = build(61, 2, 16, [32] * 7)
    s = b.stream("room", b.frames[:2] + b.frames[3:])
    W, caps = 4, []
    for k in (1, 2, 4, 5, 6, 7):    # the ends of the placed frames, in blocks
        caps += [k * 32 * W, k * 32 * W - W, k * 32 * W + 3]
    return Batch([s.but("room %d" % c) for c in caps], capacities=caps, spacing=9, seed=4), [0] * len(caps)


@functools.lru_cache(None)
def odd_batch():
    """Slots at odd byte offsets whose gaps start and end on every address 1..15 mod 16 (the output buffer's first byte
    is 16-byte aligned on the device): mono 8-bit streams of 17-sample blocks (W = 1) and 3-channel 24-bit ones (W = 9)
    with different frames lost, in slots one after the other with 1 byte between them."""
    streams, caps = [], []
    for k in range(32):
        b = build(80 + k % 4, 1, 8, [17] * 8)
        lost = 1 + k % 5
        streams.append(b.stream("odd mono %d" % k, b.frames[:lost] + b.frames[lost + 1 + k % 2:]))
        caps.append(8 * 17 + k % 3)
    for k in range(6):
        b = build(95 + k, 3, 24, [16 + k] * 6)
        streams.append(b.stream("odd 3ch %d" % k, b.frames[:2] + b.frames[3:]))
        caps.append(6 * (16 + k) * 9 + 1)
    return Batch(streams, capacities=caps, spacing=1, seed=5), [0] * len(streams)


@functools.lru_cache(None)
def crowd_batch():
    """More than 128 stereo frames in one channel class -- chains cross workgroups -- with repeated (dropped) frames
    between live ones, so that waves mix idle and live lane pairs; a few mono streams make a second class."""
    streams = []
    for k in range(6):
        b = build(110 + k, 2, 16, [16 + 16 * (k % 3)] * 30)
        f = list(b.frames)
        frames = []
        for j, x in enumerate(f):
            if (j + k) % 7 == 3:
                continue                       # lost
            frames.append(x)
            if (j + k) % 5 == 1:
                frames.append(x)               # repeated: dropped
            if (j + k) % 11 == 6:
                frames.append(f[max(0, j - 2)])  # an old frame again: dropped
        streams.append(b.stream("crowd %d" % k, frames))
    for k in range(3):
        b = build(120 + k, 1, 16, [64] * 10, kinds=[7, 5, 3, 1])
        streams.append(b.stream("crowd mono %d" % k, b.frames[:4] + b.frames[5 + k:]))
    caps = [4096 * 4] * len(streams)
    return Batch(streams, capacities=caps, spacing=40, seed=6), [0] * len(streams)


@functools.lru_cache(None)
def garbage_batch():
    """Spans of random bytes, and of random bytes salted with real headers (tests/streams_cases.garbage)."""
    streams = cases.garbage(16, 500)
    return Batch(streams, capacities=[2048] * len(streams), spacing=8, seed=7), [0] * len(streams)


def all_batches():
    return {"damage": damage_batch()[:2], "room": room_batch(), "odd": odd_batch(), "crowd": crowd_batch(),
            "garbage": garbage_batch()}
