"""flacenc_hip_recover_streams without a GPU: the model the GPU tests compare against (tests/recover_model.py) on
hand-counted cases, and the corpus' own claims (tests/recover_cases.py) -- every damage does what its name says."""
import re
import os

import numpy as np

import flac_write as fw
import recover_cases as rc
import recover_model as model
import streams_cases as cases
from flacenc_rs_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(s, origin=0, capacity=1 << 20):
    return model.expected(s.data, s.channels, s.bps, s.mbs, s.width, capacity, origin)


def test_three_frames_with_the_middle_crc_broken():
    bs = 32
    b = rc.build(1, 2, 16, [bs] * 3)
    good = run(b.stream("good"))
    assert good[1] == [3, 3 * bs, 0, 0, 0, 0, 0, 0] and good[2] == []
    f = b.frames
    s = b.stream("middle", [f[0], rc.flipped(f[1], len(f[1]) - 1), f[2]])
    slot, totals, gaps = run(s)
    # two frames, L = 3 blocks, one block of silence, nothing dropped, the middle frame's bytes in no frame; the chain
    # breaks ONCE: frame 2 does not start where frame 0 ended (the chain ends at the span's end)
    assert totals == [2, 3 * bs, bs, 0, len(f[1]), 1, 0, 0]
    assert gaps == [(bs, bs)]
    W = 4
    assert np.array_equal(slot[:bs * W], good[0][:bs * W]) and np.array_equal(slot[2 * bs * W:], good[0][2 * bs * W:])
    assert not slot[bs * W:2 * bs * W].any()
    # the last frame broken instead: the break is the tail, and nothing behind the last good frame is defined
    s = b.stream("last", [f[0], f[1], rc.flipped(f[2], len(f[2]) - 1)])
    assert run(s)[1:] == ([2, 2 * bs, 0, 0, len(f[2]), 1, 0, 0], [])
    # the first frame broken: a break in front, silence in front
    s = b.stream("first", [rc.flipped(f[0], len(f[0]) - 1), f[1], f[2]])
    assert run(s)[1:] == ([2, 3 * bs, bs, 0, len(f[0]), 1, 0, 0], [(0, bs)])


def test_hand_counted_drops_room_and_origins():
    bs = 16
    b = rc.build(2, 1, 16, [bs] * 5)
    f = b.frames
    W = 2
    # a repeated frame is dropped and breaks nothing
    assert run(b.stream("rep", f[:2] + [f[1]] + f[2:]))[1] == [5, 5 * bs, 0, 1, 0, 0, 0, 0]
    # swapped: 0 1 3 2 4 -> frame 2 comes behind frame 3's end and is dropped; its place is silence
    slot, totals, gaps = run(b.stream("swap", [f[0], f[1], f[3], f[2], f[4]]))
    assert totals == [4, 5 * bs, bs, 1, 0, 0, 0, 0] and gaps == [(2 * bs, bs)]
    # room: exactly three frames fit; one byte less and only two do
    assert run(b.stream("room"), capacity=3 * bs * W)[1] == [3, 3 * bs, 0, 0, 0, 0, _capi.DECODE_NO_ROOM, 0]
    assert run(b.stream("room"), capacity=3 * bs * W - 1)[1] == [2, 2 * bs, 0, 0, 0, 0, _capi.DECODE_NO_ROOM, 0]
    assert run(b.stream("room"), capacity=0)[1] == [0, 0, 0, 0, 0, 0, _capi.DECODE_NO_ROOM, 0]
    # an origin at frame 2: frames 0 and 1 lie before it
    slot, totals, gaps = run(b.stream("origin"), origin=2 * bs)
    assert totals == [3, 3 * bs, 0, 2, 0, 0, 0, 0] and np.array_equal(slot, run(b.stream("x"))[0][2 * bs * W:])
    # garbage and nothing
    assert run(b.stream("junk", data=rc.junk(1, 77)))[1:] == ([0, 0, 0, 0, 77, 1, 0, 0], [])
    assert run(b.stream("empty", data=b""))[1:] == ([0] * 8, [])
    # a block above the maximum is dropped, its samples are silence
    big = rc.build(3, 1, 16, [16, 32, 16], mbs=16)   # numbers 0, 1, 2: frame 1 claims samples 16..48 and is too large
    assert run(big.stream("big"))[1] == [1, 16, 0, 2, 0, 0, 0, 0]   # frame 2 at 32 lies inside the dropped frame's end


def test_the_planted_frame_is_a_frame_only_when_its_host_is_broken():
    items = rc.damage_streams()
    pl, host, at = rc.planted()
    off = pl.offsets()
    alive = items["planted, host alive"][0]
    positions = [c.pos for c in model.verified(alive.data, 1, 8)]
    assert int(off[host]) + at in positions                       # it IS a verified candidate
    assert [c.pos for c in model.chain(model.verified(alive.data, 1, 8))] == [int(v) for v in off[:-1]]
    assert run(alive)[1] == [5, 5 * 64, 0, 0, 0, 0, 0, 0]
    broken = items["planted, host broken"][0]
    chain = [c.pos for c in model.chain(model.verified(broken.data, 1, 8))]
    assert int(off[host]) + at in chain and int(off[host]) not in chain
    # number 9 of blocks of 64: it lands far behind, and frames 3 and 4 are then dropped as descending
    assert run(broken)[1][:4] == [3, 9 * 64 + 16, 9 * 64 + 16 - 2 * 64 - 16, 2]


def test_every_damage_does_what_its_name_says():
    items = rc.damage_streams()
    t = {name: run(s, origin)[1] for name, (s, origin) in items.items()}
    g = {name: run(s, origin)[2] for name, (s, origin) in items.items()}
    for name in items:
        if name.startswith("undamaged"):
            assert t[name][2:] == [0] * 6 and t[name][0] >= 3, name
    assert {items[n][0].channels for n in items if n.startswith("undamaged")} == {1, 2, 3, 8}
    for name in ("body bit", "header bit", "crc16 bit", "crc8 bit", "frame removed"):
        assert t[name][2] > 0 and t[name][3] == 0 and len(g[name]) == 1, name
    assert t["frame removed"][4:6] == [0, 0]                       # no byte lost, no break: only the numbers tell
    for n in (1, 7, 300):
        assert t["garbage %d" % n] == [5, 5 * 16, 0, 0, n, 1, 0, 0]
    assert t["leading garbage"][:6] == [6, 6 * 96, 0, 0, 33, 1]
    assert t["cut in last frame"][0] == 7 and t["cut in last frame"][5] == 1
    assert t["garbage only"] == [0, 0, 0, 0, 500, 1, 0, 0]
    assert t["first frame"][:2] == [5, 6 * 32] and g["first frame"] == [(0, 32)]
    assert g["two neighbours"] == [(3 * 17, 2 * 17)] and t["two neighbours"][5] == 1   # one gap, not two
    assert t["frame repeated"][:4] == [8, 8 * 48, 0, 1] and t["two swapped"][:4] == [7, 8 * 48, 48, 1]
    assert t["numbers restart"][:4] == [5, 5 * 48, 0, 4]
    assert t["block above max"][3] >= 1
    sizes = sorted(len(fw.utf8_number(o)) for n, (s, o) in items.items() if n.startswith("variable"))
    assert sizes == [5, 6, 7, 7]
    for n in items:
        if n.startswith("variable"):
            assert t[n][0] >= 5 and t[n][3] == 0, n
    assert t["origin at a frame"][:4] == [7, 8 * 48, 48, 0]
    assert t["a frame before the origin"][:4] == [6, 6 * 48, 0, 2]
    assert t["origin inside a frame"][:4] == [6, 7 * 48 - 7, 48 - 7, 2] and g["origin inside a frame"] == [(0, 41)]
    assert [n for _, n in g["gaps under 16 bytes"]] == [3, 11, 15, 89] and t["gaps under 16 bytes"][0] == 5
    assert g["gap of several KiB"] == [(192, 3 * 192)] and 3 * 192 * 24 > 8192
    assert t["several damages"][3] >= 2 and len(g["several damages"]) >= 2 and t["several damages"][5] >= 3
    assert t["span of 0 bytes"] == [0] * 8
    assert t["undamaged oracle writer"] == [6, 6 * 192, 0, 0, 0, 0, 0, 0]
    assert t["oracle writer, body bit"][:4] == [5, 6 * 192, 192, 0] and g["oracle writer, body bit"] == [(3 * 192, 192)]


def test_the_batches_reach_the_shapes_they_are_there_for():
    batch, origins = rc.room_batch()
    want = model.expected_batch(batch, origins)
    assert {t[6] for _, t, _ in want} == {0, _capi.DECODE_NO_ROOM}
    assert sorted({t[0] for _, t, _ in want}) == [0, 1, 2, 3, 4, 5, 6]
    # odd slots: the gaps' first and last+1 addresses cover 1..15 mod 16 (the buffer itself is 16-byte aligned)
    batch, origins = rc.odd_batch()
    lo, hi = set(), set()
    for i, (_, _, gaps) in enumerate(model.expected_batch(batch, origins)):
        W = batch.streams[i].channels * batch.streams[i].width
        for a, n in gaps:
            lo.add((batch.out_offsets[i] + a * W) % 16)
            hi.add((batch.out_offsets[i] + (a + n) * W) % 16)
    assert lo >= set(range(1, 16)) and hi >= set(range(1, 16)), (sorted(lo), sorted(hi))
    assert any(o % 2 for o in batch.out_offsets)
    batch, origins = rc.crowd_batch()
    want = model.expected_batch(batch, origins)
    stereo = [i for i, s in enumerate(batch.streams) if s.channels == 2]
    chain_frames = sum(want[i][1][0] + want[i][1][3] for i in stereo)
    assert chain_frames > 128 and all(want[i][1][3] > 0 and want[i][1][2] > 0 for i in stereo)
    batch, origins = rc.garbage_batch()
    assert any(t[0] == 0 and t[4] == len(s.data) for (_, t, _), s in zip(model.expected_batch(batch, origins),
                                                                           batch.streams))


def test_undamaged_streams_agree_with_the_stopping_model():
    """The consequence: where the verified chain from byte 0 covers the stream and the numbers run from the origin, both
    models give the same bytes."""
    import streams_model
    for s in cases.mixed():
        pcm, totals = streams_model.expected(s.data, s.channels, s.bps, s.mbs, s.width, len(s.pcm))
        if any(n != s.mbs for _, n in s.frame_sizes[:-1]) and not s.name.startswith("variable"):
            continue   # fixed-blocking numbers with uneven blocks: not numbered consecutively in samples
        slot, t, gaps = run(s)
        assert np.array_equal(slot, pcm) and t == [totals[0], totals[1], 0, 0, 0, 0, 0, 0] and gaps == [], s.name


def test_header_bindings_and_library_agree_on_the_export():
    name = "flacenc_hip_recover_streams"
    header = open(os.path.join(ROOT, "include", "flacenc_hip.h")).read()
    assert re.search(r"\bint %s\s*\(" % name, header)
    assert name in _capi.EXPORTED_SYMBOLS and "flacenc_hip_debug_last_recover_plan" in _capi.DEBUG_SYMBOLS
    assert re.search(r"pub fn %s\(" % name, open(os.path.join(ROOT, "rust", "flacenc_hip.rs")).read())
