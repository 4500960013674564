"""flacenc_hip_encode_streams_planar on the GPU, against its contract: out, frame_lengths, totals and call_totals are byte
for byte what flacenc_hip_encode_streams gives on the packed PCM P_s of the same samples (tests/planar_encode_model.py
states the samples: the elements, or q of them), digests are hashlib's MD5 of P_s, clip counts the model's.  Rows lie at
all four residues mod 16 with gaps between streams, tight and at a pitch; nothing outside the valid elements may matter;
whatever a call may not touch keeps its sentinel.  Every comparison is exact."""
import hashlib
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

import encode_streams_cases as cases
import encode_streams_model as model
import planar_encode_model as pem
from flacenc_rs_amd import _capi, crops

pytestmark = pytest.mark.gpu
FILL = cases.FILL
LEN_SENTINEL, TOTAL_SENTINEL, CLIP_SENTINEL = 0xA5A5A5A5, 0x5A5A5A5A5A5A5A5A, 0x7777777777777777
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I32, F32 = _capi.SAMPLE_I32, _capi.SAMPLE_F32
FLAGGED = _capi.FLAG_WASTED_BITS | _capi.FLAG_ORDER_GUESS


def lengths_of(block):
    """The issue's lengths; 2*block + 5, block + 5 and 5 share a tail length, as do 3*block + 1 and 1."""
    b = block
    return [0, 1, 3, 63, 64, 65, 2 * b - 1, 2 * b, 2 * b + 5, 3 * b + 1, b + 5, 5, 2 * b + 5]


def elements(total, channels, bits, fmt, seed):
    """[channels, total] int32 samples of the depth, or float32 elements: samples of the depth scaled as the decoder
    scales them, moved off the grid by less than half a step, with a few elements beyond full scale."""
    x = cases.material(total, channels, bits, seed)
    if fmt == I32:
        return x
    rng = np.random.default_rng(seed)
    f = (x.astype(np.float64) + rng.uniform(-0.49, 0.49, x.shape)) * 2.0 ** -(bits - 1)
    f = f.astype(np.float32)
    if total > 8:
        f[rng.integers(0, channels), rng.integers(0, total, 3)] = np.float32([1.5, -1.25, np.inf])
    return f


def samples_of(rows, bits, fmt):
    """-> (int32 samples, clip count) of one stream's elements."""
    if fmt == I32:
        return rows, 0
    v, clipped = pem.q(rows, bits)
    return v, int(clipped.sum())


def tables(rows, block, bits, width, rate, fmt, capacities=None, seed=0):
    """-> (descs for pem.layout, the packed buffer and table of the sibling call, per-stream packed PCM, clip counts)."""
    rng = np.random.default_rng(100 + seed)
    order = rng.permutation(len(rows))
    descs, out_at = [None] * len(rows), 0
    for i in order:
        c, n = rows[i].shape
        cap = -(-n // block) * cases.slot_bound(c, block, bits) if capacities is None or capacities[i] is None else capacities[i]
        out_at += int(rng.integers(1, 8))
        descs[i] = (out_at, cap, bits, width[i] if isinstance(width, (list, tuple)) else width, rate)
        out_at += cap
    packed, clips = [], []
    for r, d in zip(rows, descs):
        v, k = samples_of(r, bits, fmt)
        packed.append(pem.pack(v, d[3]))
        clips.append(k)
    at, parts = 0, []
    sib = np.zeros(len(rows), _capi.PCM_STREAM_DESC_DTYPE)
    for i, (r, d, p) in enumerate(zip(rows, descs, packed)):
        parts += [np.full(1, cases.GAP, np.uint8), p]
        sib[i] = (at + 1, r.shape[1], d[0], d[1], r.shape[0], d[2], d[3], d[4])
        at += 1 + p.size
    return descs, np.concatenate(parts), sib, packed, clips


def run_packed(h, pcm, table, out_bytes, cfg, block, kind="host"):
    """The sibling on the packed PCM, in the same memory kind (its plan is compared too)."""
    out = np.full(out_bytes, FILL, np.uint8)
    F = _capi.encode_streams_frames(table, block)
    lens = np.full(F + 8, LEN_SENTINEL, np.uint32)
    totals = np.full((len(table) + 2, 4), TOTAL_SENTINEL, np.uint64)
    if kind == "host":
        _, _, call, _ = h.encode_streams(pcm, table, cfg, block, out, frame_lengths=lens, totals=totals)
        return out, lens, totals, call
    import torch
    d_pcm, d_out = torch.from_numpy(pcm).cuda(), torch.from_numpy(out).cuda()
    d_lens, d_totals = torch.from_numpy(lens.view(np.int32)).cuda(), torch.from_numpy(totals.view(np.int64)).cuda()
    torch.cuda.synchronize()
    call, _ = h.encode_streams_device(d_pcm.data_ptr(), pcm.size, table, cfg, block, d_out.data_ptr(), out.size,
                                      d_lens.data_ptr(), F, d_totals.data_ptr())
    return d_out.cpu().numpy(), d_lens.cpu().numpy().view(np.uint32), d_totals.cpu().numpy().view(np.uint64), call


def run_planar(h, lay, fmt, cfg, block, kind, digests=True, clipped=True, check=True, samples_bytes=None, table=None,
               row_pitch=None, sample_format=None):
    """One call in host or device memory -> (out, lens, totals, call, digests, clipped, rc): whole buffers, sentinels in
    what the call does not own."""
    table = lay.table if table is None else table
    ns = len(table)
    F = _capi.encode_streams_frames(lay.table, block)
    out = np.full(lay.out_bytes, FILL, np.uint8)
    lens = np.full(F + 8, LEN_SENTINEL, np.uint32)
    totals = np.full((ns + 2, 4), TOTAL_SENTINEL, np.uint64)
    pitch = lay.row_pitch if row_pitch is None else row_pitch
    sfmt = fmt if sample_format is None else sample_format
    nbytes = lay.samples.nbytes if samples_bytes is None else samples_bytes
    before = lay.samples.copy()
    if kind == "host":
        got = h.encode_streams_planar(lay.samples, sfmt, pitch, table, cfg, block, out, frame_lengths=lens, totals=totals,
                                      max_frames=F, digests=digests, clipped=clipped, samples_bytes=nbytes, check=check)
        _, _, call, dig, clip, rc = got
        dig = None if dig is None else np.array(dig, copy=True)
        clip = None if clip is None else np.array(clip, copy=True)
    else:
        import torch
        d_samples = torch.from_numpy(lay.samples.view(np.int32)).cuda()   # exactly the elements: the last one is the allocation's last
        d_out = torch.from_numpy(out).cuda()
        d_lens = torch.from_numpy(lens.view(np.int32)).cuda()
        d_totals = torch.from_numpy(totals.view(np.int64)).cuda()
        d_dig = torch.full((ns + 1, 16), 0x77, dtype=torch.uint8, device="cuda")
        d_clip = torch.from_numpy(np.full(ns + 1, CLIP_SENTINEL, np.uint64).view(np.int64)).cuda()
        torch.cuda.synchronize()
        call, rc = h.encode_streams_planar_device(d_samples.data_ptr(), nbytes, sfmt, pitch, table, cfg, block,
                                                  d_out.data_ptr(), out.size, d_lens.data_ptr(), F, d_totals.data_ptr(),
                                                  d_dig.data_ptr() if digests else 0, d_clip.data_ptr() if clipped else 0,
                                                  check=check)
        assert np.array_equal(d_samples.cpu().numpy(), before.view(np.int32)), "the input was written"
        out, lens = d_out.cpu().numpy(), d_lens.cpu().numpy().view(np.uint32)
        totals = d_totals.cpu().numpy().view(np.uint64)
        dig, clip = d_dig.cpu().numpy(), d_clip.cpu().numpy().view(np.uint64)
        assert (dig[ns:] == 0x77).all() and (clip[ns:] == CLIP_SENTINEL).all()
        if not digests:
            assert (dig == 0x77).all()
        if not clipped:
            assert (clip == CLIP_SENTINEL).all()
        dig, clip = (dig[:ns] if digests else None), (clip[:ns] if clipped else None)
    assert np.array_equal(lay.samples.view(np.uint32), before.view(np.uint32)), "the input was written"
    return out, lens, totals, call, dig, clip, rc


def same(a, b):
    """out, lens, totals, call of two runs: byte for byte, sentinels included."""
    for x, y, what in zip(a[:3], b[:3], ("out", "frame_lengths", "totals")):
        assert x.shape == y.shape and np.array_equal(x, y), what
    assert list(a[3]) == list(b[3]), "call_totals"


# channels x format crossed (every residue mod 16 occurs in every batch, tight rows and a pitch in every case); block
# size, depth, memory kind and flags along the diagonal
CASES = [(1, I32, 64, 8, "host", 0), (1, F32, 192, 16, "device", 0), (2, I32, 4096, 24, "device", 0),
         (2, F32, 64, 16, "host", 0), (3, I32, 192, 16, "host", 0), (3, F32, 4096, 24, "device", 0),
         (8, I32, 4096, 16, "host", 0), (8, F32, 64, 8, "device", 0),
         (1, I32, 4096, 16, "device", FLAGGED), (2, F32, 192, 16, "host", FLAGGED), (2, F32, 4096, 16, "device", 0),
         (1, F32, 64, 24, "host", 0)]


@pytest.mark.parametrize("channels,fmt,block,bits,kind,flags", CASES)
def test_a_batch_equals_encode_streams_on_its_packed_pcm(hooks_handle, channels, fmt, block, bits, kind, flags):
    h = hooks_handle
    cfg, _ = model.configs(8, flags=flags)
    lengths = lengths_of(block)
    rows = [elements(n, channels, bits, fmt, 31 * i + channels) for i, n in enumerate(lengths)]
    width, rate = (bits + 7) // 8, 44100
    descs, pcm, sib, packed, clips = tables(rows, block, bits, width, rate, fmt, seed=block + channels)
    dtype = np.int32 if fmt == I32 else np.float32
    want = None
    for pitch in (0, max(lengths) + 3):
        lay = pem.layout(rows, descs, pitch, dtype=dtype)
        assert {int(o) % 16 for o in lay.table["offset"]} == {0, 4, 8, 12}
        if want is None:
            want = run_packed(h, pcm, sib, lay.out_bytes, cfg, block, kind)
            packed_plan = h.debug_last_encode_streams_plan()
            assert (want[2][:len(rows), 3] == 0).all() and want[3][0] == sum(-(-n // block) for n in lengths)
        got = run_planar(h, lay, fmt, cfg, block, kind)
        same(got, want)
        plan = h.debug_last_encode_streams_planar_plan()
        assert plan["syncs"] == packed_plan["syncs"] <= 2 and plan["transfers"] == packed_plan["transfers"]
        assert plan["digest_launches"] == 2
        assert plan["launches"] == packed_plan["launches"] + 2 and plan["calls"] == packed_plan["calls"]
        for i, p in enumerate(packed):
            assert got[4][i].tobytes() == hashlib.md5(p.tobytes()).digest(), ("digest", i, lengths[i])
        assert [int(c) for c in got[5]] == clips
        assert (sum(clips) > 0) == (fmt == F32)


@pytest.mark.parametrize("channels", [1, 2])
def test_mono_and_stereo_equal_the_oracles_frames(hooks_handle, channels):
    """Not only a sibling: the frames are the oracle's controller and bit writer on the quantised samples."""
    h = hooks_handle
    block, bits = 192, 16
    cfg, mod = model.configs(8)
    lengths = [2 * block + 5, 63, block]
    rows = [elements(n, channels, bits, F32, 7 + i) for i, n in enumerate(lengths)]
    descs, _, _, _, _ = tables(rows, block, bits, 2, 44100, F32, seed=3)
    lay = pem.layout(rows, descs, 0, dtype=np.float32)
    out, lens, totals, call, _, _, _ = run_planar(h, lay, F32, cfg, block, "device")
    for i, r in enumerate(rows):
        s = cases.Stream("s%d" % i, pem.q(r, bits)[0], channels, bits, 2, 44100)
        want = b"".join(model.frames(mod, s, block))
        off = int(lay.table[i]["out_offset"])
        assert int(totals[i][1]) == len(want) and out[off:off + len(want)].tobytes() == want, i


@pytest.mark.parametrize("fmt,kind,channels", [(I32, "device", 2), (F32, "device", 3), (F32, "host", 1), (I32, "host", 8)])
def test_nothing_outside_the_valid_elements_matters(hooks_handle, fmt, kind, channels):
    h = hooks_handle
    block, bits = 64, 16
    cfg, _ = model.configs(8)
    lengths = [130, 0, 65, 7, 64, 3, 129]
    rows = [elements(n, channels, bits, fmt, 11 * i + 1) for i, n in enumerate(lengths)]
    descs, _, _, _, _ = tables(rows, block, bits, 2, 44100, fmt, seed=9)
    dtype = np.int32 if fmt == I32 else np.float32
    for pitch in (0, 133):
        runs = []
        for fill in (0, 0x7FFFFFFF, 0xFFC00001):     # zero; the largest int32 = a NaN; another NaN
            lay = pem.layout(rows, descs, pitch, fill=fill, dtype=dtype)
            assert lay.elements[-1] and (~lay.elements).sum() >= 4 * len(rows)   # the last valid element ends the buffer
            runs.append(run_planar(h, lay, fmt, cfg, block, kind))
        for r in runs[1:]:
            same(r, runs[0])
            assert np.array_equal(r[4], runs[0][4]) and np.array_equal(r[5], runs[0][5])


@pytest.mark.parametrize("channels,fmt", [(1, F32), (2, I32), (3, F32), (8, I32)])
def test_the_fill_kernels_other_load_form_gives_the_same_bytes(hooks_handle, channels, fmt):
    """Four dword loads per channel (the form DESIGN 4.23 measured and did not keep) against the aligned 16-byte loads
    brought into place: rows at every residue, lengths around the vector width and the frame's ends, pad elements NaN."""
    h = hooks_handle
    block, bits = 64, 16
    cfg, _ = model.configs(8)
    lengths = [130, 4, 65, 7, 64, 3, 129, 8, 9, 12, 200]
    rows = [elements(n, channels, bits, fmt, 13 * i + 2) for i, n in enumerate(lengths)]
    descs, _, _, _, _ = tables(rows, block, bits, 2, 44100, fmt, seed=4)
    dtype = np.int32 if fmt == I32 else np.float32
    for pitch in (0, 201, 203):
        lay = pem.layout(rows, descs, pitch, fill=0x7FFFFFFF, dtype=dtype)
        want = run_planar(h, lay, fmt, cfg, block, "device")
        h.debug_set_planar_fill_form(0)
        try:
            got = run_planar(h, lay, fmt, cfg, block, "device")
        finally:
            h.debug_set_planar_fill_form(1)
        same(got, want)
        assert np.array_equal(got[4], want[4]) and np.array_equal(got[5], want[5])


@pytest.mark.parametrize("bits,kind", [(8, "host"), (16, "device"), (24, "device"), (24, "host")])
def test_float_values_quantise_as_the_model_says(hooks_handle, bits, kind):
    h = hooks_handle
    block, width = 64, (bits + 7) // 8
    cfg, _ = model.configs(8)
    x = pem.float_cases(bits)
    rng = np.random.default_rng(bits)
    tame = (cases.material(2 * block + 9, 2, bits, 5).astype(np.float32) * np.float32(2.0 ** -(bits - 1)))
    rows = [np.stack([x, x[::-1]]), np.stack([rng.permutation(x)[:block + 1]]), tame,
            np.stack([rng.permutation(x), rng.permutation(x), rng.permutation(x)])]
    descs, _, _, packed, clips = tables(rows, block, bits, width, 48000, F32, seed=bits)
    assert clips[2] == 0 and min(clips[0], clips[1], clips[3]) > 0
    lay = pem.layout(rows, descs, 0, dtype=np.float32)
    out, lens, totals, call, dig, clip, _ = run_planar(h, lay, F32, cfg, block, kind)
    assert [int(c) for c in clip] == clips
    # the way back: what a decoder reads from the frames is q of the elements
    order = np.argsort(lay.table["out_offset"], kind="stable")
    stable = np.zeros(len(rows), _capi.STREAM_DESC_DTYPE)
    at = 0
    for k, i in enumerate(order):
        stable[k] = (int(lay.table[i]["out_offset"]), int(totals[i][1]), at, packed[i].size, rows[i].shape[0], bits, block, width)
        at += packed[i].size
    back = np.zeros(at, np.uint8)
    t, c, _ = h.decode_streams(out, stable, int(call[0]), back)
    assert (t[:len(rows), 3] == 0).all()
    for k, i in enumerate(order):
        o = int(stable[k]["out_offset"])
        assert np.array_equal(back[o:o + packed[i].size], packed[i]), i
        assert dig[i].tobytes() == hashlib.md5(packed[i].tobytes()).digest()
    # int32 input and in-range floats never count
    ints = [pem.q(r, bits)[0] for r in rows]
    ilay = pem.layout(ints, descs, 0)
    iout = run_planar(h, ilay, I32, cfg, block, kind)
    same(iout, (out, lens, totals, call))
    assert not iout[5].any() and np.array_equal(iout[4], dig)


@pytest.mark.parametrize("bits,dtype_name", [(16, "float32"), (24, "float32"), (16, "int32"), (24, "int32")])
def test_decode_crops_then_encode_crops_gives_the_frames_back(hooks_handle, bits, dtype_name):
    import torch
    h = hooks_handle
    block, channels, width = 192, 2, (bits + 7) // 8
    cfg, _ = model.configs(8)
    lengths = [3 * block + 17, block, 2 * block + 17, 40]
    streams = [cases.stream("rt%d" % i, n, channels, bits, width, 44100, 50 + i) for i, n in enumerate(lengths)]
    lay = cases.layout(streams, block, seed=bits, shuffle=False)
    out = np.full(lay.out_bytes, FILL, np.uint8)
    lens, totals, call, _ = h.encode_streams(lay.pcm, lay.table, cfg, block, out)
    stable = np.zeros(len(streams), _capi.STREAM_DESC_DTYPE)
    for i, s in enumerate(streams):
        stable[i] = (int(lay.table[i]["out_offset"]), int(totals[i][1]), 0, 0, channels, bits, block, width)
    T = max(lengths)
    dtype = getattr(torch, dtype_name)
    x, dt = crops.decode_crops(h, torch.from_numpy(out).cuda(), stable, [(i, 0) for i in range(len(streams))], T, dtype=dtype,
                               max_frames=int(call[0]))
    assert [int(v) for v in dt[:, 0].cpu()] == lengths
    r = crops.encode_crops(h, x, lengths, bits, 44100, cfg, block)
    assert r["frames"].is_cuda and r["items"].shape == (len(streams), 3) and not r["clipped"].any()
    frames, items = r["frames"].cpu().numpy(), r["items"].cpu().numpy()
    assert np.array_equal(r["frame_lengths"].cpu().numpy().view(np.uint32), lens)
    for i, s in enumerate(streams):
        o = int(lay.table[i]["out_offset"])
        want = out[o:o + int(totals[i][1])]
        assert [int(v) for v in items[i, 1:]] == [int(totals[i][1]), int(totals[i][0])]
        assert np.array_equal(frames[int(items[i, 0]):int(items[i, 0]) + len(want)], want), s.name
        assert r["digests"][i].cpu().numpy().tobytes() == hashlib.md5(cases.pack(s.x, width).tobytes()).digest()


@pytest.mark.parametrize("fmt,kind", [(F32, "device"), (I32, "host")])
def test_digests_containers_no_room_and_untouched_bytes(hooks_handle, fmt, kind):
    """bytes_per_sample 2 and 4 in one table (two classes), an empty stream, one slot a byte short of its second frame
    and one with no room: the digests are those of the whole input, everything else is the sibling's; without digests
    nothing else changes and two launches go."""
    h = hooks_handle
    block, bits, channels = 192, 16, 2
    cfg, _ = model.configs(8)
    lengths = [2 * block + 5, 0, 3 * block, block + 5, 65, 2 * block]
    widths = [2, 4, 2, 4, 2, 4]
    rows = [elements(n, channels, bits, fmt, 70 + i) for i, n in enumerate(lengths)]
    dtype = np.int32 if fmt == I32 else np.float32
    descs, pcm, sib, packed, clips = tables(rows, block, bits, widths, 44100, fmt, seed=1)
    full = run_packed(h, pcm, sib, pem.layout(rows, descs, 0, dtype=dtype).out_bytes, cfg, block)
    first = int(full[2][2][2])
    short = int(full[1][first]) + int(full[1][first + 1]) - 1        # stream 2: its second frame lacks a byte
    caps = [None, None, short, 0, None, None]
    descs, pcm, sib, packed, clips = tables(rows, block, bits, widths, 44100, fmt, capacities=caps, seed=1)
    lay = pem.layout(rows, descs, 200 * 3, dtype=dtype)
    want = run_packed(h, pcm, sib, lay.out_bytes, cfg, block, kind)
    packed_plan = h.debug_last_encode_streams_plan()
    assert [int(t[3]) for t in want[2][:6]] == [0, 0, _capi.ENCODE_NO_ROOM, _capi.ENCODE_NO_ROOM, 0, 0]
    assert [int(t[0]) for t in want[2][:6]] == [3, 0, 1, 0, 1, 2]
    got = run_planar(h, lay, fmt, cfg, block, kind)
    plan = h.debug_last_encode_streams_planar_plan()
    same(got, want)
    slots = cases.slot_map(lay.table, lay.out_bytes)
    assert (got[0][~slots] == FILL).all()
    for i, d in enumerate(lay.table):       # behind what totals says was written: untouched
        o, cap, used = int(d["out_offset"]), int(d["out_capacity"]), int(got[2][i][1])
        assert (got[0][o + used:o + cap] == FILL).all(), i
    for i, p in enumerate(packed):
        assert got[4][i].tobytes() == hashlib.md5(p.tobytes()).digest(), i
    assert got[4][1].tobytes() == hashlib.md5(b"").digest()
    assert [int(c) for c in got[5]] == clips
    bare = run_planar(h, lay, fmt, cfg, block, kind, digests=False)
    bare_plan = h.debug_last_encode_streams_planar_plan()
    same(bare, got)
    assert bare[4] is None and np.array_equal(bare[5], got[5])
    assert plan["digest_launches"] == 2 and bare_plan["digest_launches"] == 0
    assert bare_plan["launches"] == plan["launches"] - 2 == packed_plan["launches"]
    for k in ("syncs", "transfers", "classes", "full_runs", "tail_runs", "calls"):
        assert plan[k] == bare_plan[k] == packed_plan[k], k
    none = run_planar(h, lay, fmt, cfg, block, kind, digests=False, clipped=False)
    same(none, got)


@pytest.mark.parametrize("kind", ["host", "device"])
def test_each_new_bad_argument_writes_nothing(hooks_handle, kind):
    h = hooks_handle
    block, bits = 64, 16
    cfg, _ = model.configs(8)
    rows = [elements(n, 2, bits, I32, i) for i, n in enumerate([100, 64, 7])]
    descs, _, _, _, _ = tables(rows, block, bits, 2, 44100, I32)
    lay = pem.layout(rows, descs, 110)
    odd = lay.table.copy()
    odd["offset"][1] += 2
    beyond = lay.table.copy()
    beyond["offset"][2] += 4
    bad = [dict(table=odd), dict(sample_format=2), dict(row_pitch=99), dict(samples_bytes=lay.samples.nbytes - 4),
           dict(table=beyond), dict(samples_bytes=0)]
    for kw in bad:
        out, lens, totals, call, dig, clip, rc = run_planar(h, lay, I32, cfg, block, kind, check=False, **kw)
        assert rc == _capi.ERR_BAD_ARGUMENT, kw
        assert (out == FILL).all() and (lens == LEN_SENTINEL).all() and (totals == TOTAL_SENTINEL).all() and call == [0, 0]
        if kind == "device":
            assert (dig == 0x77).all() and (clip == CLIP_SENTINEL).all()
        else:
            assert not dig.any() and not clip.any()      # the binding's own zeros
    good = run_planar(h, lay, I32, cfg, block, kind)
    assert good[6] == _capi.OK and good[3][0] == 2 + 1 + 1


def test_the_plan_does_not_depend_on_the_number_of_streams(hooks_handle):
    h = hooks_handle
    block, bits = 64, 16
    cfg, _ = model.configs(8)
    plans = {}
    for n in (4, 64):
        lengths = [(2 * block + 5, block + 5, 3 * block + 1, 64)[i % 4] for i in range(n)]
        rows = [elements(m, 1, bits, F32, i) for i, m in enumerate(lengths)]
        descs, pcm, sib, _, _ = tables(rows, block, bits, 2, 44100, F32, seed=n)
        lay = pem.layout(rows, descs, 0, dtype=np.float32)
        want = run_packed(h, pcm, sib, lay.out_bytes, cfg, block)
        packed_plan = h.debug_last_encode_streams_plan()
        got = run_planar(h, lay, F32, cfg, block, "host")
        same(got, want)
        plans[n] = h.debug_last_encode_streams_planar_plan()
        assert plans[n]["launches"] == packed_plan["launches"] + 2 and plans[n]["syncs"] == 2
        assert plans[n]["transfers"] == packed_plan["transfers"]
    for k in ("launches", "syncs", "transfers", "classes", "tail_runs", "digest_launches"):
        assert plans[4][k] == plans[64][k], k


def test_encode_crops_and_the_tool_write_files_decode_flac_accepts(hooks_handle, tmp_path):
    import torch
    h = hooks_handle
    bits, rate, block, T = 16, 22050, 256, 700
    lengths = [700, 333, 64]
    x = np.zeros((3, 2, T), np.float32)
    for b, n in enumerate(lengths):
        x[b, :, :n] = elements(n, 2, bits, F32, 90 + b)
    x[:, :, 650:] += np.float32(9.0)     # behind items 1 and 2's lengths: must not matter; inside item 0: clips
    cfg = _capi.make_frame_config(_capi.make_config(lpc_order=8), use_fixed=True)
    want = [pem.q(x[b, :, :n], bits) for b, n in enumerate(lengths)]
    for dev in ("cuda", "cpu"):
        r = crops.encode_crops(h, torch.from_numpy(x).to(dev), lengths, bits, rate, cfg, block)
        assert r["frames"].device.type == dev
        assert [int(c) for c in r["clipped"].cpu()] == [int(w[1].sum()) for w in want]
        assert [int(v) for v in r["items"][:, 2].cpu()] == [3, 2, 1]
        for b, (v, _) in enumerate(want):
            assert r["digests"][b].cpu().numpy().tobytes() == hashlib.md5(pem.pack(v, 2).tobytes()).digest()
    assert crops.encode_crops(h, torch.from_numpy(x).cuda(), lengths, bits, rate, cfg, block, md5=False)["digests"] is None
    np.save(tmp_path / "x.npy", x)
    np.save(tmp_path / "n.npy", np.array(lengths))
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "encode_many.py"), "--npy", str(tmp_path / "x.npy"),
                        "--lengths", str(tmp_path / "n.npy"), "--bits", str(bits), "--rate", str(rate), "--block-size",
                        str(block), "--out-dir", str(tmp_path / "flacs")], capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0 and "3 files" in p.stdout, p.stdout[-2000:] + p.stderr[-2000:]
    spec = importlib.util.spec_from_file_location("decode_flac_tool", os.path.join(ROOT, "tools", "decode_flac.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    for b, (v, _) in enumerate(want):
        data = open(tmp_path / "flacs" / ("item%05d.flac" % b), "rb").read()
        pcm, info = tool.decode(data, h)
        assert info["total_samples"] == lengths[b] and info["channels"] == 2 and info["sample_rate"] == rate
        assert tool.md5_status(pcm, info) == "MD5 OK"
        assert np.array_equal(np.asarray(pcm), pem.pack(v, 2))
