"""flacenc_hip_decode_streams on the GPU: batches of the corpus of tests/streams_cases.py (and of streams the project's own
encoders write) against the samples they were written from, against the model of tests/streams_model.py (the host build
of the decoder core + the numpy packer + the cut rule) and against flacenc_hip_decode_pcm on every stream alone -- bytes
and totals.  Slots lie in shuffled order with FILL between them, spans with gaps between them; whatever a call may not
touch must still be FILL.  Every comparison is exact."""
import numpy as np
import pytest

import streams_cases as cases
import streams_model as model
import stream_seam_cases as seams
from flacenc_rs_amd import _capi

pytestmark = pytest.mark.gpu
FILL, RATE = cases.FILL, 44100


def run(h, batch, in_kind="pageable", out_kind="pageable", max_frames=None):
    src = seams.buffer_of(in_kind, len(batch.data))
    src[:] = batch.data
    out = seams.buffer_of(out_kind, batch.out_bytes)
    out[:] = FILL
    totals, call, _ = h.decode_streams(src, batch.table, batch.max_frames() if max_frames is None else max_frames, out)
    return np.array(out, copy=True), totals, call


def check(h, batch, **kw):
    out, totals, call = run(h, batch, **kw)
    want = model.check_batch(batch, out, totals)
    assert call == [sum(t[0] for _, t in want), sum(t[1] for _, t in want)]
    return out, totals, want


def alone(h, s, capacity):
    """flacenc_hip_decode_pcm on the stream alone -> (bytes, totals)."""
    out = np.full(capacity + 16, FILL, np.uint8)
    got, totals = h.decode_pcm(s.data, s.channels, s.bps, s.mbs, bytes_per_sample=s.width, out=out, out_capacity=capacity)
    assert (out[len(got):] == FILL).all()
    return np.array(got, copy=True), totals


def encoded(h, name, channels, bps, n, full, tail, flags=0, shift=0):
    """`full` blocks of n samples + a last block of `tail` through flacenc_hip_encode_pcm."""
    width = (bps + 7) // 8
    x = seams.material(full + 1, channels, n, bps - shift, seed=len(name) + n) << shift
    pcm = seams.pack_pcm(x[:full], x[full][:, :tail] if tail else None, width)
    cfg = _capi.make_frame_config(_capi.make_config(lpc_order=8, flags=flags), use_fixed=True)
    data, lens = h.encode_pcm(pcm, channels, cfg, width, bps, n, RATE)
    return cases.Stream(name, np.array(data, copy=True), channels, bps, n, pcm, None, [(int(v), n) for v in lens])


def variable(h):
    import stream_cases
    S, levels, bps, n_sb = 1024, 3, 16, 4
    total = n_sb * S - 300
    x = stream_cases.changing(n_sb, 2, S, bps, 1)
    x[-1, :, total % S:] = 0
    v = h.encode_variable(x, bps, stream_cases.frame_cfg(8), levels, total_samples=total, sample_rate=RATE)
    assert not v["overflow"]
    pcm = seams.pack_pcm(x.transpose(1, 0, 2).reshape(2, -1)[:, :total][None], None, 2)
    return cases.Stream("encode_variable", np.frombuffer(v["data"], np.uint8), 2, bps, S, pcm)


@pytest.fixture(scope="module")
def everything(hooks_handle):
    h = hooks_handle
    return cases.mixed() + [encoded(h, "encoder 16 stereo", 2, 16, 1152, 6, 40),
                            encoded(h, "encoder 8 mono", 1, 8, 256, 9, 17),
                            encoded(h, "encoder 24 3ch", 3, 24, 576, 5, 100),
                            encoded(h, "encoder wasted", 2, 24, 576, 5, 33, flags=_capi.FLAG_WASTED_BITS, shift=8),
                            variable(h)]


def test_a_mixed_batch_equals_ground_truth_the_model_and_decode_pcm_alone(hooks_handle, everything):
    h = hooks_handle
    batch = cases.Batch(everything, seed=3)
    assert {s.channels for s in everything} == {1, 2, 3, 8}
    out, totals, _ = check(h, batch)
    for i, s in enumerate(everything):
        assert np.array_equal(batch.slot(out, i), s.pcm), s.name
        got, t = alone(h, s, len(s.pcm))
        assert np.array_equal(got, s.pcm) and t == [int(v) for v in totals[i]], s.name
    # a wider container for every stream: the same samples, sign-extended
    wide = [cases.Stream(s.name, s.data, s.channels, s.bps, s.mbs, None, 4) for s in everything[:8]]
    for w, s in zip(wide, everything):
        v = np.zeros((len(s.pcm) // s.width, 4), np.uint8)
        v[:, :s.width] = s.pcm.reshape(-1, s.width)
        v[:, s.width:] = np.where(v[:, s.width - 1:s.width] & 0x80, 0xFF, 0)
        w.pcm = v.reshape(-1)
    check(h, cases.Batch(wide, seed=4))


def test_boundaries_seams_gaps_and_starts(hooks_handle):
    h = hooks_handle
    m = cases.mixed()
    # a stream cut inside a frame, its two parts laid end to end as two streams; and two whole streams of the same
    # parameters end to end (one chain for a boundary-blind index)
    s = m[1]
    off = cases.offsets_of(s)
    cut = int(off[4]) + (int(off[5]) - int(off[4])) // 2
    parts = [s.but("first part", s.data[:cut]), s.but("second part", s.data[cut:]), m[0], m[20]]
    batch = cases.Batch(parts, capacities=[len(s.pcm), len(s.pcm), None, None], gaps=[0, 0, 0, 0])
    out, totals, want = check(h, batch)
    assert want[0][1] == [4, 4 * 192, int(off[4]), _capi.DECODE_CHAIN] and want[1][1] == [0, 0, 0, _capi.DECODE_CHAIN]
    assert want[2][1][3] == 0 and want[3][1][3] == 0 and np.array_equal(batch.slot(out, 3), m[20].pcm)
    # whole files back to back: the "metadata" in front of each stream holds planted headers and a copied frame
    files = [m[0], m[2], m[5], m[20]]
    gaps = []
    for f in files:
        planted = np.frombuffer(b"fLaC" + b"".join(cases.fw.header(256, 0 if f.channels == 1 else f.channels - 1, f.bps, k)
                                                   for k in range(5)), np.uint8)
        gaps.append(np.concatenate([planted, f.data[:f.frame_sizes[0][0]], np.full(3, 0xFF, np.uint8)]))
    check(h, cases.Batch(files, gaps=gaps))
    # stream starts at a lane's and a workgroup's first, last and second position
    for start in (15, 16, 17, 4095, 4096, 4097):
        check(h, cases.Batch([m[3], m[4], m[12]], gaps=[start, 1, 0]))


def test_lanes_across_workgroups_and_mixed_channel_counts(hooks_handle):
    h = hooks_handle
    tiny = [cases.written_stream("tiny %d" % i, 100 + i % 10, 1, 16, [16]) for i in range(10)]
    many = [tiny[i % 10] for i in range(300)]
    check(h, cases.Batch(many, gaps=[i % 3 for i in range(300)], spacing=3))
    m = cases.mixed()
    # stereo between mono and 3-channel streams (an odd number of lanes in front of every pair), 8 channels next to them
    order = [m[0], m[1], m[3], m[14], m[5], m[15], m[4], m[16], m[18], m[19], m[8], m[20], m[2], m[21], m[19]]
    check(h, cases.Batch(order, seed=7))


def test_stops_leave_their_neighbours_alone(hooks_handle):
    h = hooks_handle
    stops, base = cases.stops()
    m = cases.mixed()
    streams, caps = [], []
    for k, (name, (s, frames, why)) in enumerate(stops.items()):
        streams += [m[k], s]
        caps += [None, len(base.pcm)]
    # a slot that ends inside frame 3
    off = cases.offsets_of(base)
    streams += [m[9], base, m[6]]
    caps += [None, 3 * 192 * 4 + 100, None]
    batch = cases.Batch(streams, capacities=caps, seed=5)
    out, totals, want = check(h, batch)
    for k, (name, (s, frames, why)) in enumerate(stops.items()):
        assert want[2 * k + 1][1][0] == frames and want[2 * k + 1][1][3] == why, name
        assert want[2 * k][1][3] == 0
    i = len(streams) - 2
    assert [int(v) for v in totals[i]] == [3, 3 * 192, int(off[3]), _capi.DECODE_NO_ROOM]
    # every stop is what decode_pcm says for the stream alone
    for j, s in enumerate(streams):
        got, t = alone(h, s, batch.capacities[j])
        assert t == [int(v) for v in totals[j]] and np.array_equal(got, batch.slot(out, j)[:len(got)]), s.name
    # the second call on offset + totals[2] gives the rest
    first = batch.slot(out, i)[:3 * 192 * 4]
    rest = base.but("rest", base.data[int(totals[i][2]):])
    b2 = cases.Batch([m[0], rest], capacities=[None, len(base.pcm)])
    out2, totals2, _ = check(h, b2)
    assert int(totals2[1][3]) == 0
    assert np.array_equal(np.concatenate([first, b2.slot(out2, 1)[:len(base.pcm) - len(first)]]), base.pcm)


def test_garbage_gives_reasons_and_touches_nothing(hooks_handle):
    h = hooks_handle
    m = cases.mixed()
    streams = []
    for i, g in enumerate(cases.garbage()):
        streams += [g, m[i % len(m)]]
    batch = cases.Batch(streams, seed=11)
    out, totals, want = check(h, batch)
    assert all(want[2 * i][1][3] != 0 for i in range(32))
    assert all(np.array_equal(batch.slot(out, 2 * i + 1), m[i % len(m)].pcm) for i in range(32))


def test_the_plan_does_not_depend_on_the_number_of_streams(hooks_handle):
    h = hooks_handle
    m = cases.mixed()
    four = [m[0], m[1], m[3], m[4]]
    many = cases.Batch([four[i % 4] for i in range(400)], spacing=2)
    check(h, cases.Batch(four), max_frames=many.max_frames())   # (the candidate room sets the jump levels)
    plan4 = h.debug_last_decode_streams_plan()
    check(h, many)
    plan400 = h.debug_last_decode_streams_plan()
    assert plan4 == plan400 and plan4[3] == 4 and plan4[1] <= 3 and plan4[2] <= 6 and plan4[0] < 64
    check(h, cases.Batch([m[0], m[5]]))
    assert h.debug_last_decode_streams_plan()[3] == 1


def test_memory_kinds_give_the_same_bytes(hooks_handle):
    import torch
    h = hooks_handle
    batch = cases.Batch(cases.mixed(), seed=9)
    ref, ref_totals, want = check(h, batch)
    for kinds in (("pinned", "pinned"), ("pinned+3", "pageable"), ("pageable", "pinned+3")):
        out, totals, _ = run(h, batch, *kinds)
        assert np.array_equal(out, ref) and np.array_equal(totals, ref_totals), kinds
    dev = torch.device("cuda:0")
    d_in = torch.from_numpy(batch.data).to(dev)
    d_out = torch.full((batch.out_bytes,), FILL, dtype=torch.uint8, device=dev)
    d_tot = torch.full((len(batch.streams), 4), -1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    table = batch.table.copy()
    call, _ = h.decode_streams_device(d_in.data_ptr(), d_in.numel(), table, batch.max_frames(), d_out.data_ptr(),
                                      d_out.numel(), d_tot.data_ptr())
    table[:] = 0   # the table was read before the call returned
    assert np.array_equal(d_out.cpu().numpy(), ref)
    assert np.array_equal(d_tot.cpu().numpy().astype(np.uint64), ref_totals)
    assert call == [sum(t[0] for _, t in want), sum(t[1] for _, t in want)]


def test_arguments(hooks_handle):
    h = hooks_handle
    m = cases.mixed()
    batch = cases.Batch([m[0], m[1], m[3]], gaps=[4, 4, 4])
    lib, E = h._lib, _capi
    out = batch.fresh_out()
    totals = np.full((3, 4), 0x77, np.uint64)
    call = np.zeros(2, np.uint64)

    def rc(table=None, data=None, n_bytes=None, n_streams=None, max_frames=None, out_ptr=None, out_bytes=None,
           totals_ptr=None, call_ptr=None, table_ptr=None, kind=E.MEM_HOST):
        t = batch.table if table is None else table
        d = batch.data
        return lib.flacenc_hip_decode_streams(
            h._h, d.ctypes.data if data is None else data, len(d) if n_bytes is None else n_bytes,
            t.ctypes.data if table_ptr is None else table_ptr, len(t) if n_streams is None else n_streams,
            batch.max_frames() if max_frames is None else max_frames, out.ctypes.data if out_ptr is None else out_ptr,
            len(out) if out_bytes is None else out_bytes, totals.ctypes.data if totals_ptr is None else totals_ptr,
            call.ctypes.data if call_ptr is None else call_ptr, kind)

    def changed(i, **fields):
        t = batch.table.copy()
        for k, v in fields.items():
            t[i][k] = v
        return t

    bad = [dict(data=0), dict(table_ptr=0), dict(out_ptr=0), dict(totals_ptr=0), dict(call_ptr=0), dict(kind=7),
           dict(n_streams=(1 << 24) + 1), dict(max_frames=(1 << 30) + 1), dict(n_bytes=len(batch.data) - 60),
           dict(out_bytes=len(out) - 30), dict(table=batch.table[::-1].copy()),
           dict(table=changed(1, offset=batch.table[0]["offset"] + 3)),
           dict(table=changed(2, n_bytes=len(batch.data))), dict(table=changed(1, out_capacity=len(out))),
           dict(table=changed(0, out_offset=(1 << 64) - 1)), dict(table=changed(0, channels=0)),
           dict(table=changed(2, channels=9)), dict(table=changed(1, max_block_size=0)),
           dict(table=changed(1, max_block_size=65537)), dict(table=changed(0, bytes_per_sample=5)),
           dict(table=changed(0, bytes_per_sample=1))]
    for kw in bad:
        assert rc(**kw) == E.ERR_BAD_ARGUMENT, kw
    for bits in (3, 25, 32):
        assert rc(table=changed(1, bits_per_sample=bits, bytes_per_sample=4)) == E.ERR_UNSUPPORTED
    assert (out == FILL).all() and (totals == 0x77).all() and not call.any()
    assert rc(n_streams=0) == E.OK and (totals == 0x77).all() and (out == FILL).all()
    # too few frames: the flag, zero totals, nothing written; the retry succeeds
    frames = sum(len(s.frame_sizes) for s in batch.streams)
    assert rc(max_frames=frames - 1) == E.OK
    assert int(call[0]) == E.INDEX_ERROR and int(call[1]) == 0 and not totals.any() and (out == FILL).all()
    assert rc(max_frames=frames) == E.OK and int(call[0]) == frames
    model.check_batch(batch, out, totals)


def test_more_candidate_headers_than_the_table_holds(hooks_handle):
    """5000 planted headers in one span: with room for 64 frames (enough for the 15 there are) the candidate table holds 64 + 16 + 4096 -- the flag,
    zero totals, nothing written; with more room the good neighbours decode and the field stops with CHAIN."""
    h = hooks_handle
    m = cases.mixed()
    field = b"".join(cases.fw.header(256, 0, 16, k % 120) for k in range(5000))
    planted = cases.Stream("planted field", np.frombuffer(field, np.uint8), 1, 16, 4096)
    batch = cases.Batch([m[0], planted, m[1]])
    out, totals, call = run(h, batch, max_frames=64)
    assert call == [_capi.INDEX_ERROR, 0] and not totals.any() and (out == FILL).all()
    out, totals, want = check(h, batch, max_frames=2000)
    assert want[1][1] == [0, 0, 0, _capi.DECODE_CHAIN] and want[0][1][3] == 0 and want[2][1][3] == 0


def test_handle_reuse(hooks_handle, everything):
    h = hooks_handle
    big = cases.Batch(everything + cases.mixed(), seed=13)
    small = cases.Batch(cases.mixed()[:2])
    first = run(h, big)
    check(h, small)
    s = everything[24]
    got, _ = alone(h, s, len(s.pcm))
    assert np.array_equal(got, s.pcm)
    encoded(h, "between", 2, 16, 256, 3, 0)
    again = run(h, big)
    assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1]) and first[2] == again[2]
    model.check_batch(big, again[0], again[1])


def test_decode_many_decodes_files_in_one_call_and_checks_their_md5(hooks_handle, tmp_path):
    """tools/decode_many.py on two .flac files of tools/encode_flac.py (stereo 16-bit with a tail block, variable
    blocking): the PCM of each is its input, its STREAMINFO MD5 matches, the WAVs are written."""
    import os
    import subprocess
    import sys
    import wave
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tools"))
    import decode_flac
    import decode_many
    import encode_flac
    h = hooks_handle
    rng = np.random.default_rng(77)
    pcms = [np.cumsum(rng.integers(-300, 301, (n, 2)), axis=0).astype(np.int32).clip(-30000, 30000)
            for n in (3 * 1152 + 77, 4096 + 500)]
    files = [encode_flac.encode_pcm(pcms[0], 16, RATE, h, block_size=1152)[0],
             encode_flac.encode_pcm_variable(pcms[1], 16, RATE, h, block_size=1024, levels=3)[0]]
    results = decode_many.decode_all(files, h)
    assert h.debug_last_decode_streams_plan()[1] == 2
    for (pcm, info), want in zip(results, pcms):
        assert np.array_equal(pcm, np.ascontiguousarray(want.astype("<i2")).reshape(-1).view(np.uint8))
        assert decode_flac.md5_status(pcm, info) == "MD5 OK"
    paths = []
    for i, data in enumerate(files):
        paths.append(str(tmp_path / ("f%d.flac" % i)))
        open(paths[-1], "wb").write(data)
    p = subprocess.run([sys.executable, os.path.join(root, "tools", "decode_many.py"), *paths, "--out-dir",
                        str(tmp_path / "wavs")], check=True, capture_output=True, text=True)
    assert p.stdout.count("MD5 OK") == 2
    with wave.open(str(tmp_path / "wavs" / "f0.wav"), "rb") as w:
        assert w.getnframes() == len(pcms[0]) and w.getnchannels() == 2
        assert w.readframes(w.getnframes()) == pcms[0].astype("<i2").tobytes()
