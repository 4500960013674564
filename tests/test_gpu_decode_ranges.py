"""flacenc_hip_decode_ranges on the GPU: the corpus of tests/ranges_cases.py in host and in device memory against the model
of tests/ranges_model.py (what flacenc_hip_decode_streams gives with unlimited room + the slice rule), against the
samples the streams were written from and against the slice of flacenc_hip_decode_streams' own output on the same batch
-- bytes, totals and seek points.  Slots lie in shuffled order at odd offsets and at offsets of 2 mod 4 with FILL between
them; whatever a call may not touch must still be FILL.  Every comparison is exact."""
import numpy as np
import pytest

import ranges_cases as rcases
import ranges_model as rmodel
import streams_cases as cases
from flacenc_rs_amd import _capi

pytestmark = pytest.mark.gpu
FILL = cases.FILL


def run(h, rb, max_frames=None):
    out = rb.fresh_out()
    totals, call, _ = h.decode_ranges(rb.data, rb.table, rb.rtable, rb.max_frames() if max_frames is None else max_frames,
                                      out)
    return out, totals, call


def run_device(h, rb):
    import torch
    dev = torch.device("cuda:0")
    d_in = torch.from_numpy(rb.data).to(dev)
    d_out = torch.full((max(1, rb.out_bytes),), FILL, dtype=torch.uint8, device=dev)
    d_tot = torch.full((len(rb.ranges), 4), -1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    table, rtable = rb.table.copy(), rb.rtable.copy()
    call, _ = h.decode_ranges_device(d_in.data_ptr(), d_in.numel(), table, rtable, rb.max_frames(), d_out.data_ptr(),
                                     d_out.numel(), d_tot.data_ptr())
    table[:] = 0   # both tables were read before the call returned
    rtable[:] = 0
    return d_out.cpu().numpy(), d_tot.cpu().numpy().astype(np.uint64), call


def check(h, rb, device=False, **kw):
    out, totals, call = run_device(h, rb) if device else run(h, rb, **kw)
    want = rmodel.check_batch(rb, out, totals)
    assert call[1] == sum(t[0] for _, t in want)
    return out, totals, call, want


def whole_streams(h, rb):
    """flacenc_hip_decode_streams on the same batch with room for everything -> per stream (PCM, totals)."""
    streams = [cases.Stream(s.name, s.data, s.channels, s.bps, s.mbs, None, s.width) for s in rb.streams]
    # what the stream was written from (damage only takes away), or for garbage what its bytes could hold
    room = [(sum(n for _, n in s.frame_sizes) if s.frame_sizes else (len(s.data) // 9 + 1) * s.mbs) * s.channels * s.width
            if len(s.data) else 0 for s in rb.streams]
    batch = cases.Batch(streams, capacities=room, spacing=8)
    out = batch.fresh_out()
    totals, call, _ = h.decode_streams(batch.data, batch.table, batch.max_frames(), out)
    assert not call[0] & _capi.INDEX_ERROR
    return [(batch.slot(out, i)[:int(totals[i][1]) * s.channels * s.width], [int(v) for v in totals[i]])
            for i, s in enumerate(streams)]


def equals_the_slice_of_decode_streams(h, rb, out, totals):
    whole = whole_streams(h, rb)
    for r, (s, first, n) in enumerate(rb.ranges):
        pcm, (_, S, consumed, W) = whole[s]
        fb = rb.streams[s].channels * rb.streams[s].width
        end = min(first + n, S)
        written = max(0, end - first)
        assert int(totals[r][0]) == written
        assert int(totals[r][1]) == (0 if written == n else (W or _capi.DECODE_RANGE_END))
        at = rb.slot_offsets[r]
        assert np.array_equal(out[at:at + written * fb], pcm[first * fb:(first + written) * fb]), (r, rb.ranges[r])
        if first >= S:
            assert [int(v) for v in totals[r][2:]] == [consumed, S]


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_the_corpus_equals_the_model_ground_truth_and_the_slice_of_decode_streams(hooks_handle, device):
    h = hooks_handle
    rb, names = rcases.corpus()
    out, totals, call, want = check(h, rb, device=device)
    for r, (s, first, n) in enumerate(rb.ranges):   # against the samples the streams were written from
        st = rb.streams[s]
        fb = st.channels * st.width
        w = int(totals[r][0])
        assert np.array_equal(out[rb.slot_offsets[r]:rb.slot_offsets[r] + w * fb], st.pcm[first * fb:(first + w) * fb])
    # the frame decodes: per range, the frames between the one that holds `first` and the one that holds the last sample
    frames = 0
    for s, first, n in rb.ranges:
        pos = rcases.starts_of(rb.streams[s])
        end = min(first + n, int(pos[-1]))
        if end > first:
            frames += int(np.searchsorted(pos, end - 1, side="right")) - int(np.searchsorted(pos, first, side="right")) + 1
    assert call[0] == frames
    equals_the_slice_of_decode_streams(h, rb, out, totals)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_many_ranges_on_one_stream_damage_and_garbage(hooks_handle, device):
    h = hooks_handle
    check(h, rcases.many_on_one(), device=device)
    rb, info = rcases.damaged()
    out, totals, _, want = check(h, rb, device=device)
    equals_the_slice_of_decode_streams(h, rb, out, totals)
    for name, i, D, why in info:
        mine = [r for r, x in enumerate(rb.ranges) if x[0] == i]
        assert [int(totals[r][1]) for r in mine] == [0, why, why], name
        assert [int(totals[r][0]) for r in mine] == [min(50, D), min(10, D), 0], name
    good = [r for r, x in enumerate(rb.ranges) if rb.streams[x[0]].pcm is not None and x[0] % 2 == 0]
    assert good and all(int(totals[r][1]) == 0 and int(totals[r][0]) == 60 for r in good)
    rg = rcases.with_garbage()
    out, totals, _, _ = check(h, rg, device=device)
    equals_the_slice_of_decode_streams(h, rg, out, totals)
    for r, (s, first, n) in enumerate(rg.ranges):
        if s % 2:   # the good neighbours of the garbage are unaffected
            st = rg.streams[s]
            fb = st.channels * st.width
            assert int(totals[r][0]) == n and int(totals[r][1]) == 0
            assert np.array_equal(out[rg.slot_offsets[r]:rg.slot_offsets[r] + n * fb], st.pcm[first * fb:(first + n) * fb])


def test_spans_at_seek_points_and_returned_seek_points_give_the_same_bytes(hooks_handle):
    h = hooks_handle
    m = cases.mixed()
    chosen = [m[0], m[1], m[3], m[8], m[9], m[4]]
    for which in ("first", "last"):
        streams, ranges, shifts = [], [], []
        for i, s in enumerate(chosen):
            pos = rcases.starts_of(s)
            k = 1 if which == "first" else len(s.frame_sizes) - 1
            first, n = int(pos[k]) + 5, min(40, int(pos[-1]) - int(pos[k]) - 5)
            streams += [s, rcases.span_from(s, k)]
            ranges += [(2 * i, first, n), (2 * i + 1, first - int(pos[k]), n)]
        rb = rcases.RangeBatch(streams, ranges, seed=31)
        out, totals, _, _ = check(h, rb)
        slot = lambda r: out[rb.slot_offsets[r]:rb.slot_offsets[r] + rb.slot_bytes[r]]   # noqa: E731
        for i in range(len(chosen)):
            assert int(totals[2 * i][0]) == ranges[2 * i][2] and np.array_equal(slot(2 * i), slot(2 * i + 1))
            assert int(totals[2 * i + 1][3]) == 0 and int(totals[2 * i + 1][2]) == 0   # the span's first frame holds it
        # the seek points of this call, fed to a second: offset + [2] as the span, first_sample - [3] as the range
        again, ranges2 = [], []
        for i, s in enumerate(chosen):
            off, pos = int(totals[2 * i][2]), int(totals[2 * i][3])
            again.append(cases.Stream(s.name + " from its seek point", s.data[off:], s.channels, s.bps, s.mbs, None, s.width))
            ranges2.append((i, ranges[2 * i][1] - pos, ranges[2 * i][2]))
        rb2 = rcases.RangeBatch(again, ranges2, seed=32)
        out2, totals2, _, _ = check(h, rb2)
        for i in range(len(chosen)):
            assert np.array_equal(out2[rb2.slot_offsets[i]:rb2.slot_offsets[i] + rb2.slot_bytes[i]], slot(2 * i))
            assert [int(v) for v in totals2[i]] == [ranges2[i][2], 0, 0, 0]


def test_the_plan_depends_on_the_channel_counts_only(hooks_handle):
    h = hooks_handle
    m = cases.mixed()
    mono = [m[0], m[5], m[20], m[13]]
    four = rcases.RangeBatch(mono, [(i, 30 + i, 300) for i in range(4)])
    forty = [mono[i % 4] for i in range(40)]
    many = rcases.RangeBatch(forty, [(r % 40, (37 * r) % 500, 1 + (r * 13) % 290) for r in range(400)], seed=5)
    check(h, four, max_frames=many.max_frames())   # (the candidate room sets the jump levels)
    plan4 = h.debug_last_decode_ranges_plan()
    check(h, many)
    plan400 = h.debug_last_decode_ranges_plan()
    assert plan4 == plan400 and plan4[3] == 1 and plan4[1] == 2 and plan4[2] <= 5 and plan4[0] < 64
    # every further channel count among the ranges' streams adds exactly one launch: its ranges_decode_kernel
    mix = [m[0], m[1], m[3], m[4]]
    plans = []
    for k in (1, 2, 3, 4):
        rb = rcases.RangeBatch(mix, [(i % k, 11, 100) for i in range(8)], seed=k)
        check(h, rb, max_frames=many.max_frames())
        plans.append(h.debug_last_decode_ranges_plan())
    for k in (1, 2, 3):
        assert plans[k][3] == k + 1 and plans[k][0] == plans[0][0] + k and plans[k][1:3] == plans[0][1:3]
    # the streams' channel counts do not count, the ranges' do
    assert plans[0] == plan4
    # decode_streams' own plan hook is not touched by this call
    before = h.debug_last_decode_streams_plan()
    check(h, four)
    assert h.debug_last_decode_streams_plan() == before


def test_index_error_by_chain_frames_and_by_range_frames_then_a_clean_call(hooks_handle):
    h = hooks_handle
    m = cases.mixed()
    streams = [m[0], m[1], m[3]]
    chain = sum(len(s.frame_sizes) for s in streams)
    # 6 + 6 + 6 + 9 + 9 range-frames on 20 chain frames
    ranges = [(0, 0, 1297), (0, 0, 1297), (0, 1, 1296), (1, 0, 1576), (1, 3, 1573)]
    rb = rcases.RangeBatch(streams, ranges)
    touched = 36
    assert chain == 20 and touched > chain
    for max_frames in (chain - 1, chain, touched - 1):
        out, totals, call = run(h, rb, max_frames=max_frames)
        assert call == [_capi.INDEX_ERROR, 0] and not totals.any() and (out == FILL).all(), max_frames
    out, totals, call, _ = check(h, rb, max_frames=touched)
    assert call[0] == touched
    out, totals, call, _ = check(h, rb, device=True)
    assert call[0] == touched
    # the device-memory totals of a failed call are zero too
    import torch
    dev = torch.device("cuda:0")
    d_in = torch.from_numpy(rb.data).to(dev)
    d_out = torch.full((rb.out_bytes,), FILL, dtype=torch.uint8, device=dev)
    d_tot = torch.full((len(ranges), 4), -1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    call, _ = h.decode_ranges_device(d_in.data_ptr(), d_in.numel(), rb.table, rb.rtable, touched - 1, d_out.data_ptr(),
                                     d_out.numel(), d_tot.data_ptr())
    assert call == [_capi.INDEX_ERROR, 0] and not d_tot.cpu().numpy().any() and (d_out.cpu().numpy() == FILL).all()
    check(h, rcases.many_on_one())


def test_arguments(hooks_handle):
    h = hooks_handle
    m = cases.mixed()
    rb = rcases.RangeBatch([m[0], m[1], m[3]], [(0, 10, 50), (1, 0, 20), (2, 100, 7)])
    lib, E = h._lib, _capi
    out = rb.fresh_out()
    totals = np.full((3, 4), 0x77, np.uint64)
    call = np.zeros(2, np.uint64)

    def rc(table=None, rtable=None, data=None, n_bytes=None, n_streams=None, n_ranges=None, max_frames=None, out_ptr=None,
           out_bytes=None, totals_ptr=None, call_ptr=None, table_ptr=None, rtable_ptr=None, kind=E.MEM_HOST):
        t = rb.table if table is None else table
        r = rb.rtable if rtable is None else rtable
        d = rb.data
        return lib.flacenc_hip_decode_ranges(
            h._h, d.ctypes.data if data is None else data, len(d) if n_bytes is None else n_bytes,
            t.ctypes.data if table_ptr is None else table_ptr, len(t) if n_streams is None else n_streams,
            r.ctypes.data if rtable_ptr is None else rtable_ptr, len(r) if n_ranges is None else n_ranges,
            rb.max_frames() if max_frames is None else max_frames, out.ctypes.data if out_ptr is None else out_ptr,
            len(out) if out_bytes is None else out_bytes, totals.ctypes.data if totals_ptr is None else totals_ptr,
            call.ctypes.data if call_ptr is None else call_ptr, kind)

    def changed(which, i, **fields):
        t = (rb.table if which == "stream" else rb.rtable).copy()
        for k, v in fields.items():
            t[i][k] = v
        return t

    last = max(range(3), key=lambda r: rb.slot_offsets[r] + rb.slot_bytes[r])
    bad = [dict(data=0), dict(table_ptr=0), dict(rtable_ptr=0), dict(out_ptr=0), dict(totals_ptr=0), dict(call_ptr=0),
           dict(kind=7), dict(n_streams=(1 << 24) + 1), dict(n_ranges=(1 << 24) + 1), dict(max_frames=(1 << 30) + 1),
           dict(n_bytes=len(rb.data) - 60), dict(table=rb.table[::-1].copy()),
           dict(table=changed("stream", 2, channels=9)), dict(table=changed("stream", 0, bytes_per_sample=1)),
           dict(rtable=changed("range", 1, stream=3)), dict(rtable=changed("range", 0, reserved=1)),
           dict(rtable=changed("range", 2, first_sample=(1 << 64) - 3)),
           dict(rtable=changed("range", 2, n_samples=(1 << 64) - 1, first_sample=0)),
           dict(rtable=changed("range", last, out_offset=rb.slot_offsets[last] + 8)),
           dict(rtable=changed("range", 0, out_offset=(1 << 64) - 1)), dict(out_bytes=rb.slot_offsets[last] + 3),
           dict(n_streams=2)]
    for kw in bad:
        assert rc(**kw) == E.ERR_BAD_ARGUMENT, kw
    assert rc(table=changed("stream", 1, bits_per_sample=25, bytes_per_sample=4)) == E.ERR_UNSUPPORTED
    assert (out == FILL).all() and (totals == 0x77).all() and not call.any()
    assert rc(n_ranges=0) == E.OK and (totals == 0x77).all() and (out == FILL).all()
    assert h.debug_last_decode_ranges_plan() == [0, 0, 0, 0]
    assert rc() == E.OK
    rmodel.check_batch(rb, out, totals)


def test_crop_flac_crops_files_from_their_seek_points_in_one_call(hooks_handle, tmp_path):
    """tools/encode_flac.py --seektable writes the points, tools/crop_flac.py starts at them: the crops are the input's
    samples, the file without a SEEKTABLE is byte-identical to what the tool has always written, one call for all."""
    import os
    import sys
    import wave
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tools"))
    import crop_flac
    import encode_flac
    import flac_metadata
    h = hooks_handle
    rate = 8000
    rng = np.random.default_rng(78)
    pcms = [np.cumsum(rng.integers(-300, 301, (n, 2)), axis=0).astype(np.int32).clip(-30000, 30000)
            for n in (7 * 1152 + 77, 4 * 1024 + 500)]
    plain = encode_flac.encode_pcm(pcms[0], 16, rate, h, block_size=1152)[0]
    files = [encode_flac.encode_pcm(pcms[0], 16, rate, h, block_size=1152, seektable=0.25)[0],
             encode_flac.encode_pcm_variable(pcms[1], 16, rate, h, block_size=1024, levels=3, seektable=0.1)[0], plain]
    info, points, first = flac_metadata.read_blocks(files[0])
    assert [p[0] for p in points] == [0, 1152, 3456, 5760, 6912] and files[0][first:] == plain[flac_metadata.read_blocks(plain)[2]:]
    assert flac_metadata.read_blocks(plain)[1] is None
    start, seconds = 0.5, 0.2
    results = crop_flac.crop_all(files, h, start, seconds)
    assert h.debug_last_decode_ranges_plan()[1] == 2
    a, n = int(start * rate), int(seconds * rate)
    for (pcm, info, seek), want in zip(results, [pcms[0], pcms[1], pcms[0]]):
        assert np.array_equal(pcm, np.ascontiguousarray(want[a:a + n].astype("<i2")).reshape(-1).view(np.uint8))
        assert seek[0] <= a
    assert results[0][2][0] == 3456 and results[2][2] == (0, 0, 0) and results[1][2][0] > 0
    paths = []
    for i, data in enumerate(files[:2]):
        paths.append(str(tmp_path / ("f%d.flac" % i)))
        open(paths[-1], "wb").write(data)
    import subprocess
    subprocess.run([sys.executable, os.path.join(root, "tools", "crop_flac.py"), *paths, "--start", str(start), "--seconds",
                    str(seconds), "--out-dir", str(tmp_path / "wavs")], check=True, capture_output=True, text=True)
    for name, want in (("f0.wav", pcms[0][a:a + n]), ("f1.wav", pcms[1][a:a + n])):
        with wave.open(str(tmp_path / "wavs" / name), "rb") as w:
            assert w.getnframes() == len(want) and w.getnchannels() == 2 and w.getframerate() == rate
            assert w.readframes(len(want)) == want.astype("<i2").tobytes()
    assert len(pcms[0][a:a + n]) == n and len(pcms[1][a:a + n]) == 596   # the second file ends inside the crop
