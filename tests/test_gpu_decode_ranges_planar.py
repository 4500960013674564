"""flacenc_hip_decode_ranges_planar on the GPU: the corpus of tests/ranges_cases.py in both sample formats, in host and in
device memory, against the model of tests/planar_model.py (what flacenc_hip_decode_ranges must give, sign-extended,
de-interleaved, scaled and zero-padded), against the samples the streams were written from and against
flacenc_hip_decode_ranges' own totals on the same batch.  Slots lie in shuffled order at offsets of 0, 4, 8 and 12 mod 16
with FILL between them; whatever a call may not touch must still be FILL.  Every comparison is exact: elements are
compared as uint32 bit patterns."""
import functools

import numpy as np
import pytest

import planar_model as pmodel
import ranges_cases as rcases
import ranges_model as rmodel
import streams_cases as cases
from flacenc_rs_amd import _capi

pytestmark = pytest.mark.gpu
FILL = pmodel.FILL
I32, F32 = _capi.SAMPLE_I32, _capi.SAMPLE_F32
# launches of the planar call above flacenc_hip_decode_ranges' on the same batch: the zero pass in
# device memory, nothing in host memory (the host threads zero behind the rows they place)
EXTRA_LAUNCHES = {True: 1, False: 0}


def run(h, rb, lay, fmt, device, table=None, max_frames=None):
    """-> (out uint8, totals uint64 [n, 4], call totals)"""
    table = (rb.table if table is None else table).copy()
    rtable = lay.rtable.copy()
    max_frames = rb.max_frames() if max_frames is None else max_frames
    if not device:
        out = lay.fresh_out()
        totals, call, _ = h.decode_ranges_planar(rb.data, table, rtable, max_frames, out, fmt)
        return out, totals, call
    import torch
    dev = torch.device("cuda:0")
    d_in = torch.from_numpy(rb.data).to(dev)
    d_out = torch.full((lay.out_bytes,), FILL, dtype=torch.uint8, device=dev)
    d_tot = torch.full((len(rb.ranges), 4), -1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    call, _ = h.decode_ranges_planar_device(d_in.data_ptr(), d_in.numel(), table, rtable, max_frames, d_out.data_ptr(),
                                            d_out.numel(), fmt, d_tot.data_ptr())
    table[:] = 0   # both tables were read before the call returned
    rtable[:] = 0
    return d_out.cpu().numpy(), d_tot.cpu().numpy().astype(np.uint64), call


def packed(h, rb, table=None, max_frames=None):
    """flacenc_hip_decode_ranges on the same batch (host memory) -> (out, totals, call totals)"""
    out = rb.fresh_out()
    totals, call, _ = h.decode_ranges(rb.data, rb.table if table is None else table, rb.rtable,
                                      rb.max_frames() if max_frames is None else max_frames, out)
    return out, totals, call


@functools.lru_cache(None)
def model(which):
    rb = {"corpus": lambda: rcases.corpus()[0], "many": rcases.many_on_one, "damaged": lambda: rcases.damaged()[0],
          "garbage": rcases.with_garbage}[which]()
    return rb, rmodel.expected_batch(rb)


def check(h, which, fmt, device, seed=3):
    rb, want = model(which)
    lay = pmodel.PlanarLayout(rb, seed=seed)
    out, totals, call = run(h, rb, lay, fmt, device)
    lay.check(out, totals, pmodel.expected_slots(rb, want, fmt))
    p_out, p_totals, p_call = packed(h, rb)
    assert np.array_equal(totals, p_totals) and call == p_call
    return rb, lay, out, totals


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("fmt", [I32, F32], ids=["i32", "f32"])
def test_the_corpus_and_many_ranges_on_one_stream(hooks_handle, fmt, device):
    h = hooks_handle
    rb, lay, out, totals = check(h, "corpus", fmt, device)
    names = rcases.corpus()[1]
    assert {"nothing asked", "past the end", "begins beyond the end", "three frames, partial ends"} <= {k for _, k in names}
    for r, (s, first, n) in enumerate(rb.ranges):   # against the samples the streams were written from
        st = rb.streams[s]
        w = int(totals[r][0])
        x = pmodel.values_of(st.pcm, st.channels, st.width)[:, first:first + w]
        got = lay.slot(out, r)
        assert np.array_equal(got[:, :w], pmodel.elements_of(x, st.bps, fmt)) and not got[:, w:].any()
    check(h, "many", fmt, device, seed=4)


def sweep_stream():
    return cases.written_stream("sweep stereo 16", 41, 2, 16, [256] * 4, tags=(1, 8, 9, 10))


@pytest.mark.parametrize("residue", [4, 8, 12])
def test_the_alignment_sweep(hooks_handle, residue):
    """Every first_sample 0..20 with every length that moves the head / body / tail split, or the window across a frame
    boundary, every slot at `residue` mod 16: F32 in device memory and I32 in host memory."""
    h = hooks_handle
    st = sweep_stream()
    ranges = [(0, first, n) for first in range(21) for n in (0, 1, 3, 4, 5, 15, 16, 17, 255, 256, 257, 600)]
    rb = rcases.RangeBatch([st], ranges, seed=residue)
    want = rmodel.expected_batch(rb)
    assert all(t[0] == n and t[1] == 0 for (_, _, n), (_, t) in zip(ranges, want))
    lay = pmodel.PlanarLayout(rb, seed=residue, residues=(residue,))
    assert all(o % 16 == residue for o in lay.offsets)
    for fmt, device in ((F32, True), (I32, False)):
        out, totals, _ = run(h, rb, lay, fmt, device)
        lay.check(out, totals, pmodel.expected_slots(rb, want, fmt))


def test_values_that_do_not_fit_the_bit_depth(hooks_handle):
    """Hand-built frames: I32 is what flacenc_hip_decode_ranges stores in a 4-byte container, F32 is numpy.float32 of it
    times 2^-(bits - 1), bit for bit."""
    h = hooks_handle
    streams = pmodel.odd_streams()
    ranges = []
    for i, s in enumerate(streams):
        n = s.frame_sizes[0][1]
        ranges += [(i, 0, n), (i, 3, n - 8), (i, n - 10, 25)]
    rb = rcases.RangeBatch(streams, ranges, seed=7)
    assert (rb.table["bytes_per_sample"] == 4).all()
    p_out, p_totals, p_call = packed(h, rb)
    narrow = rb.table.copy()
    narrow["bytes_per_sample"] = (narrow["bits_per_sample"] + 7) // 8
    lay = pmodel.PlanarLayout(rb, seed=8)
    beyond = 0
    for fmt, device in ((I32, True), (F32, True), (F32, False), (I32, False)):
        out, totals, call = run(h, rb, lay, fmt, device, table=narrow)
        assert np.array_equal(totals, p_totals) and call == p_call
        mask = np.ones(len(out), bool)
        for r, (i, first, n) in enumerate(ranges):
            s = streams[i]
            w = int(totals[r][0])
            assert w == min(n, s.frame_sizes[0][1] - first) and w > 0
            at = rb.slot_offsets[r]
            v = pmodel.values_of(p_out[at:at + w * s.channels * 4], s.channels, 4)
            beyond += bool((np.abs(v.astype(np.int64)) > 1 << (s.bps - 1)).any())
            got = lay.slot(out, r)
            if fmt == I32:
                assert np.array_equal(got[:, :w].view(np.int32), v), (s.name, r)
            else:
                want = (v.astype(np.float32) * np.float32(2.0 ** -(s.bps - 1))).astype(np.float32)
                assert np.array_equal(got[:, :w], want.view(np.uint32)), (s.name, r)
            assert not got[:, w:].any()
            mask[lay.offsets[r]:lay.offsets[r] + lay.sizes[r]] = False
        assert (out[mask] == FILL).all()
    assert beyond


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_damage_and_garbage(hooks_handle, device):
    h = hooks_handle
    rb, lay, out, totals = check(h, "damaged", F32, device, seed=5)
    for name, i, D, why in rcases.damaged()[1]:
        mine = [r for r, x in enumerate(rb.ranges) if x[0] == i]
        assert [int(totals[r][1]) for r in mine] == [0, why, why], name
        assert [int(totals[r][0]) for r in mine] == [min(50, D), min(10, D), 0], name
        for r in mine:   # written up to w, zero behind it
            w = int(totals[r][0])
            assert not lay.slot(out, r)[:, w:].any()
    good = [r for r, x in enumerate(rb.ranges) if rb.streams[x[0]].pcm is not None and x[0] % 2 == 0]
    assert good and all(int(totals[r][1]) == 0 and int(totals[r][0]) == 60 for r in good)
    rg, lay, out, totals = check(h, "garbage", I32, device, seed=6)
    for r, (s, first, n) in enumerate(rg.ranges):
        if s % 2:   # the good neighbours of the garbage are unaffected
            st = rg.streams[s]
            assert int(totals[r][0]) == n and int(totals[r][1]) == 0
            x = pmodel.values_of(st.pcm, st.channels, st.width)[:, first:first + n]
            assert np.array_equal(lay.slot(out, r).view(np.int32), x)


def test_index_error_writes_nothing(hooks_handle):
    h = hooks_handle
    m = cases.mixed()
    streams = [m[0], m[1], m[3]]
    # 6 + 6 + 6 + 9 + 9 range-frames on 20 chain frames
    ranges = [(0, 0, 1297), (0, 0, 1297), (0, 1, 1296), (1, 0, 1576), (1, 3, 1573)]
    rb = rcases.RangeBatch(streams, ranges)
    lay = pmodel.PlanarLayout(rb)
    for device in (False, True):
        for max_frames in (19, 20, 35):
            out, totals, call = run(h, rb, lay, F32, device, max_frames=max_frames)
            assert call == [_capi.INDEX_ERROR, 0] and not totals.any() and (out == FILL).all(), (device, max_frames)
        out, totals, call = run(h, rb, lay, F32, device, max_frames=36)
        assert call[0] == 36
        lay.check(out, totals, pmodel.expected_slots(rb, rmodel.expected_batch(rb), F32))


def test_the_new_bad_arguments_leave_out_untouched(hooks_handle):
    h = hooks_handle
    m = cases.mixed()
    rb = rcases.RangeBatch([m[0], m[1], m[3]], [(0, 10, 50), (1, 0, 20), (2, 100, 7)])
    lay = pmodel.PlanarLayout(rb)
    lib, E = h._lib, _capi
    out = lay.fresh_out()
    totals = np.full((3, 4), 0x77, np.uint64)
    call = np.zeros(2, np.uint64)

    def rc(rtable=None, out_bytes=None, fmt=F32, kind=E.MEM_HOST, table=None, h_ptr=None):
        r = lay.rtable if rtable is None else rtable
        t = rb.table if table is None else table
        return lib.flacenc_hip_decode_ranges_planar(
            h._h if h_ptr is None else h_ptr, rb.data.ctypes.data, len(rb.data), t.ctypes.data, len(t), r.ctypes.data,
            len(r), rb.max_frames(), out.ctypes.data, len(out) if out_bytes is None else out_bytes, fmt,
            totals.ctypes.data, call.ctypes.data, kind)

    def changed(i, **fields):
        t = lay.rtable.copy()
        for k, v in fields.items():
            t[i][k] = v
        return t

    last = max(range(3), key=lambda r: lay.offsets[r] + lay.sizes[r])
    end = lay.offsets[last] + lay.sizes[last]
    bad = [dict(rtable=changed(0, out_offset=lay.offsets[0] + 1)), dict(rtable=changed(1, out_offset=lay.offsets[1] + 2)),
           dict(rtable=changed(2, out_offset=lay.offsets[2] + 3)), dict(out_bytes=end - 1), dict(out_bytes=end - 4),
           dict(rtable=changed(last, out_offset=lay.offsets[last] + 16)),
           dict(rtable=changed(0, out_offset=(1 << 64) - 4)), dict(rtable=changed(0, n_samples=(1 << 62) + 1)),
           dict(rtable=changed(0, n_samples=(1 << 64) - 11)), dict(fmt=2), dict(fmt=0xFFFFFFFF),
           # and what flacenc_hip_decode_ranges refuses
           dict(rtable=changed(1, stream=3)), dict(rtable=changed(0, reserved=1)), dict(kind=7)]
    for kw in bad:
        assert rc(**kw) == E.ERR_BAD_ARGUMENT, kw
    assert (out == FILL).all() and (totals == 0x77).all() and not call.any()
    assert rc(out_bytes=end) == E.OK
    lay.check(out, totals, pmodel.expected_slots(rb, rmodel.expected_batch(rb), F32))


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_the_plan_does_not_depend_on_the_number_of_ranges(hooks_handle, device):
    h = hooks_handle
    m = cases.mixed()
    mono = [m[0], m[5], m[20], m[13]]
    three = rcases.RangeBatch(mono, [(i, 30 + i, 300) for i in range(3)])
    thirty = [mono[i % 4] for i in range(30)]
    many = rcases.RangeBatch(thirty, [(r % 30, (37 * r) % 500, 1 + (r * 13) % 290) for r in range(300)], seed=5)
    plans = {}
    for name, rb in (("3", three), ("300", many)):
        lay = pmodel.PlanarLayout(rb)
        out, totals, _ = run(h, rb, lay, F32, device, max_frames=many.max_frames())   # (the room sets the jump levels)
        planar = h.debug_last_decode_ranges_plan()
        lay.check(out, totals, pmodel.expected_slots(rb, rmodel.expected_batch(rb), F32))
        if device:
            import torch
            dev = torch.device("cuda:0")
            d_in = torch.from_numpy(rb.data).to(dev)
            d_out = torch.zeros(rb.out_bytes, dtype=torch.uint8, device=dev)
            d_tot = torch.zeros((len(rb.ranges), 4), dtype=torch.int64, device=dev)
            torch.cuda.synchronize()
            h.decode_ranges_device(d_in.data_ptr(), d_in.numel(), rb.table, rb.rtable, many.max_frames(),
                                   d_out.data_ptr(), d_out.numel(), d_tot.data_ptr())
        else:
            packed(h, rb, max_frames=many.max_frames())
        base = h.debug_last_decode_ranges_plan()
        assert planar[0] == base[0] + EXTRA_LAUNCHES[device] and planar[1:] == base[1:], (name, planar, base)
        plans[name] = planar
    assert plans["3"] == plans["300"] and plans["3"][3] == 1 and plans["3"][1] == 2


def test_crop_flac_writes_the_crops_as_one_array(hooks_handle, tmp_path):
    """tools/crop_flac.py --npy: one float32 [files, channels, samples] array, the input's samples scaled, zero behind the
    end of the file that ends inside the crop; without the option the tool writes what it always wrote."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tools"))
    import crop_flac
    import encode_flac
    h = hooks_handle
    rate = 8000
    rng = np.random.default_rng(79)
    pcms = [np.cumsum(rng.integers(-300, 301, (n, 2)), axis=0).astype(np.int32).clip(-30000, 30000)
            for n in (5 * 1152 + 77, 4 * 1024 + 500)]
    files = [encode_flac.encode_pcm(pcms[0], 16, rate, h, block_size=1152, seektable=0.25)[0],
             encode_flac.encode_pcm(pcms[1], 16, rate, h, block_size=1024)[0]]
    start, seconds = 0.5, 0.2
    a, n = int(start * rate), int(seconds * rate)
    want = np.zeros((2, 2, n), np.float32)
    for i, p in enumerate(pcms):
        part = p[a:a + n].T.astype(np.float32) / np.float32(32768)
        want[i, :, :part.shape[1]] = part
    batch, notes = crop_flac.crop_all_planar(files, h, start, seconds)
    assert [w for w, _, _ in notes] == [n, 596] and batch.dtype == np.float32
    assert np.array_equal(batch.view(np.uint32), want.view(np.uint32))
    paths = []
    for i, data in enumerate(files):
        paths.append(str(tmp_path / ("f%d.flac" % i)))
        open(paths[-1], "wb").write(data)
    subprocess.run([sys.executable, os.path.join(root, "tools", "crop_flac.py"), *paths, "--start", str(start), "--seconds",
                    str(seconds), "--out-dir", str(tmp_path / "wavs"), "--npy", str(tmp_path / "crops.npy")], check=True,
                   capture_output=True, text=True)
    assert np.array_equal(np.load(str(tmp_path / "crops.npy")).view(np.uint32), want.view(np.uint32))
    assert sorted(os.listdir(str(tmp_path / "wavs"))) == ["f0.wav", "f1.wav"]
    with pytest.raises(ValueError, match="one shape"):
        faster = encode_flac.encode_pcm(pcms[0], 16, 2 * rate, h, block_size=1152)[0]   # twice the samples per second
        crop_flac.crop_all_planar([files[0], faster], h, start, seconds)


def test_decode_crops_gives_the_batch_tensor(hooks_handle):
    import torch
    from flacenc_rs_amd import crops
    h = hooks_handle
    m = cases.mixed()
    streams = [m[1], m[8], m[14], m[15]]   # stereo, 16 bits: 1576, 2461, 1280 and 799 samples
    batch = cases.Batch(streams, capacities=[0] * 4)
    T = 500
    picks = [(0, 0), (1, 2000), (2, 1279), (3, 400), (0, 1576), (1, 77), (3, 5000), (2, 3)]
    truths = [rmodel.truth(s) for s in streams]
    assert any(0 < t.samples - first < T for (s, first), t in ((p, truths[p[0]]) for p in picks))   # reach past the end
    d_bytes = torch.from_numpy(batch.data).to("cuda:0")
    for dtype, fmt in ((torch.float32, F32), (torch.int32, I32)):
        out, totals = crops.decode_crops(h, d_bytes, batch.table, picks, T, dtype=dtype, max_frames=batch.max_frames())
        assert out.shape == (len(picks), 2, T) and out.dtype == dtype and out.device == d_bytes.device
        assert totals.shape == (len(picks), 4) and totals.device == d_bytes.device
        got = out.cpu().numpy().view(np.uint32)
        for b, (s, first) in enumerate(picks):
            data, tot = truths[s].expected(first, T)
            assert totals[b].tolist() == tot
            assert np.array_equal(got[b], pmodel.slot_of(data, 2, 2, 16, T, fmt)), (b, s, first)
    out, totals = crops.decode_crops(h, d_bytes, batch.table, picks, T)   # the defaults: float32, a bound for max_frames
    assert out.dtype == torch.float32 and np.array_equal(out.cpu().numpy().view(np.uint32), np.stack(
        [pmodel.slot_of(truths[s].expected(first, T)[0], 2, 2, 16, T, F32) for s, first in picks]))
    # host memory: the same tensor on the CPU
    cpu, _ = crops.decode_crops(h, torch.from_numpy(batch.data), batch.table, picks, T, max_frames=batch.max_frames())
    assert cpu.device.type == "cpu" and torch.equal(cpu, out.cpu())
    # mixed channel counts fail before anything runs
    mixed = cases.Batch([m[0], m[1]], capacities=[0, 0])
    with pytest.raises(ValueError, match="one channel count"):
        crops.decode_crops(h, torch.from_numpy(mixed.data).to("cuda:0"), mixed.table, [(0, 0), (1, 0)], 64)
    with pytest.raises(ValueError):
        crops.decode_crops(h, d_bytes, batch.table, [(4, 0)], 64)
    with pytest.raises(ValueError):
        crops.decode_crops(h, d_bytes, batch.table, picks, T, dtype=torch.float16)
