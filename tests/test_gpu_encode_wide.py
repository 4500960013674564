"""The wide encode path on the GPU (flacenc_hip_encode_pack_frames_wide, flacenc_hip_set_max_encode_bits_per_sample):
the opt-in, the device step against tests/wide_model.py byte for byte, against the existing frame-level path at 16 and
24 bits, a mixed batch through flacenc_hip_encode_streams and back through the decoder, and the planar call.  Every test
makes its own handles; every comparison is exact."""
import hashlib

import numpy as np
import pytest

import depth32_cases as d32
import encode_streams_cases as cases
import encode_streams_model as model
import wide_cases as wc
import wide_model as wm
from flacenc_rs_amd import _capi

pytestmark = pytest.mark.gpu
FILL = cases.FILL
BAD = _capi.ERR_BAD_ARGUMENT


def frame_config(cfg, wasted=False, use_lpc=False, lpc_order=8):
    """The C config of a wide_model config; use_lpc and the LPC fields are not read on the wide path."""
    q = _capi.make_config(lpc_order=lpc_order, max_rice_parameter=cfg["max_rice_parameter"],
                          flags=_capi.FLAG_WASTED_BITS if wasted else 0)
    return _capi.make_frame_config(q, use_constant=cfg["use_constant"], use_fixed=cfg["use_fixed"], use_lpc=use_lpc,
                                   use_leftside=cfg["use_leftside"], use_rightside=cfg["use_rightside"],
                                   use_midside=cfg["use_midside"], fixed_max_order=cfg["fixed_max_order"],
                                   fixed_order_sel=_capi.ORDERSEL_BITCOUNT)


def pcm32(x):
    return cases.pack(np.asarray(x, np.int64).astype(np.int32), 4)


def stream_of(name, x, bps, width, rate=44100):
    x = np.ascontiguousarray(np.asarray(x, np.int64).astype(np.int32))
    return cases.Stream(name, x, x.shape[0], bps, width, rate)


# ---------------------------------------------------------------- 1. the opt-in
def test_more_than_24_bits_needs_the_opt_in_and_24_restores_the_refusal():
    rng = np.random.default_rng(1)
    fc = frame_config(wm.make_cfg())
    block = 192
    with _capi.Handle(0) as h:
        for bits in (25, 32):
            x = d32.sinusoid(rng, 500, bps=bits)[None].repeat(2, axis=0)
            pcm = pcm32(x)
            table = np.zeros(1, _capi.PCM_STREAM_DESC_DTYPE)
            table[0] = (0, 500, 0, 3 * cases.slot_bound(2, block, bits), 2, bits, 4, 44100)
            planar = np.ascontiguousarray(x.astype(np.int32))

            def calls(expect_ok):
                out = np.full(int(table[0]["out_capacity"]), FILL, np.uint8)
                lens = np.full(3, 0xA5A5A5A5, np.uint32)
                try:
                    got, glens = h.encode_pcm(pcm, 2, fc, 4, bits, block, 44100, out=out, out_len=lens)
                    rc = _capi.OK
                except _capi.FlacencHipError as e:
                    rc, got = e.code, out[:0]
                assert (rc == _capi.OK) == expect_ok and (expect_ok or rc == BAD), ("encode_pcm", bits, rc)
                if not expect_ok:
                    assert (out == FILL).all() and (lens == 0xA5A5A5A5).all()
                alone = got.tobytes()
                out[:] = FILL
                _, totals, call, rc = h.encode_streams(pcm, table, fc, block, out, check=False)
                assert (rc == _capi.OK) == expect_ok and (expect_ok or rc == BAD), ("encode_streams", bits, rc)
                assert (out == FILL).all() if not expect_ok else out[:int(totals[0][1])].tobytes() == alone
                out[:] = FILL
                res = h.encode_streams_planar(planar, _capi.SAMPLE_I32, 0, table, fc, block, out, check=False)
                assert (res[-1] == _capi.OK) == expect_ok and (expect_ok or res[-1] == BAD), ("planar", bits, res[-1])
                assert (out == FILL).all() if not expect_ok else out[:int(res[1][0][1])].tobytes() == alone
                return alone

            calls(False)
            h.set_max_encode_bits_per_sample(32)
            alone = calls(True)
            want = b"".join(wm.encode_frame(x[:, f * block:(f + 1) * block], bits, wm.make_cfg(), number=f)[0] for f in range(3))
            assert alone == want
            h.set_max_encode_bits_per_sample(24)
            calls(False)
        for bad in (0, 16, 25, 31, 33, 64):
            with pytest.raises(_capi.FlacencHipError) as e:
                h.set_max_encode_bits_per_sample(bad)
            assert e.value.code == BAD
        # the decode limit is another setting
        h.set_max_bits_per_sample(32)
        calls(False)
    assert _capi.load().flacenc_hip_set_max_encode_bits_per_sample(None, 32) == BAD


# ---------------------------------------------------------------- 2. the model
@pytest.mark.parametrize("wasted", (False, True))
def test_the_device_step_writes_the_models_frames(wasted):
    """Cases of one shape share a launch where their configs agree; each shape is also launched as a dozen frames (the
    case's frame among copies of the others of its shape, numbered from 120 so that the coded number grows)."""
    groups = {}
    for c, (want, _) in zip(wc.cases(), wc.modelled(wasted)):
        key = (c["x"].shape, c["bps"], tuple(sorted(c["cfg"].items())))
        groups.setdefault(key, []).append((c, want))
    with _capi.Handle(0) as h:
        for (shape, bps, _), members in groups.items():
            cfg = members[0][0]["cfg"]
            fc = frame_config(cfg, wasted, use_lpc=True)
            frames = np.stack([c["x"] for c, _ in members]).astype(np.int32)
            got = h.encode_frames_wide(frames, bps, fc, first_frame_number=0, frame_number_step=0)
            for (c, want), frame in zip(members, got):
                assert frame == want, c["name"]
            dozen = np.concatenate([frames] * (12 // len(members) + 1))[:12]
            got = h.encode_frames_wide(dozen, bps, fc, first_frame_number=120, frame_number_step=1)
            for f in (0, 7, 8, 11):
                c = members[f % len(members)][0]
                want, _ = wm.encode_frame(c["x"], bps, dict(cfg, wasted_bits=wasted), number=120 + f)
                assert got[f] == want, (c["name"], f)


def test_the_wide_step_checks_its_arguments():
    import torch
    fc = frame_config(wm.make_cfg())
    with _capi.Handle(0) as h:
        rows = torch.zeros((2, 64), dtype=torch.int32, device="cuda")
        bound = cases.slot_bound(2, 64, 32)
        out = torch.full((bound,), FILL, dtype=torch.uint8, device="cuda")
        lens = torch.full((1,), 77, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()

        def rc_of(channels=2, block=64, stride=64, bits=32, stride_out=bound, number=0, cfg=fc):
            try:
                h.encode_pack_frames_wide_device(cfg, rows.data_ptr(), 1, channels, block, stride, bits, 44100, number, 1,
                                                 out.data_ptr(), stride_out, lens.data_ptr())
            except _capi.FlacencHipError as e:
                return e.code
            return _capi.OK

        for kw in (dict(channels=0), dict(channels=9), dict(block=0), dict(block=32768), dict(stride=63), dict(bits=7),
                   dict(bits=33), dict(stride_out=bound - 16), dict(stride_out=bound + 8), dict(number=1 << 31)):
            assert rc_of(**kw) == BAD, kw
        assert rc_of(cfg=frame_config(wm.make_cfg(max_rice_parameter=31))) == _capi.ERR_BAD_CONFIG
        assert rc_of(cfg=frame_config(wm.make_cfg(fixed_max_order=5))) == _capi.ERR_BAD_CONFIG
        h.synchronize()
        torch.cuda.synchronize()
        assert (out.cpu().numpy() == FILL).all() and int(lens.cpu()[0]) == 77


# ---------------------------------------------------------------- 3. the existing path at 16 and 24 bits
def existing_frames(h, frames, bps, fc):
    """flacenc_hip_encode_pack_stereo_frames_async / _frames_async on a host array -> the frames' bytes."""
    import torch
    x = np.ascontiguousarray(frames, np.int32)
    nf, ch, n = x.shape
    bound = cases.slot_bound(ch, n, bps)
    rows = torch.from_numpy(x.copy()).to("cuda")
    out = torch.zeros((nf, bound), dtype=torch.uint8, device="cuda")
    lens = torch.zeros(nf, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    if ch == 2:
        rec = torch.zeros(nf * _capi.FRAME_RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        h.encode_pack_stereo_frames_device(fc, rows.data_ptr(), nf, n, n, bps, 44100, 0, 1, rec.data_ptr(), out.data_ptr(),
                                           bound, lens.data_ptr(), stream)
    else:
        rec = torch.zeros(nf * ch * _capi.CHANNEL_RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        h.encode_pack_frames_device(fc, rows.data_ptr(), nf, ch, n, n, bps, 44100, 0, 1, rec.data_ptr(), out.data_ptr(),
                                    bound, lens.data_ptr(), stream)
    torch.cuda.synchronize()
    got, lengths = out.cpu().numpy(), lens.cpu().numpy()
    return [got[f, : int(lengths[f])].tobytes() for f in range(nf)]


def narrow_frames(rng, channels, n, bps):
    """A dozen frames of `bps` bits: tones of several levels, content of bps - 8 bits shifted up (k = 8), a constant
    channel, silence, one channel a copy of another (a zero side), white noise."""
    def tone(scale, bits=bps):
        return d32.sinusoid(rng, n, scale=scale, bps=bits)
    out = []
    for f in range(12):
        rows = [tone((1.0, 0.3, 0.01, 0.001)[(f + c) % 4]) for c in range(channels)]
        if f % 4 == 1:
            rows = [tone(0.5, bps - 8) << 8 for _ in range(channels)]
        if f == 2:
            rows[-1] = np.full(n, -1234 << 4, np.int64)
        if f == 3:
            rows = [np.zeros(n, np.int64) for _ in range(channels)]
        if f == 6:
            rows[-1] = rows[0].copy()
        if f == 7:
            rows[0] = rng.integers(-(1 << (bps - 1)), 1 << (bps - 1), n)
        if f == 9:
            rows = [(r >> 3) << 3 for r in rows]
        out.append(np.stack(rows))
    return np.stack(out).astype(np.int32)


@pytest.mark.parametrize("bps", (16, 24))
@pytest.mark.parametrize("channels", (1, 2, 3))
def test_at_16_and_24_bits_the_wide_step_equals_the_existing_path(bps, channels):
    rng = np.random.default_rng(bps * 10 + channels)
    with _capi.Handle(0) as h:
        for n in (17, 64, 192, 1000, 4096):
            frames = narrow_frames(rng, channels, n, bps)
            for wasted in (False, True):
                fc = frame_config(wm.make_cfg(), wasted, use_lpc=False)
                want = existing_frames(h, frames, bps, fc)
                got = h.encode_frames_wide(frames, bps, fc)
                for f in range(len(frames)):
                    assert got[f] == want[f], (n, wasted, f)


# ---------------------------------------------------------------- 4., 5. a mixed batch, and the way back
BLOCK = 64


def mixed_batch():
    rng = np.random.default_rng(0x4D1)
    def pair(n, bps, scale=1.0):
        return np.stack([d32.sinusoid(rng, n, scale=scale, bps=bps), d32.sinusoid(rng, n, scale=scale * 0.5, bps=bps)])
    wide = [stream_of("32-bit opposed, tail 17", d32.opposed_pair(rng, 5 * BLOCK + 17), 32, 4),
            stream_of("32-bit mono, 130 frames", d32.sinusoid(rng, 130 * BLOCK)[None], 32, 4),
            stream_of("32-bit 3 ch, tail 40", np.stack([d32.sinusoid(rng, 2 * BLOCK + 40, scale=s) for s in (1, 0.1, 1e-4)]), 32, 4, 48000),
            stream_of("25-bit pair, tail 63", pair(BLOCK + 63, 25), 25, 4),
            stream_of("32-bit skewed, no room", d32.skewed_pair(rng, 4 * BLOCK), 32, 4),
            stream_of("32-bit empty", np.zeros((2, 0)), 32, 4)]
    narrow = [cases.stream("16-bit stereo, tail 17", 3 * BLOCK + 17, 2, 16, 2, 44100, 31),
              cases.stream("24-bit mono, tail 5", 2 * BLOCK + 5, 1, 24, 3, 44100, 32),
              cases.stream("16-bit empty", 0, 2, 16, 2, 44100, 33),
              cases.stream("24-bit stereo, tail 33", 6 * BLOCK + 33, 2, 24, 3, 48000, 34),
              cases.stream("16-bit 3 ch in 4 bytes, whole", 4 * BLOCK, 3, 16, 4, 44100, 35)]
    order = [wide[0], narrow[0], wide[1], narrow[1], narrow[2], wide[2], wide[3], narrow[3], wide[4], wide[5], narrow[4]]
    return order, wide, narrow


def run_streams(h, streams, cfg, capacities=None, seed=7):
    lay = cases.layout(streams, BLOCK, capacities=capacities, seed=seed)
    out = np.full(lay.out_bytes, FILL, np.uint8)
    lens, totals, call, _ = h.encode_streams(lay.pcm, lay.table, cfg, BLOCK, out)
    return lay, out, np.array(lens, copy=True), np.array(totals, copy=True), call


def test_a_mixed_batch_of_16_24_and_32_bit_streams_and_the_way_back():
    streams, wide, narrow = mixed_batch()
    mcfg = wm.make_cfg()
    fc = frame_config(mcfg, use_lpc=True)
    with _capi.Handle(0) as h, _capi.Handle(0) as fresh:
        h.set_max_encode_bits_per_sample(32)
        alone = []
        for s in streams:
            if s.x.shape[1] == 0:
                alone.append((b"", np.zeros(0, np.uint32)))
                continue
            got, lens = h.encode_pcm(cases.pack(s.x, s.width), s.channels, fc, s.width, s.bps, BLOCK, s.rate)
            alone.append((got.tobytes(), np.array(lens, copy=True)))
        no_room = streams.index(wide[4])
        caps = [None] * len(streams)
        caps[no_room] = int(alone[no_room][1][:3].sum()) - 1  # two frames fit, the third does not
        lay, out, lens, totals, call = run_streams(h, streams, fc, caps)
        assert (out[~cases.slot_map(lay.table, lay.out_bytes)] == FILL).all()
        first = 0
        for i, s in enumerate(streams):
            want, wlens = alone[i]
            off, cap = int(lay.table[i]["out_offset"]), int(lay.table[i]["out_capacity"])
            j, used = model.cut(wlens, cap)
            assert [int(v) for v in totals[i]] == model.totals(wlens, cap, first), s.name
            assert np.array_equal(lens[first:first + len(wlens)], wlens), s.name
            assert out[off:off + used].tobytes() == want[:used], s.name
            assert (out[off + used:off + cap] == FILL).all(), s.name
            first += len(wlens)
        assert int(totals[no_room][0]) == 2 and int(totals[no_room][3]) == _capi.ENCODE_NO_ROOM
        assert all(int(totals[i][3]) == 0 for i in range(len(streams)) if i != no_room)
        # the streams of more than 24 bits are the model's, with every frame's own number (two bytes from frame 128 on)
        for s in wide:
            i = streams.index(s)
            x = s.x.astype(np.int64)
            frames = [wm.encode_frame(x[:, t:t + BLOCK], s.bps, mcfg, number=t // BLOCK, rate=s.rate)[0]
                      for t in range(0, x.shape[1], BLOCK)]
            assert alone[i][0] == b"".join(frames), s.name
            assert [len(f) for f in frames] == list(alone[i][1]), s.name
        long_one = alone[streams.index(wide[1])]
        assert len(long_one[1]) == 130 and long_one[0][int(long_one[1][:128].sum()) + 4] == 0xC2  # frame 128: 0xC2 0x80
        # the streams of 24 bits or fewer: what a handle without the opt-in writes for them alone
        lay_n, out_n, lens_n, totals_n, _ = run_streams(fresh, narrow, fc, seed=9)
        for k, s in enumerate(narrow):
            i = streams.index(s)
            assert int(totals_n[k][1]) == int(totals[i][1]) == len(alone[i][0]), s.name
            o = int(lay_n.table[k]["out_offset"])
            assert out_n[o:o + int(totals_n[k][1])].tobytes() == alone[i][0], s.name

        # ---- the way back: flacenc_hip_decode_streams_md5 at limit 32 ----
        # (the decoder takes its spans in ascending order: the slots as they lie in `out`)
        kept = [int(i) for i in np.argsort(lay.table["out_offset"], kind="stable") if i != no_room]
        spans = {i: cases.pack(streams[i].x, (streams[i].bps + 7) // 8) for i in kept}
        table = np.zeros(len(kept), _capi.STREAM_DESC_DTYPE)
        at = 0
        for k, i in enumerate(kept):
            s = streams[i]
            table[k] = (int(lay.table[i]["out_offset"]), int(totals[i][1]), at, len(spans[i]), s.channels, s.bps, BLOCK,
                        (s.bps + 7) // 8)
            at += len(spans[i])
        back = np.zeros(max(1, at), np.uint8)
        n_frames = sum(int(totals[i][0]) for i in kept)
        with pytest.raises(_capi.FlacencHipError):
            fresh.decode_streams_md5(out, table, n_frames, back)  # a decoder without its own opt-in refuses the depth
        h.set_max_bits_per_sample(32)
        t, c, _, digests = h.decode_streams_md5(out, table, n_frames, back)
        assert (t[:, 3] == 0).all() and c[0] == n_frames
        for k, i in enumerate(kept):
            o = int(table[k]["out_offset"])
            assert np.array_equal(back[o:o + len(spans[i])], spans[i]), streams[i].name
            assert digests[k].tobytes() == hashlib.md5(spans[i].tobytes()).digest(), streams[i].name


# ---------------------------------------------------------------- 6. planar
def test_planar_int32_at_32_bits_equals_encode_streams_and_float32_is_refused():
    rng = np.random.default_rng(0x91A)
    B, C, T = 4, 2, 5 * BLOCK + 17
    totals_of = (T, 3 * BLOCK, 0, BLOCK + 1)
    tensor = np.zeros((B, C, T), np.int32)
    streams = []
    for b, total in enumerate(totals_of):
        x = d32.opposed_pair(rng, T) if b % 2 == 0 else d32.skewed_pair(rng, T)
        tensor[b] = x.astype(np.int32)
        streams.append(stream_of("planar %d" % b, x[:, :total], 32, 4))
    fc = frame_config(wm.make_cfg())
    with _capi.Handle(0) as h:
        h.set_max_encode_bits_per_sample(32)
        lay = cases.layout(streams, BLOCK, seed=3)
        out = np.full(lay.out_bytes, FILL, np.uint8)
        lens, totals, call, _ = h.encode_streams(lay.pcm, lay.table, fc, BLOCK, out)
        table = lay.table.copy()
        table["offset"] = np.arange(B) * (C * T * 4)
        pout = np.full(lay.out_bytes, FILL, np.uint8)
        plens, ptotals, pcall, digests, clipped, rc = h.encode_streams_planar(tensor, _capi.SAMPLE_I32, T, table, fc, BLOCK, pout)
        assert rc == _capi.OK and pcall == call and np.array_equal(plens, lens) and np.array_equal(ptotals, totals)
        assert np.array_equal(pout, out) and (clipped == 0).all()
        for b, s in enumerate(streams):
            assert digests[b].tobytes() == hashlib.md5(cases.pack(s.x, 4).tobytes()).digest(), s.name
        pout[:] = FILL
        res = h.encode_streams_planar(tensor.view(np.float32), _capi.SAMPLE_F32, T, table, fc, BLOCK, pout, check=False)
        assert res[-1] == BAD and (pout == FILL).all()
