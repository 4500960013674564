"""use_direct_mse / mae_optimization_steps on the GPU, held to the oracle on every case of tests/direct_mse_cases.py
(which tests/test_direct_mse_cases_cpu.py holds to the branch each case names, and the oracle to the covariance method's
exact system): every kernel form of launch_direct_mse -- the sliding-window chains on aligned rows at every order and
window edge, the batched solve across workgroups with a ragged last one, and the one-kernel form in its six
instantiations on device rows with an odd stride or an offset base -- on worst-case material.

  * status, R[] bits, unquantised solution bits, record fields and residual rows equal the oracle's; the residual decodes
    to the input;
  * device rows: the canary words between and behind the sample rows and the residual rows are intact, and the result is
    the one of the same rows passed aligned;
  * frame level: decisions, records, residual rows and frame bytes equal the oracle's controller and bit writer; every
    packed frame decodes to its input through flacenc_hip_verify_frames and tests/flac_parse.py;
  * composition with RICE_ESCAPE, WASTED_BITS, the streaming PCM call and the block-size search;
  * blocks the estimator cannot see (block_size < 64, so every n <= P) answer what include/flacenc_hip.h documents.
Everything is exact."""
import numpy as np
import pytest

import direct_mse_cases as dc
import flac_parse
import flac_write as fw
import pack_cases as pc
import wasted_model as wm
from flacenc_rs_amd import _capi
from oracle import oracle as orc
from test_gpu_direct_mse import exact, gcfg, ocfg, records_equal

pytestmark = pytest.mark.gpu

RATE = 44100
CANARY_IN, CANARY_OUT = 0x5A5A1234, 0x0BADF00D


@pytest.fixture(scope="module")
def handle():
    h = _capi.Handle(0)
    yield h
    h.close()


def frame_cfgs(c, flags=0):
    g = _capi.make_frame_config(gcfg(c.order, c.steps, window=c.window, flags=flags), use_fixed=True)
    o = orc.make_frame_config(ocfg(c.order, c.steps, window=c.window), use_fixed=True,
                              fixed=orc.make_fixed_config(sum_mode=orc.SUMABS_CANONICAL))
    return g, o


def decode_check(h, frames, x, bps):
    """Every frame decodes to its input: the GPU verifier on all of them, tests/flac_parse.py on all of them."""
    nf, ch, n = x.shape
    lens = np.array([len(b) for b in frames], np.uint32)
    offs = np.concatenate([[0], np.cumsum(lens[:-1], dtype=np.uint64)]).astype(np.uint64)
    st = h.verify_frames(b"".join(frames), offs, lens, ch, bps, n, np.ascontiguousarray(x.reshape(nf * ch, n)))
    assert not st.any(), st
    for f in range(nf):
        got = flac_parse.parse_frame(frames[f], bps, RATE, wasted_ok=True)
        assert np.array_equal(np.asarray(got["channels"], np.int64), x[f]), f


# ---- the entry points on host rows (staged at a padded stride: aligned) ----
def host_stereo_qlpc(h, c, x):
    gp, gres = h.stereo_qlpc_batch(x, c.bps, gcfg(c.order, c.steps, window=c.window))
    check_stereo_qlpc(c, x, gp, gres)
    return gp, gres


def check_stereo_qlpc(c, x, gp, gres):
    w = np.array([c.bps, c.bps, c.bps, c.bps + 1], np.uint8)
    for f in range(x.shape[0]):
        m, s = orc.stereo_to_midside(x[f, 0], x[f, 1])
        rows = np.stack([x[f, 0], x[f, 1], m, s])
        rp, rres, _, _ = orc.qlpc_batch(rows, w, ocfg(c.order, c.steps, window=c.window))
        assert (gp[f]["status"] == 0).all(), (c.name, f)
        records_equal(gp[f], rp)
        assert np.array_equal(gres[f], rres), (c.name, f)
        for k in range(4):
            o = int(gp[f, k]["order"])
            got = orc.decode_lpc(rows[k][:o], gp[f, k]["coefs"][:o], int(gp[f, k]["shift"]), gres[f, k])
            assert np.array_equal(got, rows[k]), (c.name, f, k)


def check_stereo_frames(h, c, x, res, resid):
    """test_frame_pipeline_and_bytes' comparison, and every packed frame decoded."""
    _, ofc = frame_cfgs(c)
    want, wres = orc.encode_stereo_frames_cfg(x, c.bps, ofc)
    assert res["channel_assignment"].tolist() == want["channel_assignment"].tolist(), c.name
    assert res["kind"].tolist() == want["kind"].tolist() and res["bits"].tolist() == want["bits"].tolist(), c.name
    assert np.array_equal(resid, wres), c.name
    assert res.tobytes() == want.tobytes(), c.name
    packed = h.pack_stereo_frames(x, res, resid, c.bps, RATE)
    for f in range(len(x)):
        assert packed[f] == orc.write_stereo_frame(res[f], x[f, 0], x[f, 1], c.bps, RATE, f, resid[f, 0], resid[f, 1]), \
            (c.name, f)
    decode_check(h, packed, x, c.bps)


def check_frames3(h, c, x, res, resid):
    """Kind, bits, record and residual row of every channel == oracle.encode_subframe; the packed frame == the frame
    tests/flac_write.py writes from the oracle's subframes; every frame decoded."""
    _, ofc = frame_cfgs(c)
    packed = h.pack_frames(x, res, resid, c.bps, RATE)
    for f in range(x.shape[0]):
        subs = [wm.subframe(x[f, ch], c.bps, ofc, wasted=False) for ch in range(x.shape[1])]
        for ch, s in enumerate(subs):
            w, g = s["enc"], res[f, ch]
            assert int(g["kind"]) == w["kind"] and int(g["bits"]) == w["bits"], (c.name, f, ch)
            if w["kind"] == _capi.KIND_LPC:
                qp = w["lpc"].qp
                assert int(g["params"]["order"]) == qp.order and int(g["params"]["shift"]) == qp.shift, (c.name, f, ch)
                assert g["params"]["coefs"][:qp.order].tolist() == [int(v) for v in qp.coefs[:qp.order]]
            if w["kind"] >= 2:
                assert np.array_equal(resid[f, ch], w["residual"]), (c.name, f, ch)
        want = fw.frame(list(x[f]), x.shape[1] - 1, c.bps, [wm._write_args(s) for s in subs], number=f)
        assert packed[f] == want, (c.name, f)
    decode_check(h, packed, x, c.bps)


HOST_CASES = [c for c in dc.GPU_CASES if c.layout == "host"]
DEVICE_CASES = [c for c in dc.GPU_CASES if c.layout != "host"]


@pytest.mark.parametrize("name", [c.name for c in HOST_CASES])
def test_aligned_rows_equal_the_oracle(handle, name):
    c = dc.by_name(name)
    x = dc.case_rows(c)
    if c.entry == "qlpc":
        exact(handle, x, dc.case_bps(c), c.order, c.steps, window=c.window)
    elif c.entry == "stereo_qlpc":
        host_stereo_qlpc(handle, c, x)
    else:
        assert c.entry == "stereo_frames"
        res, resid = handle.encode_stereo_frames(x, c.bps, frame_cfgs(c)[0])
        check_stereo_frames(handle, c, x, res, resid)


# ---- device rows with an odd stride or an offset base: the one-kernel form ----
class DeviceRows:
    """`rows` [k, n] int32 laid out on the device by a layout of direct_mse_cases, canaries everywhere else."""

    def __init__(self, rows, layout):
        import torch
        k, n = rows.shape
        self.stride, self.off = dc.layout_stride(layout, n)
        self.host = np.full(self.off + k * self.stride + 8, CANARY_IN, np.int32)
        for i in range(k):
            self.host[self.off + i * self.stride:self.off + i * self.stride + n] = rows[i]
        self.dev = torch.from_numpy(self.host).cuda()
        assert self.dev.data_ptr() % 16 == 0
        self.ptr = self.dev.data_ptr() + 4 * self.off
        assert self.ptr % 16 != 0 or self.stride % 4 != 0

    def intact(self):
        return np.array_equal(self.dev.cpu().numpy(), self.host)


class DeviceOut:
    """Residual rows at a stride of n + 3 words behind one canary word, canaries between and behind the rows."""

    def __init__(self, k, n):
        import torch
        self.k, self.n, self.stride = k, n, n + 3
        self.dev = torch.full((1 + k * self.stride + 8,), CANARY_OUT, dtype=torch.int32, device="cuda")
        self.ptr = self.dev.data_ptr() + 4

    def rows(self):
        a = self.dev.cpu().numpy()
        body = a[1:1 + self.k * self.stride].reshape(self.k, self.stride)
        assert a[0] == CANARY_OUT and (a[1 + self.k * self.stride:] == CANARY_OUT).all(), "behind the residual rows"
        assert (body[:, self.n:] == CANARY_OUT).all(), "between the residual rows"
        return body[:, :self.n].copy()


def dev_zeros(nbytes):
    import torch
    return torch.zeros(nbytes, dtype=torch.uint8, device="cuda")


def fetch(t, dtype):
    return t.cpu().numpy().view(dtype)


@pytest.mark.parametrize("name", [c.name for c in DEVICE_CASES])
def test_unaligned_device_rows_equal_the_oracle_and_the_aligned_call(handle, name):
    import torch
    c = dc.by_name(name)
    h = handle
    x = dc.case_rows(c)
    n = c.n
    stream = torch.cuda.current_stream().cuda_stream
    rows = DeviceRows(np.ascontiguousarray(x.reshape(-1, n)), c.layout)
    assert dc.case_form(c)["chains"].startswith("one-kernel")
    if c.entry == "qlpc":
        k = len(x)
        bps = dc.case_bps(c)
        d_bps = torch.from_numpy(bps).cuda()
        out = DeviceOut(k, n)
        d_p, d_R, d_A = dev_zeros(k * _capi.PARAMS_DTYPE.itemsize), dev_zeros(k * 33 * 8), dev_zeros(k * 32 * 8)
        h.qlpc_batch_device(gcfg(c.order, c.steps, window=c.window), rows.ptr, k, n, rows.stride, d_bps.data_ptr(),
                            d_p.data_ptr(), out.ptr, out.stride, d_R.data_ptr(), d_A.data_ptr(), stream=stream)
        torch.cuda.synchronize()
        gp, gres = fetch(d_p, _capi.PARAMS_DTYPE), out.rows()
        gR, gA = fetch(d_R, np.float64).reshape(k, 33), fetch(d_A, np.float64).reshape(k, 32)
        assert rows.intact()
        hp, hres, hR, hA = h.qlpc_batch(x, bps, gcfg(c.order, c.steps, window=c.window), want_fp=True)
        assert gp.tobytes() == hp.tobytes() and np.array_equal(gres, hres), name
        assert np.array_equal(gR.view(np.uint64), hR.view(np.uint64)), name
        assert np.array_equal(gA.view(np.uint64), hA.view(np.uint64)), name
        exact(h, x, bps, c.order, c.steps, window=c.window)            # ... and that one is the oracle's
    elif c.entry == "stereo_qlpc":
        nf = len(x)
        out = DeviceOut(nf * 4, n)
        d_p = dev_zeros(nf * 4 * _capi.PARAMS_DTYPE.itemsize)
        h.stereo_qlpc_batch_device(gcfg(c.order, c.steps, window=c.window), rows.ptr, nf, n, rows.stride, c.bps,
                                   d_p.data_ptr(), out.ptr, out.stride, stream=stream)
        torch.cuda.synchronize()
        gp, gres = fetch(d_p, _capi.PARAMS_DTYPE).reshape(nf, 4), out.rows().reshape(nf, 4, n)
        assert rows.intact()
        check_stereo_qlpc(c, x, gp, gres)
        hp, hres = h.stereo_qlpc_batch(x, c.bps, gcfg(c.order, c.steps, window=c.window))
        assert gp.tobytes() == hp.tobytes() and np.array_equal(gres, hres), name
    elif c.entry == "stereo_frames":
        nf = len(x)
        out = DeviceOut(nf * 2, n)
        d_res = dev_zeros(nf * _capi.FRAME_RESULT_DTYPE.itemsize)
        h.encode_stereo_frames_device(frame_cfgs(c)[0], rows.ptr, nf, n, rows.stride, c.bps, d_res.data_ptr(), out.ptr,
                                      out.stride, stream=stream)
        torch.cuda.synchronize()
        res, resid = fetch(d_res, _capi.FRAME_RESULT_DTYPE), out.rows().reshape(nf, 2, n)
        assert rows.intact()
        check_stereo_frames(h, c, x, res, resid)
        hres, hresid = h.encode_stereo_frames(x, c.bps, frame_cfgs(c)[0])
        assert res.tobytes() == hres.tobytes() and np.array_equal(resid, hresid), name
    else:
        assert c.entry == "frames3"
        nf, ch, _ = x.shape
        out = DeviceOut(nf * ch, n)
        d_res = dev_zeros(nf * ch * _capi.CHANNEL_RESULT_DTYPE.itemsize)
        h.encode_frames_device(frame_cfgs(c)[0], rows.ptr, nf, ch, n, rows.stride, c.bps, d_res.data_ptr(), out.ptr,
                               out.stride, stream=stream)
        torch.cuda.synchronize()
        res, resid = fetch(d_res, _capi.CHANNEL_RESULT_DTYPE).reshape(nf, ch), out.rows().reshape(nf, ch, n)
        assert rows.intact()
        hres, hresid = h.encode_frames(x, c.bps, frame_cfgs(c)[0])
        assert res["kind"].tolist() == hres["kind"].tolist() and res["bits"].tolist() == hres["bits"].tolist(), name
        coded = res["kind"] >= 2                                       # (a Constant / Verbatim channel writes no row)
        assert np.array_equal(resid[coded], hresid[coded]), name
        assert res["params"][coded].tobytes() == hres["params"][coded].tobytes(), name
        check_frames3(h, c, x, res, np.where(coded[:, :, None], resid, hresid))


def test_three_channels_on_aligned_rows(handle):
    c = dc.by_name("one-kernel 3 channels irls")._replace(layout="host")
    x = dc.case_rows(c)
    res, resid = handle.encode_frames(x, c.bps, frame_cfgs(c)[0])
    check_frames3(handle, c, x, res, resid)


# ---- blocks the estimator cannot see ----
@pytest.mark.parametrize("n", [8, 5, 63])
def test_blocks_below_64_samples_answer_what_the_header_documents(handle, n):
    """include/flacenc_hip.h: the candidate batches require 64 <= block_size and answer FLACENC_HIP_ERR_BAD_ARGUMENT
    below it; the frame-level calls take 1 <= block_size and run encode_subframe's too_short branch, Constant or
    Verbatim only -- so n <= P (n = 8 and n = 5 at order 8) never reaches the estimator, with or without IRLS steps, and
    the frames equal the oracle's."""
    import torch
    c = dc.Case("short", n, 8, 1, 16, dc.RECT, "stereo_frames", "host", ("equal::1", "silent::2", "hi_lo"), None)
    x = dc.case_rows(c)
    mono = np.ascontiguousarray(x.reshape(-1, n))
    for steps in (0, 1):
        q = gcfg(8, steps, window=dc.RECT)
        with pytest.raises(_capi.FlacencHipError) as e:
            handle.qlpc_batch(mono, 16, q)
        assert e.value.code == _capi.ERR_BAD_ARGUMENT
        with pytest.raises(_capi.FlacencHipError) as e:
            handle.stereo_qlpc_batch(x, 16, q)
        assert e.value.code == _capi.ERR_BAD_ARGUMENT
        d = torch.from_numpy(mono).cuda()
        d_p = dev_zeros(len(mono) * _capi.PARAMS_DTYPE.itemsize)
        d_r = torch.zeros_like(d)
        for call in (lambda: handle.qlpc_batch_device(q, d.data_ptr(), len(mono), n, n, 0, d_p.data_ptr(),
                                                      d_r.data_ptr(), n),
                     lambda: handle.stereo_qlpc_batch_device(q, d.data_ptr(), len(x), n, n, 16, d_p.data_ptr(),
                                                             d_r.data_ptr(), n)):
            with pytest.raises(_capi.FlacencHipError) as e:
                call()
            assert e.value.code == _capi.ERR_BAD_ARGUMENT
        cs = c._replace(steps=steps)
        res, resid = handle.encode_stereo_frames(x, 16, frame_cfgs(cs)[0])
        assert (res["kind"] <= _capi.KIND_VERBATIM).all()
        check_stereo_frames(handle, cs, x, res, resid)
        x3 = np.ascontiguousarray(np.concatenate([x, x[:, :1]], axis=1))
        r3, s3 = handle.encode_frames(x3, 16, frame_cfgs(cs)[0])
        assert (r3["kind"] <= _capi.KIND_VERBATIM).all()
        check_frames3(handle, cs, x3, r3, s3)
        # the streaming PCM call with a tail of n samples: the tail's frame is the frame-level call's
        fr = stream_frames(2, 1152)
        pcm = np.ascontiguousarray(fr.transpose(0, 2, 1)).reshape(-1, 2)[:1152 + n]
        raw = np.ascontiguousarray(pcm.astype("<i2")).view(np.uint8).reshape(-1)
        fcfg = frame_cfgs(cs)[0]
        data, lens = handle.encode_pcm_stereo(raw, fcfg, 2, 16, 1152, RATE)
        tail = np.ascontiguousarray(fr[1:, :, :n])
        tres, tresid = handle.encode_stereo_frames(tail, 16, fcfg)
        assert (tres["kind"] <= _capi.KIND_VERBATIM).all() and len(lens) == 2
        want = handle.pack_stereo_frames(tail, tres, tresid, 16, RATE, first_frame_number=1)[0]
        assert bytes(data)[int(lens[0]):] == want
        check_stereo_frames(handle, cs, tail, tres, tresid)


# ---- composition ----
def half_silent(n, bits):
    x = dc.material("music", n, bits, 3)
    x[n // 2:] = 0
    return x


@pytest.mark.parametrize("n", [1000, 4096])
@pytest.mark.parametrize("steps", [0, 1])
def test_rice_escape_composes(handle, n, steps):
    """The flagged records == escape_model.flagged_record on the unflagged direct-MSE record and row."""
    from test_gpu_rice_escape import check_candidates
    x = np.stack([dc.material("ramp", n, 24), half_silent(n, 24), dc.material("ramp", n, 16),
                  half_silent(n, 16)]).astype(np.int32)
    bps = np.array([24, 24, 16, 16], np.uint8)
    p0 = exact(handle, x, bps, 8, steps, window=dc.RECT)
    _, r0, R0, A0 = handle.qlpc_batch(x, bps, gcfg(8, steps, window=dc.RECT), want_fp=True)
    p1, r1, R1, A1 = handle.qlpc_batch(x, bps, gcfg(8, steps, window=dc.RECT, flags=_capi.FLAG_RICE_ESCAPE), want_fp=True)
    assert np.array_equal(r0, r1) and np.array_equal(R0, R1) and np.array_equal(A0, A1)
    assert check_candidates(p1, p0, r0, "lpc", bps, ("direct mse", n, steps)) >= 1


@pytest.mark.parametrize("steps", [0, 1])
def test_wasted_bits_compose(handle, steps):
    """16-bit content in a 24-bit container: the frame's bytes equal the oracle's encode of the shifted rows, written at
    the reduced width (tests/wasted_model.py); every frame decodes to its input."""
    n = 4096
    x16 = np.stack([dc.stereo_pair(p, n, 16, k) for k, p in enumerate(("equal", "silent", "square_noise"))])
    x = (x16.astype(np.int64) << 8).astype(np.int32)
    kw = dict(use_direct_mse=True, mae_optimization_steps=steps, window=dc.RECT)
    cfg = _capi.make_frame_config(gcfg(8, steps, window=dc.RECT, flags=_capi.FLAG_WASTED_BITS), use_fixed=True)
    fc = wm.frame_config(order=8, **kw)
    res, resid = handle.encode_stereo_frames(x, 24, cfg)
    frames = handle.pack_stereo_frames(x, res, resid, 24, RATE)
    for f in range(len(x)):
        assert frames[f] == wm.stereo_frame_bytes(x[f, 0], x[f, 1], 24, fc, number=f), f
        a, subs = wm.stereo_decision(x[f, 0], x[f, 1], 24, fc)
        assert any(subs[i]["k"] == 8 for i in wm.STEREO_ROLES[a]), f
    assert any(int(k) == _capi.KIND_LPC for k in res["kind"].reshape(-1))
    decode_check(handle, frames, x, 24)


def stream_frames(n_frames, n):
    names = ("equal", "square_noise", "silent", "inverted")
    return np.stack([dc.stereo_pair(names[f % 4], n, 16, f + 1) for f in range(n_frames)]).astype(np.int32)


@pytest.mark.parametrize("steps", [0, 1])
def test_the_streaming_pcm_call_equals_the_frame_level_call(handle, steps):
    """3 blocks of 1152 and a 700-sample tail: every frame is the frame-level call's on the same block and decodes to it."""
    n, tail = 1152, 700
    fr = stream_frames(4, n)
    pcm = np.ascontiguousarray(fr.transpose(0, 2, 1)).reshape(-1, 2)[:3 * n + tail]
    raw = np.ascontiguousarray(pcm.astype("<i2")).view(np.uint8).reshape(-1)
    cfg = _capi.make_frame_config(gcfg(8, steps, window=dc.RECT), use_fixed=True)
    data, lens = handle.encode_pcm_stereo(raw, cfg, 2, 16, n, RATE)
    data = bytes(data)
    res, resid = handle.encode_stereo_frames(fr[:3], 16, cfg)
    want = handle.pack_stereo_frames(fr[:3], res, resid, 16, RATE)
    last = np.ascontiguousarray(fr[3:, :, :tail])
    res, resid = handle.encode_stereo_frames(last, 16, cfg)
    want += handle.pack_stereo_frames(last, res, resid, 16, RATE, first_frame_number=3)
    assert [int(v) for v in lens] == [len(b) for b in want] and data == b"".join(want)
    decode_check(handle, want[:3], fr[:3], 16)
    decode_check(handle, want[3:], last, 16)
    c = dc.Case("pcm", n, 8, steps, 16, dc.RECT, "stereo_frames", "host", (), None)
    check_stereo_frames(handle, c, fr[:3], *handle.encode_stereo_frames(fr[:3], 16, cfg))   # ... which is the oracle's


@pytest.mark.parametrize("steps", [0, 1])
def test_the_block_size_search_equals_the_frame_level_call(handle, steps):
    """4096 at 2 levels: every frame's body is the frame-level call's on the same block, and decodes to it."""
    n = 4096
    fr = stream_frames(3, n)
    cfg = _capi.make_frame_config(gcfg(8, steps, window=dc.RECT), use_fixed=True)
    v = handle.encode_variable(fr, 16, cfg, 2, sample_rate=RATE)
    assert not v["overflow"]
    sizes, t = set(), 0
    for i in range(v["frames"]):
        b = int(v["block_sizes"][i])
        sb, at = divmod(t, n)
        frame = v["data"][int(v["offsets"][i]):int(v["offsets"][i]) + int(v["lengths"][i])]
        block = np.ascontiguousarray(fr[sb:sb + 1, :, at:at + b])
        res, resid = handle.encode_stereo_frames(block, 16, cfg)
        want = handle.pack_stereo_frames(block, res, resid, 16, RATE)[0]
        assert pc.body_of(frame) == pc.body_of(want), i
        got = flac_parse.parse_frame(frame, 16, RATE)
        assert np.array_equal(np.asarray(got["channels"], np.int64), block[0]), i
        sizes.add(b)
        t += b
    assert t == 3 * n and sizes <= {n, n // 2}
