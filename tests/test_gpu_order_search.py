"""FLACENC_HIP_FLAG_ORDER_SEARCH on the GPU: candidate records, residual rows, R[] and coefficients equal the model's
(tests/order_model.py) byte for byte; frames equal the model's bytes, are never longer than the REFERENCE_SUM_ORDER
frames and unchanged at lpc_order 1; the flag composes with wasted bits, the host PCM path and the block-size search,
and every flagged path decodes back to its input."""
import numpy as np
import pytest
import torch

import order_model as om
import util
from extreme_signals import check_rows
from flacenc_rs_amd import _capi
from oracle import oracle as orc

pytestmark = pytest.mark.gpu
OS = _capi.FLAG_ORDER_SEARCH
REF = _capi.FLAG_REFERENCE_SUM_ORDER
NIGHTLY = _capi.FLAG_NIGHTLY_SUM_ORDER


@pytest.fixture(scope="module")
def h():
    with _capi.Handle(0) as handle:
        yield handle


def content(n_rows, b, bits=16, start=0, seed=0):
    """Real audio (the golden fixtures, tiled) at `bits` bits -> int32 [n_rows, b]; 24-bit rows get random low bits."""
    names = ("ras103", "ras22", "sus109", "sus6")
    x = np.concatenate([util.test_signal(nm, c) for nm in names for c in (0, 1)]).astype(np.int64)
    total = n_rows * b
    x = np.tile(x, (start + total) // len(x) + 1)[start:start + total].reshape(n_rows, b)
    if bits < 16:
        x >>= 16 - bits
    elif bits > 16:
        rng = np.random.default_rng(seed + b)
        x = (x << (bits - 16)) | rng.integers(0, 1 << (bits - 16), x.shape)
    return x.astype(np.int32)


def gcfg(order, flags=0, **kw):
    return _capi.make_config(lpc_order=order, flags=OS | flags, **kw)


def ocfg(order, nightly=False, finest=False):
    return om.config(order=order, nightly=nightly, rice_finest_only=finest)


BATCH_CASES = [
    # (block, order, bits)
    (64, 8, 16), (100, 12, 16), (256, 8, 8), (1152, 12, 24), (4096, 1, 16), (4096, 2, 16), (4096, 8, 16),
    (4096, 12, 24), (4096, 16, 16), (4096, 32, 24), (4608, 12, 16), (8192, 24, 24), (16384, 16, 16),
    (16384, 32, 24), (20000, 8, 16), (20000, 32, 24),
]


@pytest.mark.parametrize("b,order,bits", BATCH_CASES)
def test_candidate_batch_equals_the_model(h, b, order, bits):
    x = content(6 if b <= 4608 else 3, b, bits, start=b)
    params, residual, R, A = h.qlpc_batch(x, bits, gcfg(order), want_fp=True)
    check_rows(params, residual, R, A, x, bits, ocfg(order), (b, order, bits))


@pytest.mark.parametrize("b,order,flags,finest,nightly", [
    (4096, 8, _capi.FLAG_FINEST_RICE_ORDER, True, False), (1152, 12, _capi.FLAG_FINEST_RICE_ORDER, True, False),
    (4096, 12, NIGHTLY, False, True), (2048, 15, NIGHTLY, False, True), (4096, 8, REF, False, False),
    (4096, 8, _capi.FLAG_CANONICAL_SUM_ORDER, False, False), (4096, 8, REF | _capi.FLAG_INTEGER_PARITY_ONLY, False, False),
])
def test_candidate_batch_under_other_flags(h, b, order, flags, finest, nightly):
    x = content(4, b, 16, start=3 * b)
    params, residual, R, A = h.qlpc_batch(x, 16, gcfg(order, flags), want_fp=True)
    check_rows(params, residual, R, A, x, 16, ocfg(order, nightly=nightly, finest=finest), (b, order, flags))


@pytest.mark.parametrize("b,order,bits", [(4096, 8, 16), (1152, 12, 24), (8192, 32, 24), (256, 8, 8)])
def test_stereo_batch_equals_the_model_with_the_side_channel(h, b, order, bits):
    x = content(6, b, bits, start=5 * b).reshape(3, 2, b)
    params, residual = h.stereo_qlpc_batch(x, bits, gcfg(order))
    cfg = ocfg(order)
    for f in range(3):
        l, r = x[f, 0], x[f, 1]
        m, s = orc.stereo_to_midside(l, r)
        for k, sig in enumerate((l, r, m, s)):
            rec, resid, _, _ = om.record(sig, bits + (1 if k == 3 else 0), cfg)
            p = params[f, k]
            assert int(p["subframe_bits"]) == rec["subframe_bits"] and int(p["order"]) == rec["order"], (f, k)
            assert np.array_equal(residual[f, k], resid), (f, k)


def test_an_ar2_signal_picks_order_2(h):
    rng = np.random.default_rng(7)
    rows = []
    for _ in range(4):
        e = rng.integers(-64, 65, 4096)
        x = np.zeros(4096)
        for t in range(2, 4096):
            x[t] = 1.6 * x[t - 1] - 0.8 * x[t - 2] + e[t]
        rows.append(np.round(x))
    x = np.array(rows, np.int32)
    params, _, _, _ = h.qlpc_batch(x, 16, gcfg(12), want_fp=True)
    assert params["order"].tolist() == [2] * 4


def test_nonpd_plateau_fixture_yields_valid_frames(h):
    x = np.load(util.GOLDEN + "/cert_nonpd_plateau_24bit.npy").astype(np.int32).reshape(-1)
    b = 4096
    n = len(x) // b
    rows = x[: n * b].reshape(n, b)
    params, residual, R, A = h.qlpc_batch(rows, 24, gcfg(12), want_fp=True)
    check_rows(params, residual, R, A, rows, 24, ocfg(12), "nonpd")
    frames = np.stack([rows, rows[::-1]], 1)[: max(1, n)]
    got = gpu_stereo(h, frame_cfg(12), frames, 24)
    decode_check(h, got, frames, 24)


# ---- frames ----
def frame_cfg(order, flags=0, use_fixed=True, stereo=True, search=True):
    qlpc = gcfg(order, flags) if search else _capi.make_config(lpc_order=order, flags=flags)
    return _capi.make_frame_config(qlpc, use_fixed=use_fixed, use_leftside=stereo, use_rightside=stereo,
                                   use_midside=stereo)


def gpu_stereo(h, cfg, x, bps):
    n, _, b = x.shape
    dx = torch.from_numpy(np.ascontiguousarray(x, np.int32)).cuda()
    slot = h.frame_bytes_bound(b, bps)
    out = torch.zeros(n * slot, dtype=torch.uint8, device="cuda")
    ln = torch.zeros(n, dtype=torch.int32, device="cuda")
    res = torch.zeros(n * 752, dtype=torch.uint8, device="cuda")
    h.encode_pack_stereo_frames_device(cfg, dx.data_ptr(), n, b, b, bps, 44100, 0, 1, res.data_ptr(), out.data_ptr(),
                                       slot, ln.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    o, lens = out.cpu().numpy(), ln.cpu().numpy()
    return [o[f * slot:f * slot + lens[f]].tobytes() for f in range(n)]


def gpu_channels(h, cfg, x, bps):
    n, C, b = x.shape
    dx = torch.from_numpy(np.ascontiguousarray(x, np.int32)).cuda()
    slot = h.frame_bytes_bound_channels(C, b, bps)
    out = torch.zeros(n * slot, dtype=torch.uint8, device="cuda")
    ln = torch.zeros(n, dtype=torch.int32, device="cuda")
    res = torch.zeros(n * C * 368, dtype=torch.uint8, device="cuda")
    h.encode_pack_frames_device(cfg, dx.data_ptr(), n, C, b, b, bps, 44100, 0, 1, res.data_ptr(), out.data_ptr(), slot,
                                ln.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    o, lens = out.cpu().numpy(), ln.cpu().numpy()
    return [o[f * slot:f * slot + lens[f]].tobytes() for f in range(n)]


def decode_check(h, frames, x, bps):
    n, C, b = x.shape
    lens = np.array([len(f) for f in frames], np.uint32)
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
    data = b"".join(frames)
    out, _, _, st = h.decode_frames(data, offs, lens, C, bps, b)
    assert st.tolist() == [0] * n
    assert np.array_equal(out[:, :, :b], x)
    assert h.verify_frames(data, offs, lens, C, bps, b, np.ascontiguousarray(x, np.int32)).tolist() == [0] * n


@pytest.mark.parametrize("b,order,bits", [(4096, 8, 16), (4096, 12, 24), (4608, 8, 16), (1152, 12, 16), (8192, 16, 24),
                                          (1000, 8, 16), (40, 8, 16)])
def test_stereo_frame_bytes_equal_the_model(h, b, order, bits):
    x = content(8, b, bits, start=7 * b).reshape(4, 2, b)
    got = gpu_stereo(h, frame_cfg(order), x, bits)
    fc = orc.make_frame_config(ocfg(order))
    for f in range(len(x)):
        assert got[f] == om.stereo_frame_bytes(x[f, 0], x[f, 1], bits, fc, number=f), (b, order, f)
    decode_check(h, got, x, bits)


@pytest.mark.parametrize("C,b,order", [(1, 4096, 8), (3, 1152, 12), (8, 4096, 8)])
def test_independent_frame_bytes_equal_the_model(h, C, b, order):
    x = content(2 * C, b, 16, start=11 * b).reshape(2, C, b)
    got = gpu_channels(h, frame_cfg(order, stereo=False), x, 16)
    fc = orc.make_frame_config(ocfg(order), use_leftside=False, use_rightside=False, use_midside=False)
    for f in range(len(x)):
        assert got[f] == om.channel_frame_bytes(list(x[f]), 16, fc, number=f), (C, b, f)
    decode_check(h, got, x, 16)


@pytest.mark.parametrize("b,order", [(4096, 8), (4096, 12), (1152, 8), (8192, 32), (4608, 12)])
def test_flagged_frames_are_never_longer_and_order_1_changes_nothing(h, b, order):
    x = content(32, b, 16).reshape(16, 2, b)
    plain = gpu_stereo(h, frame_cfg(order, REF, search=False), x, 16)
    got = gpu_stereo(h, frame_cfg(order, REF), x, 16)
    assert all(len(g) <= len(p) for g, p in zip(got, plain))
    plain1 = gpu_stereo(h, frame_cfg(1, REF, search=False), x, 16)
    assert gpu_stereo(h, frame_cfg(1, REF), x, 16) == plain1
    assert gpu_stereo(h, frame_cfg(1), x, 16) == plain1


# ---- compositions ----
def test_with_wasted_bits_equals_the_model_and_decodes(h):
    b = 4096
    x = content(8, b, 16, start=b).reshape(4, 2, b).astype(np.int64)
    x[1] <<= 8
    x[2, 0] <<= 3
    x = x.astype(np.int32)
    got = gpu_stereo(h, frame_cfg(8, _capi.FLAG_WASTED_BITS), x, 24)
    fc = orc.make_frame_config(ocfg(8))
    assert got[0] == om.stereo_frame_bytes(x[0, 0], x[0, 1], 24, fc, number=0)
    for f in range(len(x)):  # (the wasted-bits frames against the composed model)
        assert got[f] == om.wasted_stereo_frame_bytes(x[f, 0], x[f, 1], 24, fc, number=f), f
    decode_check(h, got, x, 24)
    plain = gpu_stereo(h, frame_cfg(8, 0), x, 24)
    assert len(got[1]) < len(plain[1])


@pytest.mark.parametrize("channels", [2, 3])
def test_encode_pcm_from_host_memory_decodes(h, channels):
    b = 4096
    x = content(channels * 3, b, 16, start=2 * b).reshape(channels, 3 * b)
    pcm = np.ascontiguousarray(x.T.astype("<i2")).view(np.uint8).reshape(-1)
    cfg = frame_cfg(8, stereo=channels == 2)
    data, lens = h.encode_pcm(pcm, channels, cfg, 2, 16, b, 44100)
    frames = []
    off = 0
    for ln in lens:
        frames.append(bytes(data[off:off + ln]))
        off += ln
    ref = x.reshape(channels, 3, b).transpose(1, 0, 2)
    if channels == 2:
        assert frames == gpu_stereo(h, cfg, np.ascontiguousarray(ref), 16)
    decode_check(h, frames, np.ascontiguousarray(ref), 16)


def test_encode_variable_decodes_and_is_never_longer(h):
    b = 4096
    x = content(8, b, 16, start=9 * b).reshape(4, 2, b)
    got = h.encode_variable(x, 16, frame_cfg(8), levels=3)
    plain = h.encode_variable(x, 16, frame_cfg(8, REF, search=False), levels=3)
    assert not got["overflow"]
    assert got["bytes"] <= plain["bytes"]
    out, bs, _, st = h.decode_frames(got["data"], got["offsets"], got["lengths"], 2, 16, b)
    assert st.tolist() == [0] * len(got["lengths"])
    pos = 0
    flat = x.transpose(1, 0, 2).reshape(2, -1)
    for f, n in enumerate(bs):
        assert np.array_equal(out[f, :, :n], flat[:, pos:pos + n])
        pos += n
    assert pos == flat.shape[1]


# ---- handle state and refusal ----
def test_flagged_unflagged_flagged_on_one_handle_equals_fresh_handles(h):
    x = content(8, 4096, 16, start=13 * 4096)
    a1 = h.qlpc_batch(x, 16, gcfg(12), want_fp=True)
    u = h.qlpc_batch(x, 16, _capi.make_config(lpc_order=12), want_fp=True)
    a2 = h.qlpc_batch(x, 16, gcfg(12), want_fp=True)
    with _capi.Handle(0) as fresh:
        f1 = fresh.qlpc_batch(x, 16, gcfg(12), want_fp=True)
    with _capi.Handle(0) as fresh:
        fu = fresh.qlpc_batch(x, 16, _capi.make_config(lpc_order=12), want_fp=True)
    for got, ref in ((a1, f1), (a2, f1), (u, fu)):
        assert all(np.array_equal(g, r) for g, r in zip(got, ref))


def test_direct_mse_with_the_flag_is_refused(h):
    x = content(2, 4096, 16)
    with pytest.raises(Exception):
        h.qlpc_batch(x, 16, gcfg(8, use_direct_mse=True))
    with pytest.raises(Exception):
        h.encode_stereo_frames(x.reshape(1, 2, 4096), 16, _capi.make_frame_config(gcfg(8, use_direct_mse=True)))
