"""FLACENC_HIP_FLAG_WASTED_BITS on the GPU: frame bytes equal the model's (tests/wasted_model.py) on every shape class,
a frame of 16-bit content at 24 bits costs exactly the unary counts more than the content at 16 bits, the flag changes
nothing on material without wasted bits, and every flagged path decodes and verifies back to its input."""
import numpy as np
import pytest
import torch

import util
import wasted_model as wm
from flacenc_rs_amd import _capi

pytestmark = pytest.mark.gpu
W = _capi.FLAG_WASTED_BITS
STEREO_SHAPES = [4096, 4608, 1152, 2048, 8192, 16384, 1000, 40]


@pytest.fixture(scope="module")
def h():
    with _capi.Handle(0) as handle:
        yield handle


def cfg_of(flags=W, use_fixed=True, use_constant=True, stereo=True, order=8):
    return _capi.make_frame_config(_capi.make_config(lpc_order=order, flags=flags), use_fixed=use_fixed,
                                   use_constant=use_constant, use_leftside=stereo, use_rightside=stereo,
                                   use_midside=stereo)


def content(n_frames, channels, b, start=0):
    """16-bit real audio (the golden fixtures, tiled) -> int64 [n_frames, channels, b]."""
    names = ("ras103", "ras22", "sus109", "sus6")
    ch = [np.concatenate([util.test_signal(nm, c % 2) for nm in names]) for c in range(channels)]
    total = n_frames * b
    reps = (start + total) // len(ch[0]) + 1
    x = np.stack([np.tile(c, reps)[start:start + total] for c in ch])
    return x.reshape(channels, n_frames, b).transpose(1, 0, 2).astype(np.int64)


def stereo_cases(b):
    """Frames at 24 bits: no wasted bits, << 8, L / R with different k, only S wasted, M wasted, k = w - 1, silence,
    constants (Constant with use_constant, wasted with it off)."""
    x = content(6, 2, b, start=3 * b)
    l, r = x[:, 0], x[:, 1]
    rng = np.random.default_rng(b)
    top = rng.integers(0, 2, (2, b)) * -(1 << 23)
    frames = [
        (l[0], r[0]),
        (l[1] << 8, r[1] << 8),
        (l[2] << 3, r[2] << 5),
        ((l[3] << 1) | 1, (r[3] << 1) | 1),          # L, R odd; S = 2 (l - r): only S wasted
        ((l[4] << 2) | 1, (r[4] << 2) - 1),           # M = l + r (k >= 1), L / R odd, S = 4 (l - r) + 2
        (top[0], top[1]),                            # k = 23 (L, R), 22 / 23 (M / S)
        (np.zeros(b, np.int64), np.zeros(b, np.int64)),
        (np.full(b, 256), np.full(b, -4)),
        (l[5] << 8, r[5]),                           # mixed k inside one frame
    ]
    return np.stack([np.stack(f) for f in frames]).astype(np.int32)


def gpu_stereo(h, cfg, x, bps, number0=0):
    """encode_pack_stereo_frames_async -> (frame bytes list, results)."""
    n, _, b = x.shape
    dx = torch.from_numpy(np.ascontiguousarray(x, np.int32)).cuda()
    slot = h.frame_bytes_bound(b, bps)
    out = torch.zeros(n * slot, dtype=torch.uint8, device="cuda")
    ln = torch.zeros(n, dtype=torch.int32, device="cuda")
    res = torch.zeros(n * 752, dtype=torch.uint8, device="cuda")
    h.encode_pack_stereo_frames_device(cfg, dx.data_ptr(), n, b, b, bps, 44100, number0, 1, res.data_ptr(),
                                       out.data_ptr(), slot, ln.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    o, lens = out.cpu().numpy(), ln.cpu().numpy()
    return [o[f * slot:f * slot + lens[f]].tobytes() for f in range(n)], res.cpu().numpy().view(_capi.FRAME_RESULT_DTYPE)


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
    return [o[f * slot:f * slot + lens[f]].tobytes() for f in range(n)], res.cpu().numpy().view(_capi.CHANNEL_RESULT_DTYPE)


def decode_check(h, frames, x, bps):
    n, C, b = x.shape
    lens = np.array([len(f) for f in frames], np.uint32)
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
    data = b"".join(frames)
    out, bs, _, st = h.decode_frames(data, offs, lens, C, bps, b)
    assert st.tolist() == [0] * n
    assert np.array_equal(out[:, :, :b], x)
    assert h.verify_frames(data, offs, lens, C, bps, b, np.ascontiguousarray(x, np.int32)).tolist() == [0] * n


CONFIGS = [dict(use_fixed=True, use_constant=True), dict(use_fixed=False, use_constant=False)]


@pytest.mark.parametrize("b", STEREO_SHAPES)
@pytest.mark.parametrize("sw", CONFIGS, ids=["fixed-constant", "nofixed-noconstant"])
def test_stereo_bytes_equal_the_model(h, b, sw):
    x = stereo_cases(b)
    fc = wm.frame_config(order=8, **sw)
    got, res = gpu_stereo(h, cfg_of(**sw), x, 24)
    for f in range(len(x)):
        assert got[f] == wm.stereo_frame_bytes(x[f, 0], x[f, 1], 24, fc, number=f), (b, f)
    if b >= 64:
        assert _capi.wasted_bits(res)[1].tolist() != [0, 0]  # (the << 8 frame)
    decode_check(h, got, x, 24)


@pytest.mark.parametrize("b", [4096, 1152])
@pytest.mark.parametrize("shift,bps", [(4, 20), (1, 16)])
def test_stereo_narrower_widths_equal_the_model(h, b, shift, bps):
    x = content(3, 2, b) >> (16 + shift - bps)  # (content that fits bps bits once shifted)
    x[1] <<= shift
    x[2, 0] <<= shift
    fc = wm.frame_config(order=8)
    got, _ = gpu_stereo(h, cfg_of(), x, bps)
    for f in range(len(x)):
        assert got[f] == wm.stereo_frame_bytes(x[f, 0], x[f, 1], bps, fc, number=f), (b, f)


@pytest.mark.parametrize("C", [1, 3, 8])
@pytest.mark.parametrize("b", [4096, 1152, 1000])
def test_independent_bytes_equal_the_model(h, C, b):
    x = content(3, C, b) << 4
    for c in range(C):
        x[0, c] = (x[0, c] >> 4) << (c % 5)             # a different k per channel, k = 0 included
    x[1, 0] = 0
    fc = wm.frame_config(order=8, stereo=False)
    got, res = gpu_channels(h, cfg_of(stereo=False), x, 20)
    for f in range(len(x)):
        assert got[f] == wm.channel_frame_bytes(list(x[f]), 20, fc, number=f), (C, b, f)
    assert _capi.wasted_bits(res).reshape(3, C)[2].tolist() == [4] * C
    decode_check(h, got, x, 20)


@pytest.mark.parametrize("b", [4096, 4608, 1152, 8192, 1000])
def test_content_at_24_bits_costs_exactly_the_unary_counts(h, b):
    x = content(4, 2, b) | 1  # odd samples everywhere: no wasted bits, no constant block
    plain, _ = gpu_stereo(h, cfg_of(flags=0, stereo=False), x, 16)
    wide, res = gpu_stereo(h, cfg_of(stereo=False), x << 8, 24)
    assert [len(w) - len(p) for w, p in zip(wide, plain)] == [2] * len(x)
    assert _capi.wasted_bits(res).tolist() == [[8, 8]] * len(x)


REF_IPO = _capi.FLAG_REFERENCE_SUM_ORDER | _capi.FLAG_INTEGER_PARITY_ONLY


@pytest.mark.parametrize("b", [4096, 1152, 8192, 1000])
@pytest.mark.parametrize("extra", [REF_IPO, _capi.FLAG_REFERENCE_SUM_ORDER], ids=["reference-integer-parity", "reference"])
def test_stereo_bytes_equal_the_model_with_reference_order(h, b, extra):
    """The fix-up re-analyses the shifted rows with the caller's other flags: under the drop-ins' summation-order flags
    the mixed-k frames are still the model's (the oracle's sums are the stable build's)."""
    x = stereo_cases(b)
    fc = wm.frame_config(order=8)
    got, _ = gpu_stereo(h, cfg_of(flags=W | extra), x, 24)
    for f in range(len(x)):
        assert got[f] == wm.stereo_frame_bytes(x[f, 0], x[f, 1], 24, fc, number=f), (b, f)


@pytest.mark.parametrize("b", [4096, 1152, 8192, 1000])
@pytest.mark.parametrize("extra", [REF_IPO, _capi.FLAG_NIGHTLY_SUM_ORDER, _capi.FLAG_FINEST_RICE_ORDER],
                         ids=["reference-integer-parity", "nightly", "finest-rice"])
def test_other_flags_cost_exactly_the_unary_counts(h, b, extra):
    """Under each other flag the shifted rows give the first pass's integers: X << 8 at 24 bits with the flag is X at
    16 bits without it plus 8 unary bits per subframe, frame by frame (stereo modes off, odd samples everywhere)."""
    x = content(4, 2, b) | 1
    plain, _ = gpu_stereo(h, cfg_of(flags=extra, stereo=False), x, 16)
    wide, res = gpu_stereo(h, cfg_of(flags=W | extra, stereo=False), x << 8, 24)
    assert [len(w) - len(p) for w, p in zip(wide, plain)] == [2] * len(x)
    assert _capi.wasted_bits(res).tolist() == [[8, 8]] * len(x)


def test_destroy_frees_the_fix_up_scratch():
    """A handle that ran the fix-up gives all its device memory back when it is destroyed."""
    b, n = 4096, 2048
    x = torch.from_numpy(np.ascontiguousarray(np.tile(content(8, 2, b) << 8, (n // 8, 1, 1)), np.int32)).cuda()
    slot = 0
    with _capi.Handle(0) as probe:
        slot = probe.frame_bytes_bound(b, 24)
    out = torch.empty(n * slot, dtype=torch.uint8, device="cuda")
    ln = torch.zeros(n, dtype=torch.int32, device="cuda")
    res = torch.empty(n * 752, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for _ in range(3):
        with _capi.Handle(0) as hh:
            hh.encode_pack_stereo_frames_device(cfg_of(), x.data_ptr(), n, b, b, 24, 44100, 0, 1, res.data_ptr(),
                                                out.data_ptr(), slot, ln.data_ptr(),
                                                torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
    free1 = torch.cuda.mem_get_info()[0]
    shifted_rows = n * 4 * b * 4  # one call's shifted rows alone (each call holds three such buffers)
    assert free0 - free1 < shifted_rows, (free0, free1)


@pytest.mark.parametrize("b", STEREO_SHAPES)
def test_flag_is_a_no_op_on_ordinary_material(h, b):
    x = content(4, 2, b)  # real audio: every role has odd samples
    off, res_off = gpu_stereo(h, cfg_of(flags=0), x, 16)
    on, res_on = gpu_stereo(h, cfg_of(), x, 16)
    assert on == off
    assert res_on.tobytes() == res_off.tobytes()
    xc = content(2, 3, b)
    off_c, cres_off = gpu_channels(h, cfg_of(flags=0, stereo=False), xc, 16)
    on_c, cres_on = gpu_channels(h, cfg_of(stereo=False), xc, 16)
    assert on_c == off_c
    assert cres_on.tobytes() == cres_off.tobytes()


@pytest.mark.parametrize("b", [4096, 1152, 8192, 1000])
def test_flag_off_writes_zero_pad(h, b):
    x = torch.from_numpy(np.ascontiguousarray(content(3, 2, b) << 8, np.int32)).cuda()
    res = torch.full((3 * 752,), 0xAB, dtype=torch.uint8, device="cuda")
    resid = torch.zeros(3 * 2 * b, dtype=torch.int32, device="cuda")
    h.encode_stereo_frames_device(cfg_of(flags=0), x.data_ptr(), 3, b, b, 24, res.data_ptr(), resid.data_ptr(), b,
                                  torch.cuda.current_stream().cuda_stream)
    xc = torch.from_numpy(np.ascontiguousarray(content(2, 3, b) << 8, np.int32)).cuda()
    cres = torch.full((6 * 368,), 0xAB, dtype=torch.uint8, device="cuda")
    cresid = torch.zeros(6 * b, dtype=torch.int32, device="cuda")
    h.encode_frames_device(cfg_of(flags=0, stereo=False), xc.data_ptr(), 2, 3, b, b, 24, cres.data_ptr(),
                           cresid.data_ptr(), b, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert _capi.wasted_bits(res.cpu().numpy().view(_capi.FRAME_RESULT_DTYPE)).tolist() == [[0, 0]] * 3
    assert _capi.wasted_bits(cres.cpu().numpy().view(_capi.CHANNEL_RESULT_DTYPE)).tolist() == [0] * 6


def pcm24(x):
    """int [n, channels] -> packed little-endian 24-bit bytes."""
    v = np.ascontiguousarray(x, np.int32).reshape(-1).view(np.uint8).reshape(-1, 4)[:, :3]
    return np.ascontiguousarray(v).reshape(-1)


@pytest.mark.parametrize("channels", [2, 3])
def test_encode_pcm_round_trip(h, channels):
    b = 4096
    total = 5 * b + 777
    x = content(6, channels, b).transpose(1, 0, 2).reshape(channels, -1)[:, :total]
    x[:, : 2 * b] <<= 8  # two frames with wasted bits, the rest (real audio) without
    pcm = pcm24(x.T)
    cfg = cfg_of(stereo=channels == 2)
    if channels == 2:
        data, lens = h.encode_pcm_stereo(pcm, cfg, 3, 24, b, 44100)
    else:
        data, lens = h.encode_pcm(pcm, channels, cfg, 3, 24, b, 44100)
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
    out, bs, _, st = h.decode_frames(data, offs, lens, channels, 24, b)
    assert st.tolist() == [0] * len(lens)
    got = np.concatenate([out[f, :, :bs[f]] for f in range(len(lens))], axis=1)
    assert np.array_equal(got, x)
    plain, plens = (h.encode_pcm_stereo(pcm, cfg_of(flags=0), 3, 24, b, 44100) if channels == 2 else
                    h.encode_pcm(pcm, channels, cfg_of(flags=0, stereo=False), 3, 24, b, 44100))
    assert lens[0] < plens[0] and list(lens[2:]) == list(plens[2:])


@pytest.mark.parametrize("levels", [1, 2, 3])
def test_encode_variable_round_trip(h, levels):
    S = 4096
    x = content(3, 2, S)
    x[0] <<= 8
    x[1, :, : S // 2] <<= 8  # wasted bits in half of a superblock
    r = h.encode_variable(x, 24, cfg_of(), levels)
    assert not r["overflow"]
    n = r["frames"]
    out, bs, _, st = h.decode_frames(r["data"], r["offsets"], r["lengths"], 2, 24, S)
    assert st.tolist() == [0] * n
    xs = x.transpose(1, 0, 2).reshape(2, -1)
    got = np.concatenate([out[f, :, :bs[f]] for f in range(n)], axis=1)
    assert np.array_equal(got, xs)
    want = np.zeros((n, 2, S), np.int32)
    starts = np.concatenate([[0], np.cumsum(bs.astype(np.int64))[:-1]])
    for f in range(n):
        o, k = int(starts[f]), int(bs[f])
        want[f, :, :k] = xs[:, o:o + k]
    assert h.verify_frames(r["data"], r["offsets"], r["lengths"], 2, 24, S, want).tolist() == [0] * n


def late_break_cases(b):
    """Stereo frames at 24 bits whose samples are all multiples of 2^k except one odd sample, at index 64, 65 or
    n - 1, in L only (L, M and S break late), in R only (R, M and S), or in L and R both (L, R and M; S keeps its wasted
    bits -- a break in S alone is impossible): the wasted-bits scan must not stop early."""
    x = content(1, 2, b, start=5 * b)[0] << 4
    frames = []
    for t in sorted({min(64, b - 1), min(65, b - 1), b - 1}):
        for where in ("L", "R", "LR"):
            l, r = x[0].copy(), x[1].copy()
            if "L" in where:
                l[t] |= 1
            if "R" in where:
                r[t] |= 1
            frames.append((l, r))
    return np.stack([np.stack(f) for f in frames]).astype(np.int32)


@pytest.mark.parametrize("b", STEREO_SHAPES)
def test_one_late_odd_sample_equals_the_model(h, b):
    x = late_break_cases(b)
    fc = wm.frame_config(order=8)
    got, _ = gpu_stereo(h, cfg_of(), x, 24)
    for f in range(len(x)):
        assert got[f] == wm.stereo_frame_bytes(x[f, 0], x[f, 1], 24, fc, number=f), (b, f)
    decode_check(h, got, x, 24)


def test_frame_lengths_agree_with_the_packer(h):
    b = 4096
    x = stereo_cases(b)
    frames, res = gpu_stereo(h, cfg_of(), x, 24)
    dres = torch.from_numpy(res.view(np.uint8).copy()).cuda()
    ln = torch.zeros(len(x), dtype=torch.int32, device="cuda")
    h.stereo_frame_lengths_device(dres.data_ptr(), len(x), b, 24, 44100, 0, 1, ln.data_ptr(),
                                  torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert ln.cpu().numpy().tolist() == [len(f) for f in frames]


def test_candidate_batches_reject_the_flag(h):
    x = content(1, 2, 4096).astype(np.int32)
    with pytest.raises(_capi.FlacencHipError) as e:
        h.qlpc_batch(x[0], np.full(2, 16, np.uint8), _capi.make_config(lpc_order=8, flags=W))
    assert e.value.code == _capi.ERR_UNSUPPORTED
    with pytest.raises(_capi.FlacencHipError) as e:
        h.stereo_qlpc_batch(x, 16, _capi.make_config(lpc_order=8, flags=W))
    assert e.value.code == _capi.ERR_UNSUPPORTED
    with pytest.raises(_capi.FlacencHipError) as e:
        h.fixed_lpc_batch(x, 16, cfg_of(), stereo=True)
    assert e.value.code == _capi.ERR_UNSUPPORTED
