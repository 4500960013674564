"""FLACENC_HIP_FLAG_WINDOW_SEARCH on the GPU: candidate records, residual rows, R[] and coefficients equal the model's
(tests/window_model.py) byte for byte for 0 .. 7 extra windows, with and without the order search; frames equal the model's
bytes, decode back to their input and are never longer than the REFERENCE_SUM_ORDER (or ORDER_SEARCH) frames; with no
extra window every output is that call's; the handle's list behaves as state should; big calls run in slices."""
import numpy as np
import pytest
import torch

import extreme_signals as es
import util
import window_model as wm
from extreme_signals import alternation, extreme_frames, noise
from flacenc_rs_amd import _capi
from oracle import oracle as orc
from test_gpu_order_search import content, decode_check, gpu_channels, gpu_stereo

pytestmark = pytest.mark.gpu
WS = _capi.FLAG_WINDOW_SEARCH
OS = _capi.FLAG_ORDER_SEARCH
REF = _capi.FLAG_REFERENCE_SUM_ORDER
NIGHTLY = _capi.FLAG_NIGHTLY_SUM_ORDER
FINEST = _capi.FLAG_FINEST_RICE_ORDER

E0 = ()
E1 = ((wm.PARTIAL_TUKEY, 0.5, 0, 32768),)
E2 = ((wm.RECTANGLE, 0.0, 0, 0), (wm.TUKEY, 0.1, 0, 0))
E5 = wm.DEFAULT
E7 = wm.DEFAULT + ((wm.PARTIAL_TUKEY, 1.0, 16384, 49152), (wm.PUNCHOUT_TUKEY, 0.0, 100, 65000))
LISTS = {"E0": E0, "E1": E1, "E2": E2, "E5": E5, "E7": E7}


@pytest.fixture(scope="module")
def h():
    with _capi.Handle(0) as handle:
        yield handle


def gcfg(order, flags=0, **kw):
    return _capi.make_config(lpc_order=order, flags=WS | flags, **kw)


def ocfg(order, nightly=False, finest=False):
    return wm.om.config(order=order, nightly=nightly, rice_finest_only=finest)


def with_silence(x):
    """The rows with their first half (rounded to the rows' parity) digital silence: whole pieces of zeros."""
    x = x.copy()
    x[::2, : x.shape[1] // 2] = 0
    x[1::2, : x.shape[1] // 3] = 0
    return x


def check_rows(params, residual, R, A, x, bps, cfg, extras, orders, where):
    es.check_rows(params, residual, R, A, x, bps, cfg, where, es.window_record(extras, orders))


BATCH_CASES = [
    # (block, order, bits, list, order search, material)
    (64, 8, 16, "E5", False, "music"), (100, 12, 16, "E7", True, "silence"), (256, 8, 8, "E2", False, "music"),
    (1152, 12, 24, "E5", True, "music"), (1152, 8, 16, "E1", False, "silence"), (4096, 1, 16, "E5", False, "music"),
    (4096, 8, 16, "E5", False, "silence"), (4096, 8, 16, "E7", True, "music"), (4096, 12, 24, "E5", False, "music"),
    (4096, 16, 16, "E2", True, "music"), (4096, 32, 24, "E5", False, "music"), (4096, 8, 16, "E0", True, "music"),
    (4096, 12, 16, "E0", False, "music"), (4608, 12, 16, "E1", False, "music"), (8192, 16, 24, "E5", True, "silence"),
    (16384, 32, 24, "E2", False, "music"), (20000, 8, 16, "E5", False, "music"), (20000, 32, 24, "E7", False, "music"),
    (4096, 32, 16, "E5", False, "extreme"), (1152, 24, 24, "E7", False, "extreme"),
]


def material(kind, rows, b, bits, start):
    if kind == "extreme":
        x = np.stack([alternation(b, bits), noise(b, bits, 3), np.zeros(b, np.int64),
                      np.r_[np.zeros(b // 2), alternation(b - b // 2, bits)]])
        return x[:rows].astype(np.int32)
    x = content(rows, b, bits, start=start)
    return with_silence(x) if kind == "silence" else x


@pytest.mark.parametrize("b,order,bits,lst,orders,kind", BATCH_CASES)
def test_candidate_batch_equals_the_model(h, b, order, bits, lst, orders, kind):
    extras = LISTS[lst]
    h.set_lpc_windows(extras)
    try:
        x = material(kind, 4 if b <= 4608 else 2, b, bits, 3 * b)
        params, residual, R, A = h.qlpc_batch(x, bits, gcfg(order, OS if orders else 0), want_fp=True)
        check_rows(params, residual, R, A, x, bits, ocfg(order), extras, orders, (b, order, bits, lst, orders, kind))
    finally:
        h.set_lpc_windows(wm.DEFAULT)


@pytest.mark.parametrize("b,order,flags,finest,nightly,orders", [
    (4096, 8, FINEST, True, False, False), (1152, 12, FINEST, True, False, True), (4096, 12, NIGHTLY, False, True, False),
    (2048, 15, NIGHTLY, False, True, True), (4096, 8, REF, False, False, False),
    (4096, 8, _capi.FLAG_CANONICAL_SUM_ORDER, False, False, False),
    (4096, 8, REF | _capi.FLAG_INTEGER_PARITY_ONLY, False, False, False),
])
def test_candidate_batch_under_other_flags(h, b, order, flags, finest, nightly, orders):
    x = content(4, b, 16, start=5 * b)
    params, residual, R, A = h.qlpc_batch(x, 16, gcfg(order, flags | (OS if orders else 0)), want_fp=True)
    check_rows(params, residual, R, A, x, 16, ocfg(order, nightly=nightly, finest=finest), wm.DEFAULT, orders,
               (b, order, flags))


@pytest.mark.parametrize("b,order,bits,orders", [(4096, 8, 16, False), (1152, 12, 24, True), (8192, 32, 24, False)])
def test_stereo_batch_equals_the_model_with_the_side_channel(h, b, order, bits, orders):
    x = with_silence(content(4, b, bits, start=7 * b)).reshape(2, 2, b)
    params, residual = h.stereo_qlpc_batch(x, bits, gcfg(order, OS if orders else 0))
    cfg = ocfg(order)
    for f in range(len(x)):
        m, s = orc.stereo_to_midside(x[f, 0], x[f, 1])
        for k, sig in enumerate((x[f, 0], x[f, 1], m, s)):
            rec, resid, _, _ = wm.record(sig, bits + (1 if k == 3 else 0), cfg, wm.DEFAULT, orders)
            p = params[f, k]
            assert int(p["subframe_bits"]) == rec["subframe_bits"] and int(p["order"]) == rec["order"], (f, k)
            assert np.array_equal(residual[f, k], resid), (f, k)


# ---- frames ----
def frame_cfg(order, flags=0, use_fixed=True, stereo=True, search=True):
    qlpc = gcfg(order, flags) if search else _capi.make_config(lpc_order=order, flags=flags)
    return _capi.make_frame_config(qlpc, use_fixed=use_fixed, use_leftside=stereo, use_rightside=stereo,
                                   use_midside=stereo)


def ofc(order, stereo=True):
    return orc.make_frame_config(ocfg(order), use_leftside=stereo, use_rightside=stereo, use_midside=stereo)


@pytest.mark.parametrize("b,order,bits,orders", [(4096, 8, 16, False), (4096, 12, 24, True), (4608, 8, 16, False),
                                                 (1152, 12, 16, False), (8192, 16, 24, False), (1000, 8, 16, True),
                                                 (40, 8, 16, False)])
def test_stereo_frame_bytes_equal_the_model(h, b, order, bits, orders):
    x = with_silence(content(6, b, bits, start=9 * b)).reshape(3, 2, b)
    got = gpu_stereo(h, frame_cfg(order, OS if orders else 0), x, bits)
    model = wm.Model(wm.DEFAULT, orders)
    for f in range(len(x)):
        assert got[f] == model.stereo_frame_bytes(x[f, 0], x[f, 1], bits, ofc(order), number=f), (b, order, f)
    decode_check(h, got, x, bits)


@pytest.mark.parametrize("C,b,order", [(1, 4096, 8), (3, 1152, 12), (8, 4096, 8)])
def test_independent_frame_bytes_equal_the_model(h, C, b, order):
    x = content(2 * C, b, 16, start=11 * b).reshape(2, C, b)
    got = gpu_channels(h, frame_cfg(order, stereo=False), x, 16)
    model = wm.Model()
    for f in range(len(x)):
        assert got[f] == model.channel_frame_bytes(list(x[f]), 16, ofc(order, stereo=False), number=f), (C, b, f)
    decode_check(h, got, x, 16)


def test_extreme_frames_equal_the_model_and_decode(h):
    x = extreme_frames(np.random.default_rng(11), 1152, 16)[:4]
    got = gpu_stereo(h, frame_cfg(12), x, 16)
    model = wm.Model()
    for f in range(len(x)):
        assert got[f] == model.stereo_frame_bytes(x[f, 0], x[f, 1], 16, ofc(12), number=f), f
    decode_check(h, got, x, 16)


def test_with_wasted_bits_equals_the_model_and_decodes(h):
    b = 4096
    x = content(8, b, 16, start=b).reshape(4, 2, b).astype(np.int64) << 8  # 16-bit content in a 24-bit container
    x[2, 0] >>= 5
    x = x.astype(np.int32)
    for orders in (False, True):
        got = gpu_stereo(h, frame_cfg(8, _capi.FLAG_WASTED_BITS | (OS if orders else 0)), x, 24)
        model = wm.Model(wm.DEFAULT, orders)
        for f in range(len(x)):
            assert got[f] == model.wasted_stereo_frame_bytes(x[f, 0], x[f, 1], 24, ofc(8), number=f), (orders, f)
        decode_check(h, got, x, 24)


def test_encode_pcm_stereo_equals_the_device_call_and_decodes(h):
    b = 4096
    x = content(6, b, 16, start=2 * b).reshape(2, 3 * b)
    pcm = np.ascontiguousarray(x.T.astype("<i2")).view(np.uint8).reshape(-1)
    cfg = frame_cfg(8)
    data, lens = h.encode_pcm(pcm, 2, cfg, 2, 16, b, 44100)
    frames, off = [], 0
    for ln in lens:
        frames.append(bytes(data[off:off + ln]))
        off += ln
    ref = np.ascontiguousarray(x.reshape(2, 3, b).transpose(1, 0, 2))
    assert frames == gpu_stereo(h, cfg, ref, 16)
    model = wm.Model()
    assert frames[0] == model.stereo_frame_bytes(ref[0, 0], ref[0, 1], 16, ofc(8), number=0)
    decode_check(h, frames, ref, 16)


@pytest.mark.parametrize("levels", [1, 2])
def test_encode_variable_decodes_and_is_never_longer(h, levels):
    b = 4096
    x = content(8, b, 16, start=9 * b).reshape(4, 2, b)
    got = h.encode_variable(x, 16, frame_cfg(8), levels=levels)
    plain = h.encode_variable(x, 16, frame_cfg(8, REF, search=False), levels=levels)
    assert not got["overflow"] and got["bytes"] <= plain["bytes"]
    out, bs, _, st = h.decode_frames(got["data"], got["offsets"], got["lengths"], 2, 16, b)
    assert st.tolist() == [0] * len(got["lengths"])
    flat, pos = x.transpose(1, 0, 2).reshape(2, -1), 0
    for f, n in enumerate(bs):
        assert np.array_equal(out[f, :, :n], flat[:, pos:pos + n])
        pos += n
    assert pos == flat.shape[1]


# ---- never longer; zero extra windows ----
@pytest.mark.parametrize("b,order", [(4096, 8), (4096, 12), (1152, 8), (8192, 32), (4608, 12)])
def test_flagged_frames_are_never_longer(h, b, order):
    x = content(32, b, 16).reshape(16, 2, b)
    plain = gpu_stereo(h, frame_cfg(order, REF, search=False), x, 16)
    got = gpu_stereo(h, frame_cfg(order), x, 16)
    assert all(len(g) <= len(p) for g, p in zip(got, plain))
    os_only = gpu_stereo(h, frame_cfg(order, OS, search=False), x, 16)
    both = gpu_stereo(h, frame_cfg(order, OS), x, 16)
    assert all(len(g) <= len(p) for g, p in zip(both, os_only))
    if order == 32:
        assert sum(map(len, got)) < sum(map(len, plain))


@pytest.mark.parametrize("flags", [0, NIGHTLY, FINEST, _capi.FLAG_CANONICAL_SUM_ORDER, OS, OS | NIGHTLY])
def test_zero_extra_windows_is_the_summation_order_call(h, flags):
    b, order = 4096, 12
    x = content(8, b, 16, start=13 * b)
    in_place = flags & ~_capi.FLAG_CANONICAL_SUM_ORDER
    if not flags & (OS | NIGHTLY):
        in_place |= REF
    with _capi.Handle(0) as h0:
        h0.set_lpc_windows([])
        got = h0.qlpc_batch(x, 16, gcfg(order, flags), want_fp=True)
        ref = h0.qlpc_batch(x, 16, _capi.make_config(lpc_order=order, flags=in_place), want_fp=True)
        assert all(np.array_equal(g, r) for g, r in zip(got, ref))
        fr = x.reshape(4, 2, b)
        assert gpu_stereo(h0, frame_cfg(order, flags), fr, 16) == \
            gpu_stereo(h0, frame_cfg(order, in_place, search=False), fr, 16)
        assert gpu_channels(h0, frame_cfg(order, flags, stereo=False), fr, 16) == \
            gpu_channels(h0, frame_cfg(order, in_place, stereo=False, search=False), fr, 16)


# ---- handle state ----
def test_handle_state(h):
    x = with_silence(content(4, 1152, 16, start=17 * 1152))
    cfg, oc = gcfg(12), ocfg(12)
    A_, B_ = E2, E7

    def check(handle, extras, where):
        got = handle.qlpc_batch(x, 16, cfg, want_fp=True)
        check_rows(*got, x, 16, oc, extras, False, where)
        return got

    with _capi.Handle(0) as fresh, _capi.Handle(0) as other:
        d = check(fresh, wm.DEFAULT, "fresh")
        fresh.set_lpc_windows(A_)
        a1 = check(fresh, A_, "A")
        other.set_lpc_windows(B_)
        check(other, B_, "other B")
        fresh.set_lpc_windows(B_)
        check(fresh, B_, "B")
        fresh.set_lpc_windows(A_)
        a2 = check(fresh, A_, "A again")
        assert all(np.array_equal(p, q) for p, q in zip(a1, a2))
        check(other, B_, "other still B")
        # a rejected setter changes nothing
        for bad in ([(9, 0.2, 0, 10)], [(2, 1.5, 0, 10)], [(2, 0.2, 10, 10)], [(3, 0.2, 0, 70000)], list(E7) + [E1[0]]):
            with pytest.raises(_capi.FlacencHipError):
                fresh.set_lpc_windows(bad)
        check(fresh, A_, "after rejections")
        # a list without the flag changes no byte
        u = fresh.qlpc_batch(x, 16, _capi.make_config(lpc_order=12), want_fp=True)
        uf = fresh.qlpc_batch(x, 16, _capi.make_config(lpc_order=12, flags=REF | OS), want_fp=True)
        fr = content(8, 4096, 16).reshape(4, 2, 4096)
        ustereo = gpu_stereo(fresh, frame_cfg(8, search=False), fr, 16)
    with _capi.Handle(0) as plain:
        assert all(np.array_equal(p, q) for p, q in zip(u, plain.qlpc_batch(x, 16, _capi.make_config(lpc_order=12),
                                                                            want_fp=True)))
        assert all(np.array_equal(p, q) for p, q in zip(uf, plain.qlpc_batch(
            x, 16, _capi.make_config(lpc_order=12, flags=REF | OS), want_fp=True)))
        assert ustereo == gpu_stereo(plain, frame_cfg(8, search=False), fr, 16)
    assert all(np.array_equal(p, q) for p, q in zip(d, h.qlpc_batch(x, 16, cfg, want_fp=True)))


def test_direct_mse_with_the_flag_is_refused(h):
    x = content(2, 4096, 16)
    with pytest.raises(_capi.FlacencHipError):
        h.qlpc_batch(x, 16, gcfg(8, use_direct_mse=True))
    with pytest.raises(_capi.FlacencHipError):
        h.encode_stereo_frames(x.reshape(1, 2, 4096), 16, _capi.make_frame_config(gcfg(8, use_direct_mse=True)))


def test_fixed_lpc_batch_ignores_the_flag(h):
    x = content(4, 4096, 16)
    fc = _capi.make_frame_config(_capi.make_config(lpc_order=8))
    got = h.fixed_lpc_batch(x, 16, _capi.make_frame_config(gcfg(8)))
    ref = h.fixed_lpc_batch(x, 16, fc)
    assert all(np.array_equal(g, r) for g, r in zip(got, ref))


# ---- slices and memory ----
def test_a_call_past_the_scratch_bound_runs_in_slices(h):
    b, order, rows = 1152, 32, 30000
    extras = E7  # W = 8 with the order search at P = 32: 256 candidates, about 39 KB of scratch per subframe
    assert rows * (8 * 264 + 8 * 32 * 144 + 4) > 1 << 30
    x = content(rows, b, 16, start=0)
    cfg = gcfg(order, OS)
    with _capi.Handle(0) as big:
        big.set_lpc_windows(extras)
        params, residual, R, A = big.qlpc_batch(x, 16, cfg, want_fp=True)
        # the same rows through small calls
        for lo in (0, 13000, 27520, rows - 256):
            p2, r2, R2, A2 = big.qlpc_batch(x[lo:lo + 256], 16, cfg, want_fp=True)
            assert np.array_equal(params[lo:lo + 256], p2) and np.array_equal(residual[lo:lo + 256], r2), lo
            assert np.array_equal(R[lo:lo + 256], R2) and np.array_equal(A[lo:lo + 256], A2), lo
    # the subframes around the first slice boundary against the model (the slice holds a multiple of 4 subframes)
    per = 8 * 264 + 8 * 32 * 144 + 4
    edge = ((768 << 20) // per) & ~3
    idx = [edge - 1, edge, rows - 1]
    check_rows(params[idx], residual[idx], R[idx], A[idx], x[idx], 16, ocfg(order), extras, True, "slice edge")


def test_device_memory_comes_back_after_destroy():
    """Handles that ran the search, extra windows' weights included, give all their device memory back."""
    rows, b = 4096, 4096
    x = content(rows, b, 16)
    scratch = rows * (8 * 264 + 8 * 12 * 144 + 4)  # one call's search scratch (W = 8, order search at P = 12)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for _ in range(3):
        with _capi.Handle(0) as hh:
            hh.set_lpc_windows(E7)
            hh.qlpc_batch(x, 16, gcfg(12, OS))
            torch.cuda.synchronize()
    free1 = torch.cuda.mem_get_info()[0]
    assert free0 - free1 < scratch, (free0, free1)
