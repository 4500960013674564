"""The fused 4096 kernel's window weights from the lane-major table (flacenc_rs_amd/csrc/window_lanes_core.h).

The stereo instances of the wave-per-subframe kernel that run four workgroups per CU read their window weights from a
second copy of the table, stored in the order the lanes read it: slot j holds the quad at 64 lane - 12 + 4 j of every
lane.  A weight taken from the wrong lane or slot changes R[].  Three stereo frames of 4096 samples, seeded noise plus a
tone, at 16 bits and at 24 (the side role then has 25), under

  Tukey(1.0)    every weight distinct, no flat part: any misplaced quad moves R[]
  Tukey(0.4)    the default: tapers over lanes 0..12 and 51..63, exactly 1.0f between
  Tukey(0.005)  a taper of 10 samples on either side: it ends inside lane 0's third quad and begins inside lane 63's
                last but two, everything else reads 1.0f

at orders 7 and 8 (the order-8 instances; 8-sample halo), 10 (the 12-sample halo: slot 0) and 12, through
flacenc_hip_stereo_qlpc_batch (the four-candidate kernel) and flacenc_hip_encode_stereo_frames with and without the
fixed-LPC candidate (the deciding kernels; the instances with the fixed-LPC candidate keep the time-major loads,
profiles/window_lanes_ab.txt, and are held to the same records).  Compared exactly with the oracle: every field of the records and every
residual row.  These entry points hand out no R[]; what ties the kernel's lane-order sums to the oracle's restatement of
them is the order certificate, which both run on those sums: its three counters (analysed, second tier, recomputed from
the reference's chains) must be the oracle's -- a wrong weight fails the certificate, and the fallback, which reads the
time-major table, would otherwise hide it behind correct records.  Plus one rectangle case (no table at all) and one
window-search launch on 4096-sample blocks (its pieces get lane-major copies too; the search itself reads the
time-major ones)."""
import numpy as np
import pytest

import util
import window_model as wm
from flacenc_rs_amd import _capi
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

N = 4096
NF = 3
RECORD_FIELDS = ("order", "shift", "precision", "rice_order", "status", "code_bits", "subframe_bits", "sum_quotients")
WINDOWS = [("tukey", 1.0), ("tukey", 0.4), ("tukey", 0.005)]


@pytest.fixture(scope="module")
def handle():
    h = _capi.Handle(0, hooks=True)  # (the hooks build: the certificate's device counters)
    yield h
    h.close()


_FRAMES = {}


def frames_for(bits):
    """int32 [3, 2, 4096]: a tone plus noise per channel, different in the two, so that no role is trivial"""
    if bits not in _FRAMES:
        fr = [np.stack([util.sine_noise(N, bits, 41.0 + 9 * f, 0.60, 0.03, seed=8100 + f, phase=0.3 * f),
                        util.sine_noise(N, bits, 67.0 + 5 * f, 0.55, 0.05, seed=8200 + f, phase=1.1 + 0.2 * f)])
              for f in range(NF)]
        x = np.stack(fr).astype(np.int32)
        x.setflags(write=False)
        _FRAMES[bits] = x
    return _FRAMES[bits]


def roles_of(frames, bits):
    rows, bps = [], []
    for f in range(frames.shape[0]):
        l, r = frames[f, 0], frames[f, 1]
        m, s = orc.stereo_to_midside(l, r)
        rows += [l, r, m, s]
        bps += [bits, bits, bits, bits + 1]
    return np.stack(rows), np.asarray(bps, np.uint8)


_ORACLE = {}


def oracle_for(window, order, bits):
    """the oracle's records / rows of the twelve roles, its certificate counters on them, and its frames with and
    without the fixed-LPC candidate: once per case, shared, left unchanged"""
    key = (window, order, bits)
    if key not in _ORACLE:
        frames = frames_for(bits)
        x, bps = roles_of(frames, bits)
        if bits == 24:
            assert np.abs(x[3::4].astype(np.int64)).max() >= 1 << 23, "the side role needs its 25th bit"
        cfg = orc.make_config(lpc_order=order, window=window, acorr=orc.ACORR_CANONICAL)
        orc.cert_stats(reset=True)
        cp, cres, _, _ = orc.qlpc_batch(x, bps, cfg, nthreads=1, want_fp=False)
        stats = [int(v) for v in orc.cert_stats()]
        plain = orc.encode_stereo_frames(frames, bits, cfg)
        fixed = orc.encode_stereo_frames_cfg(
            frames, bits, orc.make_frame_config(cfg, use_fixed=True, fixed=orc.make_fixed_config(sum_mode=orc.SUMABS_CANONICAL)))
        _ORACLE[key] = (cp, cres, stats, plain, fixed)
    return _ORACLE[key]


def counted(handle, launch):
    import torch
    stats = torch.zeros(3, dtype=torch.int32, device="cuda")
    handle.debug_set_cert_stats(stats.data_ptr())
    try:
        out = launch()
        torch.cuda.synchronize()
    finally:
        handle.debug_set_cert_stats(0)
    return out, stats.cpu().tolist()


def check_frames(got, gres, want, wres, where):
    for f in range(NF):
        g, w = got[f], want[f]
        for fld in ("channel_assignment", "role", "kind", "dc_offset", "bits"):
            assert g[fld].tolist() == w[fld].tolist(), (where, f, fld, g[fld].tolist(), w[fld].tolist())
        for c in range(2):
            if int(g["kind"][c]) >= 2:
                gl, wl = g["lpc"][c], w["lpc"][c]
                for fld in RECORD_FIELDS:
                    assert int(gl[fld]) == int(wl[fld]), (where, f, c, fld)
                assert gl["coefs"].tolist() == wl["coefs"].tolist(), (where, f, c)
                assert gl["rice_params"].tolist() == wl["rice_params"].tolist(), (where, f, c)
            assert np.array_equal(gres[f, c], wres[f, c]), (where, f, c)


def check_case(handle, window, order, bits):
    frames = frames_for(bits)
    cp, cres, want_stats, (pw, pwres), (fw, fwres) = oracle_for(window, order, bits)
    gcfg = _capi.make_config(lpc_order=order, window=window)
    # the four-candidate entry point: L, R, M, S of every frame
    (params, residual), got_stats = counted(handle, lambda: handle.stereo_qlpc_batch(frames, bits, gcfg))
    gp = params.reshape(-1)
    assert (gp["status"] == 0).all()
    for fld in RECORD_FIELDS + ("coefs", "rice_params"):
        assert np.array_equal(gp[fld], cp[fld]), ("stereo_qlpc_batch", window, order, bits, fld)
    assert np.array_equal(residual.reshape(-1, N), cres)
    print(f"{window} order {order} bits {bits}: certificate counters device {got_stats} oracle {want_stats}")
    assert got_stats == want_stats, ("stereo_qlpc_batch", got_stats, want_stats)
    # the deciding entry point, without and with the fixed-LPC candidate
    (got, gres), got_stats = counted(
        handle, lambda: handle.encode_stereo_frames(frames, bits, _capi.make_frame_config(gcfg, use_fixed=False)))
    check_frames(got, gres, pw, pwres, ("encode_stereo_frames", window, order, bits))
    assert got_stats == want_stats, ("encode_stereo_frames", got_stats, want_stats)
    got, gres = handle.encode_stereo_frames(frames, bits, _capi.make_frame_config(gcfg, use_fixed=True))
    check_frames(got, gres, fw, fwres, ("encode_stereo_frames, fixed", window, order, bits))
    assert {int(k) for k in got["kind"].ravel()} & {3}, "the QLPC candidate is chosen somewhere"


@pytest.mark.parametrize("bits", [16, 24])
@pytest.mark.parametrize("order", [7, 8, 10, 12])
@pytest.mark.parametrize("window", WINDOWS, ids=lambda w: f"tukey{w[1]}")
def test_lane_major_weights_give_the_oracles_records(handle, window, order, bits):
    check_case(handle, window, order, bits)


def test_rectangle_window_has_no_table(handle):
    check_case(handle, "rectangle", 8, 16)
    check_case(handle, "rectangle", 10, 24)


def test_window_search_on_4096_blocks(handle):
    """FLACENC_HIP_FLAG_WINDOW_SEARCH with the default pieces: their entries are built (lane-major copies included) and the
    launch gives the model's choice for every role"""
    bits, order = 16, 8
    frames = frames_for(bits)
    params, residual = handle.stereo_qlpc_batch(frames, bits, _capi.make_config(lpc_order=order, flags=_capi.FLAG_WINDOW_SEARCH))
    cfg = wm.om.config(order=order)
    for f in range(NF):
        m, s = orc.stereo_to_midside(frames[f, 0], frames[f, 1])
        for k, sig in enumerate((frames[f, 0], frames[f, 1], m, s)):
            rec, resid, _, _ = wm.record(sig, bits + (1 if k == 3 else 0), cfg, wm.DEFAULT, False)
            p = params[f, k]
            assert int(p["subframe_bits"]) == rec["subframe_bits"] and int(p["order"]) == rec["order"], (f, k)
            assert np.array_equal(residual[f, k], resid), (f, k)
    # and the plain window right after it on the same handle, its entry long cached
    check_case(handle, ("tukey", 0.4), 8, 16)
