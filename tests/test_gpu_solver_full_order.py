"""The fused 4096 / 4608 kernel's solver at and one below each instance's full order, against the CPU oracle.

The wave-per-subframe kernel has one instance per order bucket (MAXP = 8, 10, 12).  At lpc_order == MAXP wave 0 runs the
straight-line form of Levinson-Durbin + quantisation + the certificate's first tier (levinson_quantize_full); at every
other order the generic, guarded form; and a workgroup in which a system leaves the straight line (a zero denominator,
digital silence, a coefficient that is not finite) is solved once more by the generic form.  Both forms must give the
oracle's records, field by field, through every entry point that reaches the kernel:

  qlpc_batch            (plain instances)        R[] and the unquantised coefficients bit for bit, records, residual
  stereo_qlpc_batch     (stereo L, R, M, S)      records and residual per role
  encode_stereo_frames  (the bench's instance)   the frame decision, the chosen records and residual rows
  ... with use_fixed    (fixed-LPC instances)    the same with the fixed-LPC candidate in the kernel

on orders 7 .. 12 (equal to and one below each MAXP), precisions 3, 8 and 15, blocks of 4096 and 4608 samples, and
material that reaches the solver's corners: digital silence (R[0] == 0: the second solve), constant blocks, full-scale
noise, near-pure tones (denominators next to zero, the certificate's second tier), and coefficients that quantise to a
zero tail (the order truncation of lpc.rs:295-299).
"""
import numpy as np
import pytest

import util
from flacenc_rs_amd import _capi
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

BPS = 16
RECORD_FIELDS = ("order", "shift", "precision", "rice_order", "status", "code_bits", "subframe_bits", "sum_quotients")


@pytest.fixture(scope="module")
def handle():
    h = _capi.Handle(0)
    yield h
    h.close()


def gpu_cfg(order, precision):
    return _capi.make_config(lpc_order=order, quant_precision=precision)


def orc_cfg(order, precision):
    return orc.make_config(lpc_order=order, quant_precision=precision, acorr=orc.ACORR_CANONICAL)


def material(n, seed):
    """name -> int32[n], 16-bit.  An even number of signals: consecutive pairs are the stereo frames."""
    lo, hi = -(1 << (BPS - 1)), (1 << (BPS - 1)) - 1
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    ar1 = np.zeros(n)
    e = rng.normal(0.0, 300.0, n)
    for i in range(1, n):
        ar1[i] = 0.9 * ar1[i - 1] + e[i]
    sigs = {
        "silence": np.zeros(n),
        "silence_too": np.zeros(n),                                   # (a frame that is silent in all four roles)
        "constant": np.full(n, 12345),
        "constant_minus_one": np.full(n, -1),
        "constant_full_scale": np.full(n, lo),
        "noise_full_scale": rng.integers(lo, hi + 1, n),
        "noise_full_scale_2": rng.integers(lo, hi + 1, n),
        "noise_small": rng.integers(-40, 41, n),                      # every coefficient near zero: the shift at its clamp of 15
        "tone_pure": util.quantize(util.sine(n, 37.3, 0.98), BPS),
        "tone_period_4": np.round(hi * np.sin(np.pi * t / 2.0 + 0.3)),  # R[] of rank 2: denominators next to zero
        "tone_low": util.quantize(util.sine(n, 1531.0, 0.999), BPS),
        "tone_plus_lsb": util.sine_noise(n, BPS, 61.0, 0.9, 1.5 / 32768, seed=seed + 1),
        "two_tones": util.quantize(util.sine(n, 23.0, 0.45) + util.sine(n, 7.7, 0.45, phase=1.0), BPS),
        "ar1_zero_tail": np.clip(np.round(ar1), lo, hi),              # a = (0.9, ~0, ~0, ...): a zero tail
        "alternation": np.where(t % 2 == 0, hi, lo),
        "impulse": np.where(t == n // 3, hi, 0),
        "half_silent": np.where(t < n // 2, 0, util.quantize(util.noise(seed + 2, n, 0.5), BPS)),
        "music_like": util.sine_noise(n, BPS, 200.0, 0.4, 0.05, seed=seed + 3),
    }
    assert len(sigs) % 2 == 0
    return {k: np.asarray(v).astype(np.int32) for k, v in sigs.items()}


def assert_records_equal(g, o, what):
    for f in RECORD_FIELDS:
        assert np.array_equal(g[f], o[f]), (what, f, g[f].tolist(), o[f].tolist())
    assert np.array_equal(g["coefs"], o["coefs"]), what
    assert np.array_equal(g["rice_params"], o["rice_params"]), what


def check_plain(handle, names, x, order, precision):
    gp, gres, gR, gA = handle.qlpc_batch(x, BPS, gpu_cfg(order, precision), want_fp=True)
    cp, cres, cR, cA = orc.qlpc_batch(x, BPS, orc_cfg(order, precision))
    for k, name in enumerate(names):
        where = ("qlpc_batch", name)
        assert int(gp["status"][k]) == 0, where
        assert np.array_equal(gR[k].view(np.uint64), cR[k].view(np.uint64)), (where, "autocorrelation bits")
        assert np.array_equal(gA[k].view(np.uint64), cA[k].view(np.uint64)), (where, "LPC coefficient bits")
        assert_records_equal(gp[k:k + 1], cp[k:k + 1], where)
        assert np.array_equal(gres[k], cres[k]), where
        p = gp[k]
        o = int(p["order"])
        dec = orc.decode_lpc(x[k][:o], p["coefs"][:o], int(p["shift"]), gres[k])
        assert np.array_equal(dec, x[k]), where
    return cp


def check_stereo_roles(handle, frames, order, precision):
    params, residual = handle.stereo_qlpc_batch(frames, BPS, gpu_cfg(order, precision))
    ocfg = orc_cfg(order, precision)
    for f in range(frames.shape[0]):
        l, r = frames[f, 0], frames[f, 1]
        m, s = orc.stereo_to_midside(l, r)
        for role, (sig, b) in enumerate(((l, BPS), (r, BPS), (m, BPS), (s, BPS + 1))):
            where = ("stereo_qlpc_batch", f, role)
            want = orc.estimated_qlpc(sig, b, ocfg)
            got = params[f, role]
            k = want["order"]
            assert int(got["status"]) == 0, where
            assert (int(got["order"]), int(got["shift"]), int(got["precision"])) == (k, want["shift"], precision), where
            assert got["coefs"][:k].tolist() == want["coefs"].tolist(), where
            assert (got["coefs"][k:] == 0).all(), where
            assert np.array_equal(residual[f, role], want["residual"]), where
            assert int(got["rice_order"]) == want["rice_order"], where
            assert got["rice_params"][: 1 << want["rice_order"]].tolist() == want["rice_params"].tolist(), where
            assert int(got["code_bits"]) == want["code_bits"], where
            assert int(got["subframe_bits"]) == want["subframe_bits"], where


def check_frames(handle, frames, order, precision, use_fixed):
    cfg = _capi.make_frame_config(gpu_cfg(order, precision), use_fixed=use_fixed)
    got, gres = handle.encode_stereo_frames(frames, BPS, cfg)
    if use_fixed:
        ofc = orc.make_frame_config(orc_cfg(order, precision), use_fixed=True,
                                    fixed=orc.make_fixed_config(sum_mode=orc.SUMABS_CANONICAL))
        want, wres = orc.encode_stereo_frames_cfg(frames, BPS, ofc)
    else:
        want, wres = orc.encode_stereo_frames(frames, BPS, orc_cfg(order, precision))
    for f in range(frames.shape[0]):
        g, w = got[f], want[f]
        where = ("encode_stereo_frames", "fixed" if use_fixed else "qlpc", f)
        for fld in ("channel_assignment", "role", "kind", "dc_offset", "bits"):
            assert g[fld].tolist() == w[fld].tolist(), (where, fld, g[fld].tolist(), w[fld].tolist())
        for c in range(2):
            if int(g["kind"][c]) >= 2:
                gl, wl = g["lpc"][c], w["lpc"][c]
                for fld in RECORD_FIELDS:
                    assert int(gl[fld]) == int(wl[fld]), (where, c, fld)
                assert gl["coefs"].tolist() == wl["coefs"].tolist(), (where, c)
                assert gl["rice_params"].tolist() == wl["rice_params"].tolist(), (where, c)
            assert np.array_equal(gres[f, c], wres[f, c]), (where, c)


@pytest.mark.parametrize("n", [4096, 4608])
@pytest.mark.parametrize("precision", [3, 8, 15])
@pytest.mark.parametrize("order", [7, 8, 9, 10, 11, 12])
def test_fused_kernel_solver_equals_oracle(handle, order, precision, n):
    sigs = material(n, seed=1000 * order + 10 * precision + (n != 4096))
    names = list(sigs)
    x = np.stack([sigs[k] for k in names])
    frames = np.ascontiguousarray(x.reshape(len(names) // 2, 2, n))
    cp = check_plain(handle, names, x, order, precision)
    # the material reaches what it is here for (from the oracle's records: nothing of this depends on the GPU)
    rec = {name: cp[k] for k, name in enumerate(names)}
    assert int(rec["silence"]["order"]) == 1 and (rec["silence"]["coefs"] == 0).all() and int(rec["silence"]["shift"]) == 15
    if precision == 3:  # (the tail is estimation noise of ~n^-1/2: below half a step of the coarsest quantiser only)
        assert int(rec["ar1_zero_tail"]["order"]) < order, "a zero tail truncates the order (lpc.rs:295-299)"
    assert int(rec["impulse"]["order"]) == 1 and (rec["impulse"]["coefs"] == 0).all()  # R[0] > 0, every a[i] == 0
    check_stereo_roles(handle, frames, order, precision)
    check_frames(handle, frames, order, precision, use_fixed=False)
    check_frames(handle, frames, order, precision, use_fixed=True)
