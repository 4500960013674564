"""The fused 4096 kernel's lane-parallel quantise-and-certify step (levinson_phase_lanes) against the CPU oracle.

At lpc_order == 8 the order-8 instances of the wave-per-subframe kernel run the recursion on four lanes of wave 0 and
then quantise and certify one coefficient per lane: max |a|, the order and the certificate's verdict are formed across
lanes (a butterfly maximum, two ballots) where one lane used to walk its system.  Small launches, eight stereo frames of
4096 samples, whose content is built so that each of these happens inside the launch -- and the oracle alone says that
it does (the asserts of `content`, nothing of them depends on the GPU):

  four_orders    the four roles L, R, M, S quantise to four different orders.  Impulse groups 64 samples apart leave R[k]
                 exactly zero except at the lags of their partners: lag 5 strongly in both channels (it cancels in S),
                 lags 6, 7, 8 ever more weakly in the left channel only, so that the part of them that survives the
                 dilution by the lag-5 energy -- all in S, half in L, a fifth in M, none in R -- ends at a different
                 trailing zero in each role.  The amplitudes follow the quantiser's step: one frame per precision.
  clamp_hi       pairs of equal impulses 8 apart inside the window's flat part: a[7] = R[8] / R[0] = 0.5 exactly, which
                 quantises to 2^(precision-1), one above hi; max |a| is a power of two, where no certificate holds: the
                 role is recomputed from the reference's chains
  silence        L == R: the side role is digital silence (R[0] == 0: the second solve through the generic code -- of the
                 workgroup's four systems)
  near_pure,     Sine + Noise(5e-4), a pure sine, two sines: the first tier cannot certify, the rows of T^-1 are
  tones          evaluated; they certify some of these roles and leave others to the reference's chains (which of them
                 depends on the precision: the asserts say what must occur, the counters are compared role by role)
  plateau,       further material without a claim of its own: a full-scale plateau in front of a noisy sine, full-scale
  noise, music   and 6-bit noise, noisy sines

Compared exactly: every field of the records and the residual rows of flacenc_hip_stereo_qlpc_batch and
flacenc_hip_encode_stereo_frames (with and without the fixed-LPC candidate), R[] and the unquantised coefficients bit for
bit through flacenc_hip_qlpc_batch on the 32 roles as independent channels (the plain order-8 instance takes the same
path, and it alone hands these rows out), and the certificate's three device counters against the oracle's decisions on
the same systems.  One launch at lpc_order 7 shows the generic code still serving the same instance."""
import numpy as np
import pytest

import util
from flacenc_rs_amd import _capi
from oracle import oracle as orc
from test_gpu_solver_full_order import assert_records_equal, check_frames, check_stereo_roles

pytestmark = pytest.mark.gpu

BPS = 16
N = 4096
ORDER = 8
# four_orders: (lag, amplitude) of the left channel's weak partners, by precision
WEAK = {3: ((6, 8000, 1), (7, 4800, 1), (8, 1800, 1)),
        8: ((6, 320, 1), (7, 100, 1), (8, 16, 1)),
        15: ((6, 5, 2), (7, 3, 2), (8, 1, 3))}


def impulse_groups(parts, base, start, first=None, last=None):
    """x[t0] = base and x[t0 + d] = amp (in every `every`-th group) for groups 64 samples apart"""
    x = np.zeros(N, np.int64)
    for j, t0 in enumerate(range(start, N - 16, 64)):
        if first is not None and not first <= t0 < last:
            continue
        x[t0] += base
        for d, amp, every in parts:
            if j % every == 0:
                x[t0 + d] += amp
    return x


def frames_for(precision):
    music = [util.sine_noise(N, BPS, 200.0 + 13 * k, 0.4, 0.05, seed=70 + k) for k in range(4)]
    near = [util.sine_noise(N, BPS, 57.3, 0.6, 5e-4, 400 + k, phase=0.1 * k) for k in range(2)]
    plateau = [util.sine_noise(N, BPS, 36.0 + k, 0.4, 0.04, 31 + k, phase=0.2 * k) for k in range(2)]
    for k in range(2):
        plateau[k] = plateau[k].copy()
        plateau[k][: 9 + k] = 30000 if k else -30000
    a5 = impulse_groups([(5, 8000, 1)], 16000, 40)
    weak = impulse_groups(WEAK[precision], 16000, 72)
    pairs = impulse_groups([(8, 12000, 1)], 12000, 40, first=N // 4, last=3 * N // 4)  # (Tukey(0.4): flat on [0.2 n, 0.8 n])
    rng = np.random.default_rng(9)
    lo, hi = -(1 << (BPS - 1)), (1 << (BPS - 1)) - 1
    named = [
        ("four_orders", a5 + weak, a5),
        ("clamp_hi", music[0], pairs),
        ("silence", music[1], music[1]),
        ("near_pure", near[0], near[1]),
        ("plateau", plateau[0], plateau[1]),
        ("tones", util.quantize(util.sine(N, 37.3, 0.98), BPS), util.quantize(util.sine(N, 23.0, 0.45) + util.sine(N, 7.7, 0.45, phase=1.0), BPS)),
        ("noise", rng.integers(lo, hi + 1, N), rng.integers(-40, 41, N)),
        ("music", music[2], music[3]),
    ]
    names = [k for k, _, _ in named]
    frames = np.stack([np.stack([np.asarray(l), np.asarray(r)]) for _, l, r in named]).astype(np.int32)
    assert frames.shape == (8, 2, N) and np.abs(frames.astype(np.int64)).max() <= 1 << (BPS - 1)
    return names, frames


def roles_of(frames):
    """the 32 roles as independent channels: int32 [32, N] and their bits per sample"""
    rows, bps = [], []
    for f in range(frames.shape[0]):
        l, r = frames[f, 0], frames[f, 1]
        m, s = orc.stereo_to_midside(l, r)
        rows += [l, r, m, s]
        bps += [BPS, BPS, BPS, BPS + 1]
    return np.stack(rows), np.asarray(bps, np.uint8)


_CONTENT = {}


def content(precision):
    """(names, frames, role rows, their bps, the oracle's records / residual / R / a of the roles, its certificate
    decisions per role) -- computed once per precision, shared, left unchanged; the events asserted from the oracle."""
    if precision in _CONTENT:
        return _CONTENT[precision]
    names, frames = frames_for(precision)
    x, bps = roles_of(frames)
    cfg = orc.make_config(lpc_order=ORDER, quant_precision=precision, acorr=orc.ACORR_CANONICAL)
    cp, cres, cR, cA = orc.qlpc_batch(x, bps, cfg, nthreads=1)
    stats = []
    for k in range(x.shape[0]):
        orc.cert_stats(reset=True)
        orc.qlpc_batch(x[k:k + 1], bps[k:k + 1], cfg, nthreads=1, want_fp=False)
        stats.append(orc.cert_stats())
    stats = np.asarray(stats)
    assert (stats[:, 0] == 1).all()
    hi = (1 << (precision - 1)) - 1
    f = {name: slice(4 * k, 4 * k + 4) for k, name in enumerate(names)}
    assert len(set(cp["order"][f["four_orders"]].tolist())) == 4, cp["order"][f["four_orders"]].tolist()
    k = f["clamp_hi"].start + 1  # the right channel
    assert int(cp["coefs"][k][7]) == hi and int(cp["order"][k]) == 8 and stats[k].tolist() == [1, 1, 1], (cp[k], stats[k])
    k = f["silence"].start + 3
    assert not x[k].any() and int(cp["order"][k]) == 1 and not cp["coefs"][k].any() and int(cp["shift"][k]) == 15
    tonal = np.r_[stats[f["near_pure"]], stats[f["tones"]]]
    assert tonal[:, 1].sum() >= 2, "near-pure tones take the certificate's second tier"
    assert ((tonal[:, 1] == 1) & (tonal[:, 2] == 0)).any(), "... which certifies one of them"
    assert tonal[:, 2].sum() >= 1, "... and leaves one to the reference's chains"
    assert 0 < stats[:, 1].sum() < len(stats), "both tiers decide somewhere"
    _CONTENT[precision] = (names, frames, x, bps, cp, cres, cR, cA, stats)
    return _CONTENT[precision]


@pytest.fixture(scope="module")
def handle():
    h = _capi.Handle(0, hooks=True)  # (the hooks build: the certificate's device counters)
    yield h
    h.close()


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


@pytest.mark.parametrize("precision", [3, 8, 15])
def test_lane_parallel_quantiser_gives_the_oracles_records(handle, precision):
    names, frames, x, bps, cp, cres, cR, cA, stats = content(precision)
    want_stats = stats.sum(axis=0).tolist()
    gcfg = _capi.make_config(lpc_order=ORDER, quant_precision=precision)
    # the roles as independent channels: R[], a[], records, rows; the counters
    (gp, gres, gR, gA), got_stats = counted(handle, lambda: handle.qlpc_batch(x, bps, gcfg, want_fp=True))
    assert np.array_equal(gR.view(np.uint64), cR.view(np.uint64)), "autocorrelation bits"
    assert np.array_equal(gA.view(np.uint64), cA.view(np.uint64)), "LPC coefficient bits"
    assert_records_equal(gp, cp, "qlpc_batch")
    assert np.array_equal(gres, cres)
    assert got_stats == want_stats, (got_stats, want_stats)
    # the stereo instances: the four roles' records, then the bench's entry point with and without the fixed-LPC candidate
    _, got_stats = counted(handle, lambda: check_stereo_roles(handle, frames, ORDER, precision))
    assert got_stats == want_stats, (got_stats, want_stats)
    _, got_stats = counted(handle, lambda: check_frames(handle, frames, ORDER, precision, use_fixed=False))
    assert got_stats == want_stats, (got_stats, want_stats)
    check_frames(handle, frames, ORDER, precision, use_fixed=True)


def test_one_order_below_the_generic_code_serves_the_same_instance(handle):
    names, frames, *_ = content(8)
    check_stereo_roles(handle, frames, ORDER - 1, 8)
    check_frames(handle, frames, ORDER - 1, 8, use_fixed=False)
