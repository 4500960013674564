"""The fused 4096 / 4608 kernel's partitioned-Rice search against the CPU oracle, field by field, on material that takes
each of its paths: the reduce-scatter search of the common case (one group of four parameters, tagged entries) and the
clamped search for wider windows, a configured parameter limit, the finest-order flag, 4608-sample blocks and the
fixed-LPC instances.  The lane model's predicate (tests/rice_scatter_model.py) classifies the subframes on the CPU, from
the oracle's residuals, and both paths must have been exercised."""
import functools

import numpy as np
import pytest

import rice_scatter_model as rsm
import util
from flacenc_rs_amd import _capi
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

BPS = 16
NFRAMES = 64
RECORD_FIELDS = ("order", "shift", "precision", "rice_order", "status", "code_bits", "sum_quotients", "subframe_bits")


@pytest.fixture(scope="module")
def handle():
    h = _capi.Handle(0)
    yield h
    h.close()


@functools.lru_cache(maxsize=None)
def frames_of(n):
    """64 stereo frames, int32 [64, 2, n], 16-bit.  White noise leaves the predictor nothing, so the residual's partition
    means follow the amplitudes set here."""
    rng = np.random.default_rng(0x51CE0000 + n)
    lo, hi = -(1 << (BPS - 1)), (1 << (BPS - 1)) - 1
    out = []
    for k in range(1, 16):  # white noise at amplitude 2^1 .. 2^15
        out.append(rng.integers(-(1 << k), (1 << k) + 1, (2, n)))
    parts = -(-n // 64)
    for step in (2, 4, 64):  # amplitude steps between 64-sample partitions: windows of 4, 5 and more
        for base in (3, 40, 300):
            env = np.repeat(base * np.where(rng.random(parts) < 0.5, 1, step), 64)[:n]
            out.append(rng.integers(-1000, 1001, (2, n)) * env[None, :] // 1000)
    for k in range(6):  # silence with sparse impulses
        hit = rng.random((2, n)) < 2.0 ** -(4 + k)
        out.append(np.where(hit, rng.integers(-(1 << (3 + 2 * k)), 1 << (3 + 2 * k), (2, n)), 0))
    for k in range(6):  # |s| <= 1: rich in ties
        out.append(rng.integers(-1, 2, (2, n)) * (rng.random((2, n)) < (k + 1) / 6.0))
    for name in ("sus109", "ras22", "ras103", "sus6"):  # the real-audio fixtures
        x = np.stack([util.test_signal(name, c) for c in range(2)])
        for f in range(8192 // n):
            out.append(x[:, f * n:(f + 1) * n])
    k = 0
    while len(out) < NFRAMES:  # tonal material with a noise floor
        out.append(np.stack([util.sine_noise(n, BPS, 50.0 + 37.0 * k + 11.0 * c, 0.4, 0.02 * (1 + k % 5), seed=77 + 2 * k + c)
                             for c in range(2)]))
        k += 1
    return np.ascontiguousarray(np.clip(np.stack(out[:NFRAMES]), lo, hi).astype(np.int32))


def configs(order, max_rice, finest):
    g = _capi.make_config(lpc_order=order, max_rice_parameter=max_rice, rice_finest_only=finest)
    o = orc.make_config(lpc_order=order, max_rice_parameter=max_rice, rice_finest_only=finest, acorr=orc.ACORR_CANONICAL)
    return g, o


def fast_subframes(records, residual, max_rice):
    """The model's predicate on the oracle's residual rows (4096 samples, warm-up = the record's order)."""
    fast = np.zeros(len(records), bool)
    for warm in np.unique(records["order"]):
        sel = np.nonzero(records["order"] == warm)[0]
        rows = residual[sel].copy()
        rows[:, :int(warm)] = 0
        fast[sel] = rsm.is_fast(rows, int(warm), max_rice)
    return fast


CASES = [
    # id, n, order, max_rice_parameter, finest-order flag
    ("order8", 4096, 8, 30, False),
    ("order10", 4096, 10, 30, False),
    ("max_rice3", 4096, 8, 3, False),
    ("max_rice13", 4096, 8, 13, False),
    ("finest_order", 4096, 8, 30, True),
    ("block4608", 4608, 8, 30, False),
]


@pytest.mark.parametrize("name,n,order,max_rice,finest", CASES, ids=[c[0] for c in CASES])
def test_roles_equal_oracle(handle, name, n, order, max_rice, finest):
    """stereo_qlpc_batch: the records and residual rows of L, R, M and S of every frame."""
    frames = frames_of(n)
    gcfg, ocfg = configs(order, max_rice, finest)
    params, residual = handle.stereo_qlpc_batch(frames, BPS, gcfg)
    roles = np.empty((NFRAMES, 4, n), np.int32)
    for f in range(NFRAMES):
        l, r = frames[f, 0], frames[f, 1]
        m, s = orc.stereo_to_midside(l, r)
        roles[f] = (l, r, m, s)
    bps = np.tile(np.array([BPS, BPS, BPS, BPS + 1], np.uint8), NFRAMES)
    want, wres, _, _ = orc.qlpc_batch(roles.reshape(-1, n), bps, ocfg, nthreads=8, want_fp=False)
    got = params.reshape(-1)
    gres = residual.reshape(-1, n)
    for fld in RECORD_FIELDS:
        bad = np.nonzero(got[fld] != want[fld])[0]
        assert len(bad) == 0, (name, fld, bad[:8].tolist(), got[fld][bad[:8]].tolist(), want[fld][bad[:8]].tolist())
    assert np.array_equal(got["rice_params"], want["rice_params"]), name
    assert np.array_equal(got["coefs"], want["coefs"]), name
    assert np.array_equal(gres, wres), name
    if n == 4096:
        fast = fast_subframes(want, wres, max_rice)
        if max_rice == 30:  # (the kernel adds !finest_only to the predicate)
            assert fast.sum() >= 32 and (~fast).sum() >= 32, (name, int(fast.sum()))
        else:
            assert (~fast).sum() >= 32, name  # a limit below the bit length sends the subframe to the clamped search


FRAME_CASES = [
    # id, n, order, max_rice_parameter, finest-order flag, fixed-LPC candidate
    ("headline", 4096, 8, 30, False, False),
    ("headline_order10", 4096, 10, 30, False, False),
    ("headline_max_rice13", 4096, 8, 13, False, False),
    ("headline_finest_order", 4096, 8, 30, True, False),
    ("fixed_candidate", 4096, 8, 30, False, True),
]


@pytest.mark.parametrize("name,n,order,max_rice,finest,use_fixed", FRAME_CASES, ids=[c[0] for c in FRAME_CASES])
def test_frames_equal_oracle(handle, name, n, order, max_rice, finest, use_fixed):
    """encode_stereo_frames, the instance the bench runs (and the fixed-LPC one): the decision, the chosen subframes'
    records and their residual rows."""
    frames = frames_of(n)
    gcfg, ocfg = configs(order, max_rice, finest)
    got, gres = handle.encode_stereo_frames(frames, BPS, _capi.make_frame_config(gcfg, use_fixed=use_fixed))
    if use_fixed:
        ofc = orc.make_frame_config(ocfg, use_fixed=True, fixed=orc.make_fixed_config(sum_mode=orc.SUMABS_CANONICAL))
        want, wres = orc.encode_stereo_frames_cfg(frames, BPS, ofc)
    else:
        want, wres = orc.encode_stereo_frames(frames, BPS, ocfg)
    for fld in ("channel_assignment", "role", "kind", "dc_offset", "bits"):
        assert np.array_equal(got[fld], want[fld]), (name, fld)
    lpc = want["kind"] >= 2  # [frames, 2]: the subframes whose record is meaningful
    for fld in RECORD_FIELDS:
        assert np.array_equal(got["lpc"][fld][lpc], want["lpc"][fld][lpc]), (name, fld)
    assert np.array_equal(got["lpc"]["rice_params"][lpc], want["lpc"]["rice_params"][lpc]), name
    assert np.array_equal(got["lpc"]["coefs"][lpc], want["lpc"]["coefs"][lpc]), name
    assert np.array_equal(gres, wres), name
    assert lpc.sum() >= NFRAMES, name  # (most subframes are coded with the LPC candidate)
    if not use_fixed and not finest and max_rice == 30:
        fast = fast_subframes(want["lpc"][lpc], wres[lpc], max_rice)
        assert fast.sum() >= 16 and (~fast).sum() >= 8, (name, int(fast.sum()), int((~fast).sum()))
