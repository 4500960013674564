"""FLACENC_HIP_FLAG_ORDER_SEARCH on worst-case material: every branch of order_search_kernel (residual arithmetic, the
proved and the widened parameter window, saturated table entries, RICE2 parameters, both residual-row homes), every
levinson_bucket edge and the shapes where the partition layout changes, held to tests/order_model.py record by record;
a seeded fuzz over the configuration space; invariants that need no model; frames with and without wasted bits; and
flagged and unflagged big-block batches, one of them through the clean-up launch, on one handle.  Each deterministic case asserts (from the model, on the CPU) that it
reaches the branch it names."""
import numpy as np
import pytest
import torch

import extreme_signals as es
import order_model as om
import util
from flacenc_rs_amd import _capi
from oracle import oracle as orc

pytestmark = pytest.mark.gpu
OS = _capi.FLAG_ORDER_SEARCH
REF = _capi.FLAG_REFERENCE_SUM_ORDER
NIGHTLY = _capi.FLAG_NIGHTLY_SUM_ORDER
FINEST = _capi.FLAG_FINEST_RICE_ORDER
LDS_EDGE = list(es.lds_edge())  # [20243: the largest image that fits, 20244, 20245: past it]


@pytest.fixture(scope="module")
def h():
    with _capi.Handle(0) as handle:
        yield handle


def run_case(h, rows, bps, order, flags=0, nightly=False, finest=False, **kw):
    """The flagged candidate batch on `rows` == the model, record by record."""
    x = np.ascontiguousarray(np.asarray(rows, np.int64).astype(np.int32))
    gflags = OS | flags | (NIGHTLY if nightly else 0) | (FINEST if finest else 0)
    params, residual, R, A = h.qlpc_batch(x, bps, _capi.make_config(lpc_order=order, flags=gflags, **kw), want_fp=True)
    cfg = om.config(order=order, nightly=nightly, rice_finest_only=finest, **kw)
    es.check_rows(params, residual, R, A, x, bps, cfg, (x.shape, bps if np.ndim(bps) == 0 else "rows", order, kw))
    return params, cfg


def reaches(rows, bps, cfg):
    out = set()
    for i, r in enumerate(rows):
        out |= es.branches(r, int(bps[i]) if np.ndim(bps) else bps, cfg)
    return out


# ---- a: one case per branch ----
def _sine(n, amp, period=37.0, phase=0.0):
    return np.round(np.sin(np.arange(n) * 2 * np.pi / period + phase) * amp).astype(np.int64)


def test_residual_arithmetic_on_both_sides_of_the_i24_criterion(h):
    # maxabs < 2^23 with a small sum of |c| (precision 3): v_mad_i32_i24; one sample at -2^23: the i64 path
    lo24 = _sine(4096, (1 << 23) - 1)
    at24 = lo24.copy()
    at24[777] = -(1 << 23)
    _, cfg = run_case(h, [lo24, at24], 24, 2, quant_precision=3, window="rectangle")
    assert es.branches(lo24, 24, cfg) >= {"i24"} and "i64" not in es.branches(lo24, 24, cfg)
    assert "i64" in es.branches(at24, 24, cfg)
    # maxabs . sum|c| on both sides of 2^31 - 1 with maxabs < 2^23: the same sine at two amplitudes, precision 15
    small, big = _sine(4096, 3000), _sine(4096, 1 << 22)
    _, cfg = run_case(h, [small, big], 24, 8)
    assert "i64" not in es.branches(small, 24, cfg) and "i64" in es.branches(big, 24, cfg)


def test_window_left_as_proved_on_ordinary_material(h):
    rows = [es.music(4096, 16, start=k * 4096) for k in range(4)]
    _, cfg = run_case(h, rows, 16, 8)
    assert reaches(rows, 16, cfg).isdisjoint({"wide", "ksat", "clamp"})


@pytest.mark.parametrize("bits,order,window,precision", [
    (24, 24, "rectangle", 12), (24, 32, ("tukey", 0.0), 8), (25, 32, ("tukey", 1.0), 5), (25, 24, "rectangle", 3)])
def test_window_widened_by_codes_of_2_27(h, bits, order, window, precision):
    # full-scale alternation: a high order's residual wraps i32, codes >= 2^27 -> the wide key's quotient pass, and
    # chosen parameters above 14 (RICE2)
    x = es.alternation(4096, bits)
    rows = [x, -x - 1]
    _, cfg = run_case(h, rows, bits, order, window=window, quant_precision=precision)
    assert reaches(rows, bits, cfg) >= {"wide", "rice2"}


@pytest.mark.parametrize("n,bits", [(4097, 22), (32767, 20), (4095, 22)])
def test_window_widened_by_partition_sums_of_2_32(h, n, bits):
    # odd n: one partition; noise residuals sum past 2^32 with codes below 2^27 -> kSat alone
    rows = [es.noise(n, bits, seed=n + k) for k in range(2)]
    _, cfg = run_case(h, rows, 24, 8)
    got = reaches(rows, 24, cfg)
    assert "ksat" in got and "wide" not in got


@pytest.mark.parametrize("n", [4096, 4097, 1000])
@pytest.mark.parametrize("max_p", [0, 1, 2, 4])
def test_chosen_level_clamped(h, n, max_p):
    # 24- / 25-bit material with max_rice_parameter far below its scale: the chosen level's table entries saturate at
    # MAX_P_TO_BITS, so its key is the true quotient sum at p = 0, not the clamped table sum
    rows = [es.music(n, 24, start=0), es.music(n, 24, start=5 * n), es.noise(n, 24, seed=n)]
    _, cfg = run_case(h, rows, 24, 8, max_rice_parameter=max_p)
    rows25 = [es.noise(n, 25, seed=n + 1)]
    run_case(h, rows25, 25, 12, max_rice_parameter=max_p)
    if max_p <= 2:
        assert "clamp" in reaches(rows, 24, cfg)


def test_statuses_and_ties(h):
    # silence (R[0] = 0), DC and a single impulse: every order ties, the lower order must win; the plateau fixture
    n = 4096
    rows = [np.zeros(n, np.int64), np.full(n, 1234), np.full(n, -(1 << 23)), np.eye(1, n, 100)[0].astype(np.int64) * 8000000]
    for window in ("rectangle", ("tukey", 0.4)):
        params, _ = run_case(h, rows, 24, 8, window=window)
        assert int(params["order"][0]) == 1 and int(params["order"][3]) == 1
    plateau = np.load(util.GOLDEN + "/cert_nonpd_plateau_24bit.npy").astype(np.int64).reshape(-1)[:n]
    run_case(h, [plateau, plateau[::-1]], 24, 12)
    # short blocks of music where several orders tie exactly (found by a search of the model)
    for n2, bits, P, prec, start in ((65, 16, 16, 2, 2755), (65, 16, 12, 2, 42459), (97, 8, 32, 1, 83823),
                                     (127, 16, 16, 1, 92411)):
        x = es.music(n2, bits, start=start)
        cfg = om.config(order=P, quant_precision=prec)
        _, _, keys = om.search(x.astype(np.int32), bits, cfg)
        ok = [k for k in keys.values() if k is not None]
        assert ok.count(min(ok)) > 1
        run_case(h, [x], bits, P, quant_precision=prec)


SHAPES = [64, 65, 97, 127, 1000, 4095, 4096, 4097, 4160, 4608, 6144, 8192, 16383, 16384] + LDS_EDGE + [24576, 32767]


@pytest.mark.parametrize("n", SHAPES)
def test_shapes(h, n):
    # finest partition order 0 (n < 128, odd n), psize 65 (4160: a wave straddles two partitions), the big-block stage 3
    # (4096 / 8192 / 16384), the generic stage 3 elsewhere, the residual rows in LDS (up to 16383, and 16385..20243
    # mostly) and out of it (16384: its 256 partitions' tables; 20244, 20245: past the largest image, 20243's)
    order = 32 if n >= 8192 else 12
    rows = [es.music(n, 24, start=n), es.alternation(n, 24), es.noise(n, 24, seed=n)]
    run_case(h, rows, 24, order, window="rectangle", quant_precision=12)
    rows16 = [es.music(n, 16, start=2 * n), es.extreme_frames(np.random.default_rng(n), n, 16)[0, 0]]
    run_case(h, rows16, 16, 8)


@pytest.mark.parametrize("order", [1, 2, 8, 9, 12, 13, 16, 17, 24, 25, 32])
def test_every_levinson_bucket_edge(h, order):
    n = 4096
    rows = [es.music(n, 24, start=order * n), es.music(n, 16, start=3 * order * n), es.alternation(n, 24)]
    run_case(h, rows, np.array([24, 16, 24], np.uint8), order, window="rectangle", quant_precision=12)


@pytest.mark.parametrize("n,bits", [(4096, 16), (1152, 8), (8192, 16)])
def test_per_row_bits_per_sample(h, n, bits):
    x = es.extreme_frames(np.random.default_rng(n + bits), n, bits).reshape(-1, n)
    bpsv = np.full(x.shape[0], bits, np.uint8)
    bpsv[1::2] = bits + 1
    run_case(h, x, bpsv, 12)


# ---- b: a seeded fuzz over the configuration space ----
FUZZ_SHAPES = SHAPES
WINDOWS = ["rectangle", ("tukey", 0.0), ("tukey", 0.1), ("tukey", 0.4), ("tukey", 1.0)]
MAX_PS = [0, 1, 2, 4, 6, 14, 15, 30]


def fuzz_trial(rng):
    """-> (rows, per-row bps, order, nightly, finest, config keywords) of one sampled configuration."""
    n = int(rng.choice(FUZZ_SHAPES))
    bits = int(rng.choice([8, 16, 24]))
    nightly = bool(rng.random() < 0.25)
    finest = bool(rng.random() < 0.2)
    order = int(rng.choice([1, 2, 8, 9, 12, 13] if nightly else [1, 2, 8, 9, 12, 13, 16, 17, 24, 25, 32]))
    kw = dict(quant_precision=int(rng.integers(1, 16)), window=WINDOWS[int(rng.integers(0, len(WINDOWS)))],
              max_rice_parameter=int(rng.choice(MAX_PS)))
    x = es.extreme_frames(rng, n, bits).reshape(-1, n)
    keep = 2 if n >= 8192 else 6
    x = x[rng.permutation(len(x))[:keep]]
    bpsv = np.full(len(x), bits, np.uint8)
    if bits < 24:
        bpsv[1::2] = bits + 1
    return x, bpsv, order, nightly, finest, kw


# seeds 2, 5, 6 and 7 found the saturated-level key (the kernel keyed such levels by their clamped table sums):
# 24-bit rows at max_rice_parameter 0, 1 or 6 (n = 4096 / 1000 / 4608 / 24576); and seed 3 of the invariants below
# found the record that was longer than REFERENCE_SUM_ORDER's (n = 32767, order 32, max_rice_parameter 6)
@pytest.mark.parametrize("seed", range(8))
def test_configuration_fuzz(h, seed):
    rng = np.random.default_rng(8100 + seed)
    for trial in range(4):
        x, bpsv, order, nightly, finest, kw = fuzz_trial(rng)
        tag = (seed, trial, x.shape, bpsv.tolist(), order, nightly, finest, kw)
        try:
            run_case(h, x, bpsv, order, nightly=nightly, finest=finest, **kw)
        except AssertionError as e:
            raise AssertionError(f"configuration {tag}: {e}") from e


# ---- c: invariants without the model ----
@pytest.mark.parametrize("seed", range(4))
def test_never_longer_than_the_reference_order_and_unchanged_at_order_1(h, seed):
    rng = np.random.default_rng(8200 + seed)
    for trial in range(4):
        x, bpsv, order, _, finest, kw = fuzz_trial(rng)
        tag = (seed, trial, x.shape, bpsv.tolist(), order, finest, kw)
        extra = FINEST if finest else 0
        try:
            got = h.qlpc_batch(x, bpsv, _capi.make_config(lpc_order=order, flags=OS | REF | extra, **kw), want_fp=True)
            ref = h.qlpc_batch(x, bpsv, _capi.make_config(lpc_order=order, flags=REF | extra, **kw), want_fp=True)
            for i in range(len(x)):
                if int(ref[0][i]["status"]) == 0:
                    assert int(got[0][i]["status"]) == 0, i
                    assert int(got[0][i]["subframe_bits"]) <= int(ref[0][i]["subframe_bits"]), i
            one = h.qlpc_batch(x, bpsv, _capi.make_config(lpc_order=1, flags=OS | REF | extra, **kw), want_fp=True)
            ref1 = h.qlpc_batch(x, bpsv, _capi.make_config(lpc_order=1, flags=REF | extra, **kw), want_fp=True)
            assert one[0].tobytes() == ref1[0].tobytes()
            assert np.array_equal(one[1], ref1[1])
        except AssertionError as e:
            raise AssertionError(f"configuration {tag}: {e}") from e


# ---- d: frames ----
def frame_cfg(order, flags=0, use_fixed=False, stereo=True, search=True, **kw):
    qlpc = _capi.make_config(lpc_order=order, flags=(OS if search else 0) | flags, **kw)
    return _capi.make_frame_config(qlpc, use_fixed=use_fixed, use_leftside=stereo, use_rightside=stereo,
                                   use_midside=stereo)


def gpu_frames(h, cfg, x, bps, stereo=True):
    n, C, b = x.shape
    dx = torch.from_numpy(np.ascontiguousarray(x, np.int32)).cuda()
    slot = h.frame_bytes_bound(b, bps) if stereo else h.frame_bytes_bound_channels(C, b, bps)
    out = torch.zeros(n * slot, dtype=torch.uint8, device="cuda")
    ln = torch.zeros(n, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    if stereo:
        res = torch.zeros(n * 752, dtype=torch.uint8, device="cuda")
        h.encode_pack_stereo_frames_device(cfg, dx.data_ptr(), n, b, b, bps, 44100, 0, 1, res.data_ptr(), out.data_ptr(),
                                           slot, ln.data_ptr(), stream)
    else:
        res = torch.zeros(n * C * 368, dtype=torch.uint8, device="cuda")
        h.encode_pack_frames_device(cfg, dx.data_ptr(), n, C, b, b, bps, 44100, 0, 1, res.data_ptr(), out.data_ptr(),
                                    slot, ln.data_ptr(), stream)
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


FRAME_CASES = [(4096, 24, 8, 0), (4096, 24, 32, 2), (4097, 24, 12, 0), (1000, 16, 12, 30), (8192, 16, 32, 4),
               (4096, 8, 8, 30)]


@pytest.mark.parametrize("n,bits,order,max_p", FRAME_CASES)
def test_worst_case_frames_equal_the_model_and_are_never_longer(h, n, bits, order, max_p):
    rng = np.random.default_rng(8300 + n + order)
    x = es.extreme_frames(rng, n, bits)
    x[0] = np.stack([es.music(n, bits, start=n), es.music(n, bits, start=3 * n)])
    kw = dict(max_rice_parameter=max_p, window="rectangle", quant_precision=12)
    fc = orc.make_frame_config(om.config(order=order, **kw), use_fixed=False)
    got = gpu_frames(h, frame_cfg(order, **kw), x, bits)
    for f in range(len(x)):
        assert got[f] == om.stereo_frame_bytes(x[f, 0], x[f, 1], bits, fc, number=f), (n, bits, order, max_p, f)
    decode_check(h, got, x, bits)
    plain = gpu_frames(h, frame_cfg(order, REF, search=False, **kw), x, bits)
    assert all(len(g) <= len(p) for g, p in zip(got, plain))
    # independent channels: three per frame
    xc = np.concatenate([x[:3], x[3:]], 1)[:, :3]
    fci = orc.make_frame_config(om.config(order=order, **kw), use_fixed=False, use_leftside=False,
                                use_rightside=False, use_midside=False)
    gotc = gpu_frames(h, frame_cfg(order, stereo=False, **kw), xc, bits, stereo=False)
    for f in range(len(xc)):
        assert gotc[f] == om.channel_frame_bytes(list(xc[f]), bits, fci, number=f), (n, bits, order, max_p, f)
    decode_check(h, gotc, xc, bits)


@pytest.mark.parametrize("n,order,max_p", [(4096, 8, 30), (4096, 32, 2), (1000, 12, 0), (8192, 12, 14)])
def test_worst_case_frames_with_wasted_bits(h, n, order, max_p):
    rng = np.random.default_rng(8400 + n + order)
    x = es.extreme_frames(rng, n, 16).astype(np.int64)
    for f in range(len(x)):
        x[f] <<= 1 + f  # shifted left by 1..6 bits
    x[-1, 0] <<= 2      # (and 8 bits in one channel: different k inside one frame)
    x = x.astype(np.int32)
    kw = dict(max_rice_parameter=max_p)
    fc = orc.make_frame_config(om.config(order=order, **kw), use_fixed=False)
    got = gpu_frames(h, frame_cfg(order, _capi.FLAG_WASTED_BITS, **kw), x, 24)
    for f in range(len(x)):
        assert got[f] == om.wasted_stereo_frame_bytes(x[f, 0], x[f, 1], 24, fc, number=f), (n, order, max_p, f)
    decode_check(h, got, x, 24)
    plain = gpu_frames(h, frame_cfg(order, REF | _capi.FLAG_WASTED_BITS, search=False, **kw), x, 24)
    assert all(len(g) <= len(p) for g, p in zip(got, plain))


# ---- e: handle state ----
def test_flagged_and_unflagged_big_blocks_on_one_handle_equal_fresh_handles(h):
    # 1. a flagged 8192-sample batch: slow full-scale 25-bit sines with a full-swing impulse at a trough (the flagged
    #    orders are low, so these rows stay below the 2^26 that marks rows for the clean-up launch; no material found
    #    makes a flagged batch mark rows at 25 bits); 2. an unflagged order-32 batch of 24-bit full-scale alternation
    #    whose order-32 residuals wrap, which the big-block stage 3 marks and the clean-up launch redoes; 3. an unflagged
    #    4096 batch; 4. the flagged batch again.  Every result equals a fresh handle's.
    n = 8192
    big = np.stack([_sine(n, (1 << 24) - 1, period=2000.0 + 300 * k) for k in range(3)])
    for k in range(3):
        t = int(np.argmin(big[k, 1000:3000])) + 1000
        big[k, t] = (1 << 24) - 1
    big = big.astype(np.int32)
    kw = dict(window="rectangle", quant_precision=12)
    flagged = _capi.make_config(lpc_order=32, flags=OS, **kw)
    alt = np.stack([es.alternation(n, 24), -es.alternation(n, 24) - 1]).astype(np.int32)
    marking = _capi.make_config(lpc_order=32, **kw)
    x4 = np.stack([es.music(4096, 16, start=k * 4096) for k in range(8)]).astype(np.int32)
    plain = _capi.make_config(lpc_order=12)
    with _capi.Handle(0) as hh:
        a1 = hh.qlpc_batch(big, 25, flagged, want_fp=True)
        m = hh.qlpc_batch(alt, 24, marking, want_fp=True)
        u = hh.qlpc_batch(x4, 16, plain, want_fp=True)
        a2 = hh.qlpc_batch(big, 25, flagged, want_fp=True)
    with _capi.Handle(0) as fresh:
        f1 = fresh.qlpc_batch(big, 25, flagged, want_fp=True)
    with _capi.Handle(0) as fresh:
        fm = fresh.qlpc_batch(alt, 24, marking, want_fp=True)
    with _capi.Handle(0) as fresh:
        fu = fresh.qlpc_batch(x4, 16, plain, want_fp=True)
    for got, ref in ((a1, f1), (m, fm), (u, fu), (a2, f1)):
        assert all(np.array_equal(g, r) for g, r in zip(got, ref))
    assert all(int(es.zigzag(r).max()) >= 1 << 26 for r in fm[1])  # (rows the big-block stage 3 marks)
    es.check_rows(*f1, big, 25, om.config(order=32, **kw), "big block")
