"""FLACENC_HIP_FLAG_WINDOW_SEARCH on worst-case material, as tests/test_gpu_order_search_extremes.py holds the order
search: every branch of order_search_kernel with several windows in one workgroup (residual arithmetic, the proved and
the widened parameter window, saturated table entries, RICE2 parameters, both residual-row homes); candidates of one
subframe in different regimes, so that state carried from one candidate to the next shows; ties between windows; extra
windows without a non-zero weight; every levinson_bucket edge and the shapes where the partition layout changes; a
seeded fuzz over configurations and extra-window lists; invariants that need no model; slices with a first subframe
above 0 for stereo samples, per-row bps and residual rows outside LDS; and frames with and without wasted bits.  All of
it is held to tests/window_model.py record by record and byte by byte: no comparison here has a tolerance.  Each
deterministic case (tests/window_cases.py) first asserts from the model, on the CPU, that it reaches what it names.

Not reached: order_pick_kernel's "no candidate with status 0, so candidate (0, P)" arm.  R[] of finite integer input is
finite with R[0] >= 0, so every candidate of every window has status 0 (the non-positive-definite plateau fixture too,
forwards and reversed; window_cases.claims asserts it for every case), and nothing the ABI accepts reaches that arm."""
import numpy as np
import pytest

import extreme_signals as es
import order_model as om
import window_cases as wc
import window_model as wm
from flacenc_rs_amd import _capi
from oracle import oracle as orc
from test_gpu_order_search_extremes import FRAME_CASES, decode_check, fuzz_trial, gpu_frames

pytestmark = pytest.mark.gpu
WS = _capi.FLAG_WINDOW_SEARCH
OS = _capi.FLAG_ORDER_SEARCH
REF = _capi.FLAG_REFERENCE_SUM_ORDER
NIGHTLY = _capi.FLAG_NIGHTLY_SUM_ORDER
FINEST = _capi.FLAG_FINEST_RICE_ORDER
SCRATCH_CAP = 768 << 20  # kSearchScratchCap


@pytest.fixture(scope="module")
def h():
    with _capi.Handle(0) as handle:
        yield handle


def batch(h, x, bps, order, extras, orders, flags=0, **kw):
    h.set_lpc_windows(extras)
    cfg = _capi.make_config(lpc_order=order, flags=WS | (OS if orders else 0) | flags, **kw)
    return h.qlpc_batch(x, bps, cfg, want_fp=True)


def run(h, c, orders):
    """Case c reaches what it names (from the model), and its flagged candidate batch == the model, record by record."""
    wc.claims(c, orders)
    got = batch(h, c.rows, c.bps, c.order, c.extras, orders, **c.kw)
    es.check_rows(*got, c.rows, c.bps, wc.config(c), (c.name, orders), es.window_record(c.extras, orders))
    return got


def params_of(cases):
    p, ids = wc.expand(cases)
    return dict(argnames="c,orders", argvalues=p, ids=ids)


# ---- a: one case per branch, several windows per workgroup ----
@pytest.mark.parametrize(**params_of(wc.branch_cases()))
def test_branch(h, c, orders):
    run(h, c, orders)


# ---- b: regimes that change between consecutive candidates ----
@pytest.mark.parametrize(**params_of(wc.regime_cases()))
def test_regime_change(h, c, orders):
    run(h, c, orders)


# ---- c: ties ----
@pytest.mark.parametrize(**params_of(wc.tie_cases()))
def test_tie(h, c, orders):
    params, _, _, _ = run(h, c, orders)
    if c.name.startswith("degenerate") and orders:  # silence and the impulses: every candidate ties, (0, 1) wins
        assert [int(params["order"][i]) for i in (0, 3, 4, 5, 6, 7)] == [1] * 6


# ---- d: windows without a non-zero weight ----
@pytest.mark.parametrize(**params_of(wc.dead_cases()))
def test_dead_window(h, c, orders):
    n = c.rows.shape[1]
    for e in c.extras:
        w = _capi.lpc_window_weights(*e, n)
        assert np.array_equal(w.view(np.uint32), wm.weights(e, n).view(np.uint32)), (c.name, e)
    run(h, c, orders)


# ---- e: shapes ----
@pytest.mark.parametrize("orders", [False, True], ids=["P", "orders"])
@pytest.mark.parametrize("n", wc.SHAPES)
def test_shapes(h, n, orders):
    # finest partition order 0 (n < 128, odd n), psize 65, the big-block stage 3 (4096 / 8192 / 16384), the generic one
    # elsewhere, the residual rows in LDS and out of it (16384; 20244, 20245: past the largest image, 20243's); four
    # windows, order 32 from 8192 up, per-row bps
    run(h, wc.shape_case(n), orders)


@pytest.mark.parametrize("orders", [False, True], ids=["P", "orders"])
@pytest.mark.parametrize("extras", [wc.E1, wc.E7], ids=["W2", "W8"])
@pytest.mark.parametrize("order", wc.BUCKET_EDGES)
def test_every_levinson_bucket_edge(h, order, extras, orders):
    run(h, wc.bucket_case(order, extras), orders)


# ---- f: a seeded fuzz over configurations and extra-window lists ----
def window_fuzz_trial(rng):
    """fuzz_trial of the order-search suite + a random extra-window list and the orders switch."""
    x, bpsv, order, nightly, finest, kw = fuzz_trial(rng)
    extras = wm.random_extras(rng, x.shape[1])
    orders = bool(rng.random() < 0.5)
    return x, bpsv, order, nightly, finest, kw, extras, orders


@pytest.mark.parametrize("seed", range(8))
def test_configuration_fuzz(h, seed):
    rng = np.random.default_rng(9100 + seed)
    for trial in range(4):
        x, bpsv, order, nightly, finest, kw, extras, orders = window_fuzz_trial(rng)
        tag = (seed, trial, x.shape, bpsv.tolist(), order, nightly, finest, kw, extras, orders)
        try:
            got = batch(h, x, bpsv, order, extras, orders, (NIGHTLY if nightly else 0) | (FINEST if finest else 0), **kw)
            cfg = om.config(order=order, nightly=nightly, rice_finest_only=finest, **kw)
            es.check_rows(*got, x, bpsv, cfg, "fuzz", es.window_record(extras, orders))
        except AssertionError as e:
            raise AssertionError(f"configuration {tag}: {e}") from e


@pytest.mark.parametrize("seed", range(4))
def test_invariants_without_the_model(h, seed):
    rng = np.random.default_rng(9200 + seed)
    for trial in range(4):
        x, bpsv, order, _, finest, kw, extras, _ = window_fuzz_trial(rng)
        tag = (seed, trial, x.shape, bpsv.tolist(), order, finest, kw, extras)
        extra = FINEST if finest else 0

        def plain(flags):
            return h.qlpc_batch(x, bpsv, _capi.make_config(lpc_order=order, flags=flags | extra, **kw), want_fp=True)

        try:
            ref, os_only = plain(REF), plain(OS)
            one = batch(h, x, bpsv, order, extras, False, extra, **kw)
            both = batch(h, x, bpsv, order, extras, True, extra, **kw)
            for i in range(len(x)):
                if int(ref[0][i]["status"]) == 0:
                    assert int(one[0][i]["status"]) == 0 and int(both[0][i]["status"]) == 0, i
                    assert int(one[0][i]["subframe_bits"]) <= int(ref[0][i]["subframe_bits"]), i
                    assert int(both[0][i]["subframe_bits"]) <= int(one[0][i]["subframe_bits"]), i
                if int(os_only[0][i]["status"]) == 0:
                    assert int(both[0][i]["subframe_bits"]) <= int(os_only[0][i]["subframe_bits"]), i
            # with an empty list the flag is the summation-order call, and with the order search that call
            for got, want in ((batch(h, x, bpsv, order, (), False, extra, **kw), ref),
                              (batch(h, x, bpsv, order, (), True, extra, **kw), os_only)):
                assert got[0].tobytes() == want[0].tobytes()
                assert all(np.array_equal(g, w) for g, w in zip(got[1:], want[1:]))
        except AssertionError as e:
            raise AssertionError(f"configuration {tag}: {e}") from e


# ---- g: slices whose first subframe is above 0 ----
def slice_edge(W, C):
    """The first slice's subframes: as many as the scratch cap holds, whole stereo frames."""
    return (SCRATCH_CAP // (W * 264 + C * 144 + 4)) & ~3


def distinct_rows(rows, n, bits, seed):
    """`rows` rows of n samples, no two alike: a period of music rows plus the row's number of periods as an offset."""
    period = min(rows, 509)
    base = es.music(period * n, bits).reshape(period, n)
    x = base[np.arange(rows) % period] + (np.arange(rows) // period)[:, None]
    x[:, 0] += np.random.default_rng(seed).integers(0, 64, rows)  # (and within a period too, whatever the fixtures repeat)
    lo, hi = es.full_scale(bits)
    x = np.clip(x, lo, hi).astype(np.int32)
    return x


def test_stereo_slices_read_their_own_frames():
    # frame f of a later slice is read at samples + (sf0 / 2 + 2 f) stride: every frame distinct, so any other offset shows
    b, order, bits = 1152, 32, 16
    extras = wc.E7
    edge = slice_edge(8, 8 * order)
    nf = edge // 4 + 150
    assert 4 * nf * (8 * 264 + 8 * order * 144 + 4) > SCRATCH_CAP and edge % 4 == 0
    x = distinct_rows(2 * nf, b, bits, 1).reshape(nf, 2, b)
    cfg = _capi.make_config(lpc_order=order, flags=WS | OS)
    ocfg = om.config(order=order)
    with _capi.Handle(0) as big:
        big.set_lpc_windows(extras)
        params, residual = big.stereo_qlpc_batch(x, bits, cfg)
        for lo in (0, edge // 4 - 32, nf - 64):  # (the middle one straddles the boundary)
            p2, r2 = big.stereo_qlpc_batch(x[lo:lo + 64], bits, cfg)
            assert np.array_equal(params[lo:lo + 64], p2) and np.array_equal(residual[lo:lo + 64], r2), lo
    # the subframes on both sides of the first boundary and the last one against the model
    for sf in (edge - 1, edge, edge + 1, edge + 3, 4 * nf - 1):
        f, k = divmod(sf, 4)
        m, s = orc.stereo_to_midside(x[f, 0], x[f, 1])
        sig = (x[f, 0], x[f, 1], m, s)[k]
        rec, resid, _, _ = wm.record(sig, bits + (1 if k == 3 else 0), ocfg, extras, True)
        assert int(params[f, k]["status"]) == 0 and es.params_record(params[f, k]) == rec, (sf, f, k)
        assert np.array_equal(residual[f, k], resid), (sf, f, k)


def test_mono_slices_read_their_own_bits_per_sample():
    # bps alternates b and b + 1 from row to row.  A slice starts at a multiple of 4 subframes, so an alternation in
    # step with it would give row sf0 + i the bps of row i: the phase flips at the first boundary, and every row of the
    # second slice then differs from the row a missing offset would read
    b, order, bits = 1152, 32, 16
    extras = wc.E7
    edge = slice_edge(8, 8 * order)
    rows = edge + 600
    x = distinct_rows(rows, b, bits, 2)
    bpsv = (bits + (np.arange(rows) + (np.arange(rows) >= edge)) % 2).astype(np.uint8)
    assert bpsv[edge] != bpsv[0] and bpsv[edge + 1] != bpsv[1] and bpsv[edge - 1] != bpsv[edge - 2]
    cfg = _capi.make_config(lpc_order=order, flags=WS | OS)
    with _capi.Handle(0) as big:
        big.set_lpc_windows(extras)
        got = big.qlpc_batch(x, bpsv, cfg, want_fp=True)
        for lo in (0, edge - 128, rows - 256):
            small = big.qlpc_batch(x[lo:lo + 256], bpsv[lo:lo + 256], cfg, want_fp=True)
            assert all(np.array_equal(g[lo:lo + 256], s_) for g, s_ in zip(got, small)), lo
    idx = [edge - 1, edge, edge + 1, rows - 1]
    es.check_rows(*(g[idx] for g in got), x[idx], bpsv[idx], om.config(order=order), "bps slice edge",
                  es.window_record(extras, True))


def test_slices_with_the_residual_rows_outside_lds():
    # 16384 samples: order_search_kernel keeps its zig-zag rows in the output rows, at residual + (sf0 + sf) stride
    b, order, bits = 16384, 32, 24
    extras = wc.E7
    assert es.search_lds_bytes(b) > es.LDS_BUDGET
    edge = slice_edge(8, 8 * order)
    rows = edge + 200
    # what the call needs on the device: the samples and the residual rows, the scratch at its cap, 33 + 32 doubles of
    # R[] and coefficients and a record per row
    need = 2 * rows * b * 4 + SCRATCH_CAP + rows * (65 * 8 + 368)
    assert need < 4 << 30
    x = distinct_rows(rows, b, bits, 3)
    cfg = _capi.make_config(lpc_order=order, flags=WS | OS)
    with _capi.Handle(0) as big:
        big.set_lpc_windows(extras)
        got = big.qlpc_batch(x, bits, cfg, want_fp=True)
        for lo in (0, edge - 128, rows - 256):
            small = big.qlpc_batch(x[lo:lo + 256], bits, cfg, want_fp=True)
            assert all(np.array_equal(g[lo:lo + 256], s_) for g, s_ in zip(got, small)), lo
    idx = [edge - 1, edge, rows - 1]
    es.check_rows(*(g[idx] for g in got), x[idx], bits, om.config(order=order), "out-of-LDS slice edge",
                  es.window_record(extras, True))


# ---- h: frames ----
def frame_cfg(order, flags, use_fixed, stereo=True, **kw):
    qlpc = _capi.make_config(lpc_order=order, flags=flags, **kw)
    return _capi.make_frame_config(qlpc, use_fixed=use_fixed, use_leftside=stereo, use_rightside=stereo,
                                   use_midside=stereo)


@pytest.mark.parametrize("orders", [False, True], ids=["P", "orders"])
@pytest.mark.parametrize("use_fixed", [False, True], ids=["lpc", "fixed"])
@pytest.mark.parametrize("n,bits,order,max_p", FRAME_CASES)
def test_worst_case_frames_equal_the_model_and_are_never_longer(h, n, bits, order, max_p, use_fixed, orders):
    rng = np.random.default_rng(9300 + n + order)
    x = es.extreme_frames(rng, n, bits)
    x[0] = np.stack([es.music(n, bits, start=n), es.music(n, bits, start=3 * n)])
    kw = dict(max_rice_parameter=max_p, window="rectangle", quant_precision=12)
    extras, flags = wc.E3, WS | (OS if orders else 0)
    model = wm.Model(extras, orders)
    h.set_lpc_windows(extras)
    fc = orc.make_frame_config(om.config(order=order, **kw), use_fixed=use_fixed)
    got = gpu_frames(h, frame_cfg(order, flags, use_fixed, **kw), x, bits)
    for f in range(len(x)):
        assert got[f] == model.stereo_frame_bytes(x[f, 0], x[f, 1], bits, fc, number=f), (n, bits, order, max_p, f)
    decode_check(h, got, x, bits)
    plain = gpu_frames(h, frame_cfg(order, REF, use_fixed, **kw), x, bits)
    assert all(len(g) <= len(p) for g, p in zip(got, plain))
    # independent channels: three per frame
    xc = np.concatenate([x[:3], x[3:]], 1)[:, :3]
    fci = orc.make_frame_config(om.config(order=order, **kw), use_fixed=use_fixed, use_leftside=False,
                                use_rightside=False, use_midside=False)
    gotc = gpu_frames(h, frame_cfg(order, flags, use_fixed, stereo=False, **kw), xc, bits, stereo=False)
    for f in range(len(xc)):
        assert gotc[f] == model.channel_frame_bytes(list(xc[f]), bits, fci, number=f), (n, bits, order, max_p, f)
    decode_check(h, gotc, xc, bits)
    plainc = gpu_frames(h, frame_cfg(order, REF, use_fixed, stereo=False, **kw), xc, bits, stereo=False)
    assert all(len(g) <= len(p) for g, p in zip(gotc, plainc))


@pytest.mark.parametrize("orders", [False, True], ids=["P", "orders"])
@pytest.mark.parametrize("use_fixed", [False, True], ids=["lpc", "fixed"])
@pytest.mark.parametrize("n,order,max_p", [(4096, 8, 30), (4096, 32, 2), (1000, 12, 0), (8192, 12, 14)])
def test_worst_case_frames_with_wasted_bits(h, n, order, max_p, use_fixed, orders):
    rng = np.random.default_rng(9400 + n + order)
    x = es.extreme_frames(rng, n, 16).astype(np.int64)
    for f in range(len(x)):
        x[f] <<= 1 + f  # shifted left by 1..6 bits
    x[-1, 0] <<= 2      # (and 8 bits in one channel: different k inside one frame)
    x = x.astype(np.int32)
    kw = dict(max_rice_parameter=max_p)
    extras, flags = wc.E3, WS | _capi.FLAG_WASTED_BITS | (OS if orders else 0)
    model = wm.Model(extras, orders)
    h.set_lpc_windows(extras)
    fc = orc.make_frame_config(om.config(order=order, **kw), use_fixed=use_fixed)
    got = gpu_frames(h, frame_cfg(order, flags, use_fixed, **kw), x, 24)
    for f in range(len(x)):
        assert got[f] == model.wasted_stereo_frame_bytes(x[f, 0], x[f, 1], 24, fc, number=f), (n, order, max_p, f)
    decode_check(h, got, x, 24)
    plain = gpu_frames(h, frame_cfg(order, REF | _capi.FLAG_WASTED_BITS, use_fixed, **kw), x, 24)
    assert all(len(g) <= len(p) for g, p in zip(got, plain))
