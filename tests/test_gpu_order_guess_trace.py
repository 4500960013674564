"""The guess of FLACENC_HIP_FLAG_ORDER_GUESS itself on the GPU: the per-window eligible count, mask and cost[] that
order_guess_kernel computes (order_guess_core.h, compiled for the device), read through
flacenc_hip_debug_set_order_guess_trace and held to tests/guess_model.py exactly -- eligible and mask as integers, the costs
as raw 64-bit patterns, +0.0 above the eligible count.  tests/test_gpu_order_guess.py compares the winning candidate only,
and (0, P) or a guess both sets share wins whatever the guess was; here a wrong width, block size, precision, k_o, log2f,
rounding, tie or trace index shows in the record of the window it happens in.  Every call also keeps the outcome's check
(records and residual rows, or the frames' bytes, against the model), so trace and outcome are held together.

The calls are tests/guess_trace_cases.py's (each first asserts from the model what it reaches; the same claims run
without a GPU in tests/test_order_guess_cpu.py) and the corpus of tests/guess_cases.py; then slices of a call past the
scratch bound, a seeded fuzz over shapes, widths, orders, both summation orders, the Rice switch, window lists and K, and
the hook's own hygiene.

Not reached: an infinite or NaN x_o = (float)(e_o / 2n).  e_o <= R[0] <= n (2^24)^2 for the widest subframe the ABI takes
(the side of 24-bit stereo, window weights at most 1), so x_o <= 2^47, far inside a float; largest_square comes within
a factor of two of that bound.  bits_per_sample's guard for such x is held on the host build only
(tests/test_order_guess_cpu.py).  A call that launches the search more than once (encode_variable, wasted bits with
unmarked frames) overwrites the trace and is not compared here."""
import numpy as np
import pytest
import torch

import extreme_signals as es
import guess_cases as gc
import guess_model as gm
import guess_trace_cases as tc
import order_model as om
import window_cases as wc
import window_model as wm
from flacenc_rs_amd import _capi
from oracle import oracle as orc
from test_gpu_order_guess import SCRATCH_CAP, check_stereo, gcfg, guess_record, state
from test_gpu_order_search import gpu_channels
from test_gpu_order_search_extremes import fuzz_trial
from test_gpu_window_search_extremes import distinct_rows

pytestmark = pytest.mark.gpu
TRACE = _capi.ORDER_GUESS_TRACE_DTYPE
WS = _capi.FLAG_WINDOW_SEARCH
OS = _capi.FLAG_ORDER_SEARCH
WASTED = _capi.FLAG_WASTED_BITS


@pytest.fixture(scope="module")
def h():
    with _capi.Handle(0, hooks=True) as handle:
        yield handle


class traced:
    """A device buffer of n_sub x W trace records, every byte 0xFF, set on the handle for one block."""

    def __init__(self, handle, n_sub, W):
        self.h, self.shape = handle, (n_sub, W)
        self.buf = torch.full((n_sub * W * TRACE.itemsize,), 0xFF, dtype=torch.uint8, device="cuda")

    def __enter__(self):
        torch.cuda.synchronize()
        self.h.debug_set_order_guess_trace(self.buf.data_ptr())
        return self

    def __exit__(self, *exc):
        self.h.debug_set_order_guess_trace(0)

    def read(self):
        torch.cuda.synchronize()
        return self.buf.cpu().numpy().view(TRACE).reshape(self.shape)


def model_trace(found):
    """The trace records of gm.search(...)[2] per subframe."""
    out = np.zeros((len(found), len(found[0])), TRACE)
    for i, per_window in enumerate(found):
        assert len(per_window) == out.shape[1]
        for j, g in enumerate(per_window):
            out[i, j]["eligible"], out[i, j]["mask"] = g["eligible"], tc.mask_of(g)
            out[i, j]["cost"][:g["eligible"]] = g["cost"]
    return out


def check_trace(got, want, where):
    assert got.shape == want.shape, where
    for idx in np.ndindex(*got.shape):
        g, w = got[idx], want[idx]
        at = (where, "subframe %d window %d" % idx)
        assert int(g["eligible"]) == int(w["eligible"]), at + (int(g["eligible"]), int(w["eligible"]))
        assert int(g["mask"]) == int(w["mask"]), at + (hex(int(g["mask"])), hex(int(w["mask"])))
        gc_, wc_ = g["cost"].view(np.uint64), w["cost"].view(np.uint64)
        assert np.array_equal(gc_, wc_), at + (g["cost"].tolist(), w["cost"].tolist())


def ofc(c):
    return tc.frame_config(c)


def run(hh, c, found):
    """Call c through its entry point with the trace set: the outcome and the trace against the model."""
    extras = c.extras
    qcfg = gcfg(c.order, windows=bool(extras), quant_precision=c.q, **c.kw)
    ocfg = tc.config(c)
    n_sub, W = len(tc.subframes(c)), 1 + len(extras)
    x = c.rows
    with state(hh, c.K, extras if extras else None), traced(hh, n_sub, W) as t:
        if c.entry == "batch":
            got = hh.qlpc_batch(x, c.bps, qcfg, want_fp=True)
            trace = t.read()
            es.check_rows(*got, x, c.bps, ocfg, c.name, guess_record(c.K, extras))
        elif c.entry == "stereo":
            sp, sr = hh.stereo_qlpc_batch(x, c.bps, qcfg)
            trace = t.read()
            check_stereo(sp, sr, x, c.bps, ocfg, c.K, extras)
        elif c.entry == "stereo_frames":
            fcfg = _capi.make_frame_config(qcfg, use_fixed=True, use_leftside=True, use_rightside=True, use_midside=True)
            res, resid = hh.encode_stereo_frames(x, c.bps, fcfg)
            trace = t.read()
            packed = hh.pack_stereo_frames(x, res, resid, c.bps, 44100)
            model = gm.Model(c.K, extras)
            for f in range(len(x)):
                assert packed[f] == model.stereo_frame_bytes(x[f, 0], x[f, 1], c.bps, ofc(c), number=f), (c.name, f)
        else:
            wcfg = gcfg(c.order, WASTED, windows=bool(extras), quant_precision=c.q, **c.kw)
            fcfg = _capi.make_frame_config(wcfg, use_fixed=True, use_leftside=False, use_rightside=False,
                                           use_midside=False)
            hh.encode_frames(x, c.bps, fcfg)
            trace = t.read()
            got = gpu_channels(hh, fcfg, x, c.bps)
            assert np.array_equal(t.read(), trace), c.name  # (the fused entry point runs the same search)
            model = gm.Model(c.K, extras)
            assert got[0] == model.wasted_channel_frame_bytes(list(x[0]), c.bps, ofc(c), number=0), c.name
    check_trace(trace, model_trace(found), c.name)


# ---- a - e: the deterministic calls ----
CORPUS = [tc.corpus_call(c) for c in gc.all_cases()]
CALLS = tc.all_calls()


@pytest.mark.parametrize("c", CORPUS, ids=tc.ids(CORPUS))
def test_corpus_traces_equal_the_model(h, c):
    run(h, c, tc.claims(c))


@pytest.mark.parametrize("c", CALLS, ids=tc.ids(CALLS))
def test_call_traces_equal_the_model(h, c):
    run(h, c, tc.claims(c))


def test_the_calls_take_every_log2f_table_index():
    assert tc.log2f_indices(CALLS) == set(range(16))


# ---- f: slices ----
def slice_shape():
    b, order, K = 256, 32, 2
    per = 8 * 264 + 8 * order * (144 + 8) + 4
    edge = (SCRATCH_CAP // per) & ~3
    return b, order, K, per, edge


def boundary_rows(edge, last):
    return [0, edge - 1, edge, edge + 1, edge + 3, last]


def test_stereo_slices_trace_their_own_subframes():
    b, order, K, per, edge = slice_shape()
    bits, extras = 16, wc.E7
    nf = edge // 4 + 150
    assert 4 * nf * per > SCRATCH_CAP and edge % 4 == 0
    x = distinct_rows(2 * nf, b, bits, 1).reshape(nf, 2, b)
    ocfg = om.config(order=order)
    found = {}
    for sf in boundary_rows(edge, 4 * nf - 1):
        f, k = divmod(sf, 4)
        m, s = orc.stereo_to_midside(x[f, 0], x[f, 1])
        found[sf] = ((x[f, 0], x[f, 1], m, s)[k], bits + (1 if k == 3 else 0))
    found = {sf: (sig, w, gm.search(sig, w, ocfg, K, extras)[2]) for sf, (sig, w) in found.items()}
    want = {sf: model_trace([per_window]) for sf, (_, _, per_window) in found.items()}
    # a trace indexed within the slice would put subframe `edge` where subframe 0 belongs: the two differ
    assert want[edge].tobytes() != want[0].tobytes()
    with _capi.Handle(0, hooks=True) as big, traced(big, 4 * nf, 8) as t:
        big.set_lpc_windows(extras)
        big.set_order_guesses(K)
        params, residual = big.stereo_qlpc_batch(x, bits, gcfg(order, windows=True))
        trace = t.read()
    for sf, (sig, w, _) in found.items():
        f, k = divmod(sf, 4)
        rec, resid, _, _ = gm.record(sig, w, ocfg, K, extras)
        assert int(params[f, k]["status"]) == 0 and es.params_record(params[f, k]) == rec, (sf, f, k)
        assert np.array_equal(residual[f, k], resid), (sf, f, k)
        check_trace(trace[sf:sf + 1], want[sf], ("stereo slices", sf))


def test_mono_slices_trace_their_own_bits_per_sample():
    # bps cycles 16, 17, 24, 25 from row to row, and a slice starts at a multiple of 4 subframes: the phase moves by one
    # at the first boundary, so every row of the second slice differs in width from the row a missing offset would read
    b, order, K, per, edge = slice_shape()
    extras = wc.E7
    rows = edge + 600
    assert rows * per > SCRATCH_CAP
    x = distinct_rows(rows, b, 16, 2)
    i = np.arange(rows)
    bpsv = np.array([16, 17, 24, 25], np.uint8)[(i + (i >= edge)) % 4]
    assert all(bpsv[edge + d] != bpsv[d] for d in range(4))
    ocfg = om.config(order=order)
    idx = boundary_rows(edge, rows - 1)
    found = [gm.search(x[sf], int(bpsv[sf]), ocfg, K, extras)[2] for sf in idx]
    want = model_trace(found)
    assert want[idx.index(edge)].tobytes() != want[0].tobytes()
    # ... and the width shows in every eligible cost: the row past the boundary at the width of row 0 gives other costs
    other = model_trace([gm.search(x[edge], int(bpsv[0]), ocfg, K, extras)[2]])
    assert other.tobytes() != want[idx.index(edge)].tobytes()
    with _capi.Handle(0, hooks=True) as big, traced(big, rows, 8) as t:
        big.set_lpc_windows(extras)
        big.set_order_guesses(K)
        got = big.qlpc_batch(x, bpsv, gcfg(order, windows=True), want_fp=True)
        trace = t.read()
    es.check_rows(*(g[idx] for g in got), x[idx], bpsv[idx], ocfg, "bps slice edge", guess_record(K, extras))
    check_trace(trace[idx], want, ("mono slices", idx))


# ---- g: a seeded fuzz ----
def guess_fuzz_trial(rng):
    """fuzz_trial of the order-search suite + a random extra-window list and K."""
    x, bpsv, order, nightly, finest, kw = fuzz_trial(rng)
    extras = wm.random_extras(rng, x.shape[1])
    K = int(rng.choice([1, 2, 3, order, 32]))
    return x, bpsv, order, nightly, finest, kw, extras, K


@pytest.mark.parametrize("seed", range(8))
def test_configuration_fuzz(h, seed):
    rng = np.random.default_rng(10100 + seed)
    for trial in range(4):
        x, bpsv, order, nightly, finest, kw, extras, K = guess_fuzz_trial(rng)
        tag = (seed, trial, x.shape, bpsv.tolist(), order, nightly, finest, kw, extras, K)
        flags = (_capi.FLAG_NIGHTLY_SUM_ORDER if nightly else 0) | (_capi.FLAG_FINEST_RICE_ORDER if finest else 0)
        ocfg = om.config(order=order, nightly=nightly, rice_finest_only=finest, **kw)
        try:
            # (the window flag with an empty list too: the call then searches one window)
            with state(h, K, extras), traced(h, len(x), 1 + len(extras)) as t:
                got = h.qlpc_batch(x, bpsv, gcfg(order, flags, windows=True, **kw), want_fp=True)
                trace = t.read()
            es.check_rows(*got, x, bpsv, ocfg, "fuzz", guess_record(K, extras))
            found = [gm.search(x[i], int(bpsv[i]), ocfg, K, extras)[2] for i in range(len(x))]
            check_trace(trace, model_trace(found), "fuzz")
        except AssertionError as e:
            raise AssertionError(f"configuration {tag}: {e}") from e


# ---- h: the hook's hygiene ----
def test_the_hook_changes_no_output_and_unflagged_calls_store_nothing(h):
    b, order, K = 256, 12, 2
    x = np.stack([es.music(b, 16, start=(i + 40) * b) for i in range(8)]).astype(np.int32)
    frames = x.reshape(4, 2, b)
    cfg = gcfg(order, windows=True)

    def outputs(hh):
        return hh.qlpc_batch(x, 16, cfg, want_fp=True) + hh.stereo_qlpc_batch(frames, 16, cfg)

    with _capi.Handle(0) as never:
        never.set_order_guesses(K)
        want = outputs(never)
    W = 1 + len(wm.DEFAULT)
    with state(h, K):
        with traced(h, 16, W) as t:
            hooked = outputs(h)
            filled = t.read().copy()
            assert not np.any(filled["eligible"] == 0xFFFFFFFF)  # (every record of the stereo call's 16 x W written)
            t.buf.zero_()
            torch.cuda.synchronize()
            # calls without the flag, the hook still set: the plain call, the exhaustive searches
            h.qlpc_batch(x, 16, _capi.make_config(lpc_order=order), want_fp=True)
            h.qlpc_batch(x, 16, _capi.make_config(lpc_order=order, flags=OS | WS), want_fp=True)
            h.stereo_qlpc_batch(frames, 16, _capi.make_config(lpc_order=order, flags=WS))
            assert not np.any(t.read().view(np.uint8))
        unhooked = outputs(h)
    for a, b_, c in zip(want, hooked, unhooked):
        assert a.tobytes() == b_.tobytes() == c.tobytes()
