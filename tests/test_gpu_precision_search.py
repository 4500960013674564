"""FLACENC_HIP_FLAG_PRECISION_SEARCH on the GPU: candidate records, residual rows, R[] and coefficients equal the model's
(tests/precision_model.py) byte for byte across block sizes, order buckets, widths, floors and quant_precision, alone and
with the order search, the window search, both, and the order guess (whose trace does not move); rows whose two best
precisions tie take the higher one; frames equal the model's bytes, decode back to their input and are never longer than
the REFERENCE_SUM_ORDER frames or the same call without the flag; a floor at or above quant_precision is the call without
the flag; the floor behaves as handle state should; big calls run in slices; the refused configs are refused.

Every equality case also asserts that a row of its own chose a precision below quant_precision: where the flag's bit is
ignored the records carry quant_precision everywhere and the case fails."""
import numpy as np
import pytest
import torch

import extreme_signals as es
import flac_parse
import order_model as om
import precision_model as pm
import window_model as wm
from extreme_signals import alternation, extreme_frames, noise
from flacenc_rs_amd import _capi
from oracle import oracle as orc
from test_gpu_order_search import content, decode_check, gpu_channels, gpu_stereo
from test_gpu_variable_block import check as variable_check

pytestmark = pytest.mark.gpu
PS = _capi.FLAG_PRECISION_SEARCH
OS = _capi.FLAG_ORDER_SEARCH
WS = _capi.FLAG_WINDOW_SEARCH
OG = _capi.FLAG_ORDER_GUESS
REF = _capi.FLAG_REFERENCE_SUM_ORDER
NIGHTLY = _capi.FLAG_NIGHTLY_SUM_ORDER
FINEST = _capi.FLAG_FINEST_RICE_ORDER
CANON = _capi.FLAG_CANONICAL_SUM_ORDER
WASTED = _capi.FLAG_WASTED_BITS
SCRATCH_CAP = 768 << 20  # kSearchScratchCap
TRACE = _capi.ORDER_GUESS_TRACE_DTYPE

# the other search flags of a case: name -> (flags, extra windows of the model, orders, K)
SEARCHES = {"": (0, (), False, 0), "os": (OS, (), True, 0), "ws": (WS, wm.DEFAULT, False, 0),
            "os+ws": (OS | WS, wm.DEFAULT, True, 0), "g1": (OG, (), False, 1), "g2": (OG, (), False, 2),
            "g2+ws": (OG | WS, wm.DEFAULT, False, 2)}


@pytest.fixture(scope="module")
def h():
    with _capi.Handle(0) as handle:
        yield handle


class state:
    """The floor (and K) on a handle for one block; a fresh handle's values afterwards."""

    def __init__(self, handle, floor, K=0):
        self.h, self.floor, self.K = handle, floor, K

    def __enter__(self):
        self.h.set_precision_floor(self.floor)
        if self.K:
            self.h.set_order_guesses(self.K)
        return self.h

    def __exit__(self, *exc):
        self.h.set_precision_floor(pm.DEFAULT_FLOOR)
        self.h.set_order_guesses(1)


def pcfg(order, flags=0, q=15, search=True, **kw):
    return _capi.make_config(lpc_order=order, quant_precision=q, flags=(PS if search else 0) | flags, **kw)


def ocfg(order, q=15, nightly=False, finest=False):
    return om.config(order=order, nightly=nightly, quant_precision=q, rice_finest_only=finest)


def with_silence(x):
    """The rows with their first half (a third on odd rows) digital silence."""
    x = x.copy()
    x[::2, : x.shape[1] // 2] = 0
    x[1::2, : x.shape[1] // 3] = 0
    return x


def material(kind, rows, b, bits, start):
    if kind == "extreme":  # (alternation and noise take stage 3's marked clean-up on the big-block shapes)
        x = np.stack([alternation(b, bits), noise(b, bits, 3), np.zeros(b, np.int64),
                      np.r_[np.zeros(b // 2), alternation(b - b // 2, bits)]])
        return x[:rows].astype(np.int32)
    x = content(rows, b, bits, start=start)
    return with_silence(x) if kind == "silence" else x


def searched_below(params, q0, x=None):
    """A row with status 0 (of x: one that is not digital silence) chose a precision below q0: not the unflagged call's
    record."""
    p = np.asarray(params).reshape(-1)
    loud = np.ones(len(p), bool) if x is None else np.any(np.asarray(x).reshape(len(p), -1) != 0, axis=1)
    return bool(np.any((p["status"] == 0) & (p["precision"] < q0) & loud))


# ---- 1. records against the model ----
BATCH_CASES = [
    # (block, order, bits, q0, floor, the other search flags, material)
    (64, 8, 16, 15, 5, "", "music"), (100, 12, 16, 12, 1, "os", "silence"), (256, 8, 8, 15, 14, "", "music"),
    (256, 12, 16, 6, 1, "ws", "music"), (1152, 12, 24, 15, 5, "os+ws", "music"), (1152, 8, 16, 12, 11, "g1", "silence"),
    (4096, 1, 16, 15, 5, "", "music"), (4096, 8, 16, 15, 1, "", "silence"), (4096, 12, 16, 15, 5, "g2", "music"),
    (4096, 16, 16, 15, 5, "os", "music"), (4096, 32, 24, 15, 5, "", "music"), (4096, 8, 16, 6, 5, "ws", "music"),
    (4096, 12, 24, 15, 14, "g2+ws", "music"), (4608, 12, 16, 15, 5, "", "music"), (8192, 32, 24, 15, 14, "", "silence"),
    (16384, 8, 16, 15, 5, "", "music"), (20000, 8, 16, 15, 1, "", "music"), (20000, 32, 24, 15, 5, "", "music"),
    (4096, 32, 16, 15, 5, "", "extreme"), (1152, 24, 24, 15, 5, "", "extreme"), (8192, 12, 16, 15, 5, "os", "extreme"),
    (16384, 8, 24, 6, 1, "", "extreme"),
]


@pytest.mark.parametrize("b,order,bits,q0,floor,search,kind", BATCH_CASES)
def test_candidate_batch_equals_the_model(h, b, order, bits, q0, floor, search, kind):
    flags, extras, orders, K = SEARCHES[search]
    x = material(kind, 4 if b <= 4608 else 2, b, bits, 3 * b)
    with state(h, floor, K):
        got = h.qlpc_batch(x, bits, pcfg(order, flags, q0), want_fp=True)
    es.check_rows(*got, x, bits, ocfg(order, q0), (b, order, bits, q0, floor, search, kind),
                  pm.record_fn(floor, extras, orders, K))
    assert searched_below(got[0], q0, x)


@pytest.mark.parametrize("b,order,flags,finest,nightly,search", [
    (4096, 8, FINEST, True, False, ""), (1152, 12, FINEST, True, False, "os"), (2048, 15, NIGHTLY, False, True, ""),
    (2048, 15, NIGHTLY, False, True, "os"), (4096, 8, REF, False, False, ""), (4096, 8, CANON, False, False, ""),
    (4096, 8, REF | _capi.FLAG_INTEGER_PARITY_ONLY, False, False, ""), (4096, 12, CANON, False, False, "g1"),
])
def test_candidate_batch_under_other_flags(h, b, order, flags, finest, nightly, search):
    more, extras, orders, K = SEARCHES[search]
    x = content(4, b, 16, start=5 * b)
    with state(h, pm.DEFAULT_FLOOR, K):
        got = h.qlpc_batch(x, 16, pcfg(order, flags | more), want_fp=True)
        if flags & (CANON | _capi.FLAG_INTEGER_PARITY_ONLY | REF):  # ... change nothing
            same = h.qlpc_batch(x, 16, pcfg(order, more), want_fp=True)
            assert all(np.array_equal(g, s) for g, s in zip(got, same))
    es.check_rows(*got, x, 16, ocfg(order, nightly=nightly, finest=finest), (b, order, flags, search),
                  pm.record_fn(pm.DEFAULT_FLOOR, extras, orders, K))
    assert searched_below(got[0], 15)


def test_per_row_bits_per_sample_enter_the_key(h):
    b, order = 1152, 12
    x = content(4, b, 16, start=5 * b)
    bps = np.array([16, 25, 17, 20], np.uint8)
    got = h.qlpc_batch(x, bps, pcfg(order, OS), want_fp=True)
    es.check_rows(*got, x, bps, ocfg(order), "per-row bps", pm.record_fn(orders=True))
    assert searched_below(got[0], 15)


class traced:
    """A device buffer of n_sub x W order-guess trace records, every byte 0xFF, set on the handle for one block."""

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
        return self.buf.cpu().numpy().copy()


@pytest.mark.parametrize("K,windows", [(1, False), (2, True)])
def test_the_order_guess_trace_is_that_of_the_call_without_the_flag(K, windows):
    b, order = 4096, 12
    x = content(4, b, 16, start=7 * b)
    flags, W = (OG | WS, 6) if windows else (OG, 1)
    with _capi.Handle(0, hooks=True) as hh:
        hh.set_order_guesses(K)
        with traced(hh, len(x), W) as t:
            plain = hh.qlpc_batch(x, 16, pcfg(order, flags, search=False))
            want = t.read()
        with traced(hh, len(x), W) as t:
            got = hh.qlpc_batch(x, 16, pcfg(order, flags))
            trace = t.read()
    assert np.array_equal(trace, want) and not (want == 0xFF).all()
    assert searched_below(got[0], 15) and not searched_below(plain[0], 15)
    assert (got[0]["subframe_bits"] <= plain[0]["subframe_bits"]).all()


# ---- 2. the tie rule ----
def tied_rows():
    """64-sample random walks on which the two (or more) shortest candidates are precisions of one (0, P): found by
    scanning seeds with the model; the premise is asserted from the model again where they are used."""
    rows = []
    for order, seed in ((1, 4), (1, 17), (1, 41), (1, 39)):
        rng = np.random.default_rng(seed)
        rows.append((order, (rng.integers(-300, 301, 64).cumsum() // 2).clip(-32768, 32767).astype(np.int32)))
    return rows


def test_tied_precisions_take_the_higher_one(h):
    for order, x in tied_rows():
        cfg = ocfg(order)
        best, cands = pm.search(x, 16, cfg, 1)
        tied = [c["q"] for c in cands if c["status"] == 0 and c["subframe_bits"] == best["subframe_bits"]]
        assert len(tied) >= 2 and best["q"] == max(tied) < 15, (order, tied)
        with state(h, 1):
            got = h.qlpc_batch(x[None, :], 16, pcfg(order), want_fp=True)
        es.check_rows(*got, x[None, :], 16, cfg, ("tie", order, tied), pm.record_fn(1))
        assert int(got[0][0]["precision"]) == max(tied)


# ---- 3. stereo and frames ----
@pytest.mark.parametrize("b,order,bits,search", [(4096, 8, 16, ""), (1152, 12, 24, "os"), (8192, 32, 24, "")])
def test_stereo_batch_equals_the_model_with_the_side_channel(h, b, order, bits, search):
    flags, extras, orders, K = SEARCHES[search]
    x = with_silence(content(4, b, bits, start=7 * b)).reshape(2, 2, b)
    params, residual = h.stereo_qlpc_batch(x, bits, pcfg(order, flags))
    cfg = ocfg(order)
    for f in range(len(x)):
        m, s = orc.stereo_to_midside(x[f, 0], x[f, 1])
        for k, sig in enumerate((x[f, 0], x[f, 1], m, s)):
            rec, resid, _, _ = pm.record(sig, bits + (1 if k == 3 else 0), cfg, pm.DEFAULT_FLOOR, extras, orders, K)
            assert int(params[f, k]["status"]) == rec["status"] == 0, (f, k)
            assert es.params_record(params[f, k]) == rec, (f, k)
            assert np.array_equal(residual[f, k], resid), (f, k)
    assert searched_below(params, 15)


def frame_cfg(order, flags=0, q=15, stereo=True, search=True):
    return _capi.make_frame_config(pcfg(order, flags, q, search), use_fixed=True, use_leftside=stereo,
                                   use_rightside=stereo, use_midside=stereo)


def ofc(order, q=15, stereo=True):
    return orc.make_frame_config(ocfg(order, q), use_leftside=stereo, use_rightside=stereo, use_midside=stereo)


def parse_check(frames, x, bps, wasted_ok=False):
    """Every frame decodes to its input with the test-side parser."""
    for f, fr in enumerate(frames):
        p = flac_parse.parse_frame(fr, stream_bps=bps, stream_rate=44100, wasted_ok=wasted_ok)
        assert p["length"] == len(fr) and np.array_equal(p["channels"], x[f]), f


@pytest.mark.parametrize("b,order,bits,search", [(4096, 8, 16, ""), (4096, 12, 24, "os"), (4608, 8, 16, ""),
                                                 (1152, 12, 24, "ws"), (256, 8, 16, "g2"), (8192, 32, 24, ""),
                                                 (63, 8, 16, ""), (1000, 8, 16, "os")])
def test_stereo_frame_bytes_equal_the_model(h, b, order, bits, search):
    flags, extras, orders, K = SEARCHES[search]
    x = with_silence(content(6, b, bits, start=9 * b)).reshape(3, 2, b)
    with state(h, pm.DEFAULT_FLOOR, K):
        cfg = frame_cfg(order, flags)
        got = gpu_stereo(h, cfg, x, bits)
        res, resid = h.encode_stereo_frames(x, bits, cfg)
        assert h.pack_stereo_frames(x, res, resid, bits, 44100) == got
        plain = gpu_stereo(h, frame_cfg(order, flags or REF, search=False), x, bits)
    model = pm.Model(pm.DEFAULT_FLOOR, extras, orders, K)
    for f in range(len(x)):
        assert got[f] == model.stereo_frame_bytes(x[f, 0], x[f, 1], bits, ofc(order), number=f), (b, order, f)
    decode_check(h, got, x, bits)
    parse_check(got, x, bits)
    assert all(len(g) <= len(p) for g, p in zip(got, plain))
    if b >= 64:  # (a shorter block has no LPC candidate: the flag changes nothing there)
        assert got != plain and sum(map(len, got)) < sum(map(len, plain))
    else:
        assert got == plain


@pytest.mark.parametrize("C,b,order", [(1, 4096, 8), (3, 1152, 12), (8, 256, 8)])
def test_independent_frame_bytes_equal_the_model(h, C, b, order):
    x = content(2 * C, b, 16, start=11 * b).reshape(2, C, b)
    cfg = frame_cfg(order, stereo=False)
    got = gpu_channels(h, cfg, x, 16)
    res, resid = h.encode_frames(x, 16, cfg)
    assert h.pack_frames(x, res, resid, 16, 44100) == got
    model = pm.Model()
    for f in range(len(x)):
        assert got[f] == model.channel_frame_bytes(list(x[f]), 16, ofc(order, stereo=False), number=f), (C, b, f)
    decode_check(h, got, x, 16)
    parse_check(got, x, 16)
    assert got != gpu_channels(h, frame_cfg(order, REF, stereo=False, search=False), x, 16)


def test_extreme_frames_equal_the_model_and_decode(h):
    x = extreme_frames(np.random.default_rng(11), 1152, 16)[:4]
    got = gpu_stereo(h, frame_cfg(12), x, 16)
    model = pm.Model()
    for f in range(len(x)):
        assert got[f] == model.stereo_frame_bytes(x[f, 0], x[f, 1], 16, ofc(12), number=f), f
    decode_check(h, got, x, 16)
    parse_check(got, x, 16)
    # (these frames keep few LPC subframes; the candidates behind them did search)
    assert searched_below(h.stereo_qlpc_batch(x, 16, pcfg(12))[0], 15, np.stack([x[:, 0], x[:, 1], x[:, 0], x[:, 1]], 1))


# ---- 4. other paths ----
def shifted_frames(b):
    """16-bit music in a 24-bit container: every row shifted by 8 bits, one by 4 more, one frame left at full width."""
    x = content(8, b, 16, start=b).reshape(4, 2, b).astype(np.int64) << 8
    x[2, 0] >>= 4
    x[3] = content(2, b, 24, start=2 * b)
    return x.astype(np.int32)


@pytest.mark.parametrize("b,order,search", [(4096, 8, ""), (1152, 12, "os"), (4096, 12, "g2")])
def test_stereo_frames_with_wasted_bits_equal_the_model(h, b, order, search):
    flags, extras, orders, K = SEARCHES[search]
    x = shifted_frames(b)
    with state(h, pm.DEFAULT_FLOOR, K):
        got = gpu_stereo(h, frame_cfg(order, WASTED | flags), x, 24)
        plain = gpu_stereo(h, frame_cfg(order, WASTED | (flags or REF), search=False), x, 24)
    model = pm.Model(pm.DEFAULT_FLOOR, extras, orders, K)
    for f in range(len(x)):
        assert got[f] == model.wasted_stereo_frame_bytes(x[f, 0], x[f, 1], 24, ofc(order), number=f), f
    decode_check(h, got, x, 24)
    parse_check(got, x, 24, wasted_ok=True)
    assert all(len(g) <= len(p) for g, p in zip(got, plain)) and got != plain


def test_independent_frames_with_wasted_bits_equal_the_model(h):
    b, order = 1152, 12
    x = shifted_frames(b)[:, :1].repeat(3, axis=1)
    x[:, 1] = shifted_frames(b)[:, 1]
    x[:, 2] >>= 2
    got = gpu_channels(h, frame_cfg(order, WASTED, stereo=False), x, 24)
    model = pm.Model()
    for f in range(len(x)):
        assert got[f] == model.wasted_channel_frame_bytes(list(x[f]), 24, ofc(order, stereo=False), number=f), f
    decode_check(h, got, x, 24)
    assert got != gpu_channels(h, frame_cfg(order, WASTED | REF, stereo=False, search=False), x, 24)


def test_encode_pcm_stereo_equals_the_device_call_across_a_chunk_seam():
    b, nf = 1152, 5
    x = content(2 * nf, b, 16, start=2 * b).reshape(2, nf * b)
    pcm = np.ascontiguousarray(x.T.astype("<i2")).view(np.uint8).reshape(-1)
    cfg = frame_cfg(12)
    ref = np.ascontiguousarray(x.reshape(2, nf, b).transpose(1, 0, 2))
    with _capi.Handle(0, hooks=True) as hh:
        hh.debug_set_stream_chunk(2)
        data, lens = hh.encode_pcm_stereo(pcm, cfg, 2, 16, b, 44100)
        assert hh.debug_last_stream_plan() == (2, 3)  # frames 0-1, 2-3, 4: two seams
        hh.debug_set_stream_chunk(0)
        frames, off = [], 0
        for ln in lens:
            frames.append(bytes(data[off:off + ln]))
            off += ln
        assert frames == gpu_stereo(hh, cfg, ref, 16)
        plain = gpu_stereo(hh, frame_cfg(12, REF, search=False), ref, 16)
        decode_check(hh, frames, ref, 16)
    model = pm.Model()
    for f in (1, 2, 4):  # either side of the first seam, and the last chunk
        assert frames[f] == model.stereo_frame_bytes(ref[f, 0], ref[f, 1], 16, ofc(12), number=f), f
    parse_check(frames, ref, 16)
    assert frames != plain and all(len(g) <= len(p) for g, p in zip(frames, plain))


@pytest.mark.parametrize("levels", [1, 2])
def test_encode_variable_keeps_the_fixed_paths_bodies_and_is_never_longer(h, levels):
    S = 4096
    x = content(8, S, 16, start=9 * S).reshape(4, 2, S)
    total = 4 * S - 333
    got = variable_check(h, frame_cfg(8), x, total, S, levels, 16)  # (decodes; every body is the fixed call's)
    plain = h.encode_variable(x, 16, frame_cfg(8, REF, search=False), levels, total_samples=total, block_size=S)
    assert not plain["overflow"] and got["bytes"] < plain["bytes"]
    both = h.encode_variable(x, 16, frame_cfg(8, OS), levels, total_samples=total, block_size=S)
    os_only = h.encode_variable(x, 16, frame_cfg(8, OS, search=False), levels, total_samples=total, block_size=S)
    assert both["bytes"] <= os_only["bytes"]


# ---- 5. never longer, a floor at or above quant_precision, the floor as state ----
@pytest.mark.parametrize("b,order,bits", [(4096, 8, 16), (4096, 12, 24), (1152, 8, 16), (8192, 32, 16), (256, 12, 16)])
def test_flagged_frames_are_never_longer(h, b, order, bits):
    x = content(16, b, bits).reshape(8, 2, b)
    plain = gpu_stereo(h, frame_cfg(order, REF, search=False), x, bits)
    got = gpu_stereo(h, frame_cfg(order), x, bits)
    assert all(len(g) <= len(p) for g, p in zip(got, plain)) and sum(map(len, got)) < sum(map(len, plain))
    for other in (OS, WS, OG):
        without = gpu_stereo(h, frame_cfg(order, other, search=False), x, bits)
        both = gpu_stereo(h, frame_cfg(order, other), x, bits)
        assert all(len(g) <= len(p) for g, p in zip(both, without)), other
        assert sum(map(len, both)) < sum(map(len, without)), other


@pytest.mark.parametrize("flags", [0, NIGHTLY, FINEST, CANON, OS, WS, OG])
@pytest.mark.parametrize("q0,floor", [(15, 15), (12, 13), (5, 5)])
def test_a_floor_at_or_above_the_precision_is_the_call_without_the_flag(flags, q0, floor):
    b, order = 4096, 12
    x = content(8, b, 16, start=13 * b)
    in_place = flags & ~CANON
    if not flags & (OS | WS | OG | NIGHTLY):
        in_place |= REF
    with _capi.Handle(0) as h0:
        if q0 != 5:  # (5: a fresh handle's floor)
            h0.set_precision_floor(floor)
        got = h0.qlpc_batch(x, 16, pcfg(order, flags, q0), want_fp=True)
        ref = h0.qlpc_batch(x, 16, pcfg(order, in_place, q0, search=False), want_fp=True)
        assert all(np.array_equal(g, r) for g, r in zip(got, ref))
        assert (got[0]["precision"][got[0]["status"] == 0] == q0).all()
        fr = x.reshape(4, 2, b)
        assert gpu_stereo(h0, frame_cfg(order, flags, q0), fr, 16) == \
            gpu_stereo(h0, frame_cfg(order, in_place, q0, search=False), fr, 16)
        assert gpu_channels(h0, frame_cfg(order, flags, q0, stereo=False), fr, 16) == \
            gpu_channels(h0, frame_cfg(order, in_place, q0, stereo=False, search=False), fr, 16)
        if q0 == 15:  # one precision lower and the flag acts (on these rows: 14 bits beat 15)
            h0.set_precision_floor(14)
            assert searched_below(h0.qlpc_batch(x, 16, pcfg(order, flags, q0))[0], q0)


def test_the_floor_is_handle_state():
    b, order = 1152, 12
    x = content(4, b, 16, start=17 * b)
    cfg, oc = pcfg(order), ocfg(order)
    plain_cfg = _capi.make_config(lpc_order=order)
    with _capi.Handle(0) as fresh, _capi.Handle(0) as other:
        u0 = fresh.qlpc_batch(x, 16, plain_cfg, want_fp=True)
        o0 = fresh.qlpc_batch(x, 16, _capi.make_config(lpc_order=order, flags=OS), want_fp=True)
        f5 = fresh.qlpc_batch(x, 16, cfg, want_fp=True)
        es.check_rows(*f5, x, 16, oc, "fresh: floor 5", pm.record_fn(5))
        fresh.set_precision_floor(13)
        f13 = fresh.qlpc_batch(x, 16, cfg, want_fp=True)
        es.check_rows(*f13, x, 16, oc, "floor 13", pm.record_fn(13))
        assert (f13[0]["precision"] >= 13).all() and searched_below(f13[0], 15)
        assert not np.array_equal(f5[0], f13[0])  # (the floor changes these rows' records: the setter is seen to act)
        es.check_rows(*other.qlpc_batch(x, 16, cfg, want_fp=True), x, 16, oc, "another handle", pm.record_fn(5))
        for bad in (0, 16, 1 << 31):
            with pytest.raises(_capi.FlacencHipError) as e:
                fresh.set_precision_floor(bad)
            assert e.value.code == _capi.ERR_BAD_ARGUMENT
        again = fresh.qlpc_batch(x, 16, cfg, want_fp=True)  # a refused setter keeps the value; it survives calls
        assert all(np.array_equal(p, q) for p, q in zip(again, f13))
        # without the flag no byte changes with the floor
        for cfg0, before in ((plain_cfg, u0), (_capi.make_config(lpc_order=order, flags=OS), o0)):
            now = fresh.qlpc_batch(x, 16, cfg0, want_fp=True)
            assert all(np.array_equal(p, q) for p, q in zip(before, now))
        fr = x.reshape(2, 2, b)
        assert gpu_stereo(fresh, frame_cfg(order, OS, search=False), fr, 16) == \
            gpu_stereo(other, frame_cfg(order, OS, search=False), fr, 16)
        fresh.set_precision_floor(1)
        es.check_rows(*fresh.qlpc_batch(x, 16, cfg, want_fp=True), x, 16, oc, "floor 1", pm.record_fn(1))
        fresh.set_precision_floor(5)
        back = fresh.qlpc_batch(x, 16, cfg, want_fp=True)
        assert all(np.array_equal(p, q) for p, q in zip(back, f5))


# ---- 6. refusals ----
def test_direct_mse_with_the_flag_is_refused(h):
    x = content(2, 4096, 16)
    fr = x.reshape(1, 2, 4096)
    for more in (0, OS, WS, OG):
        kw = dict(use_direct_mse=True)
        calls = (lambda: h.qlpc_batch(x, 16, pcfg(8, more, **kw)),
                 lambda: h.stereo_qlpc_batch(fr, 16, pcfg(8, more, **kw)),
                 lambda: h.encode_stereo_frames(fr, 16, _capi.make_frame_config(pcfg(8, more, **kw))),
                 lambda: h.encode_frames(fr, 16, _capi.make_frame_config(pcfg(8, more, **kw))),
                 lambda: h.encode_variable(fr, 16, _capi.make_frame_config(pcfg(8, more, **kw)), levels=2))
        for call in calls:
            with pytest.raises(_capi.FlacencHipError) as e:
                call()
            assert e.value.code == _capi.ERR_UNSUPPORTED, more
    with pytest.raises(_capi.FlacencHipError) as e:  # the candidate batches have no field for wasted bits
        h.qlpc_batch(x, 16, pcfg(8, WASTED))
    assert e.value.code == _capi.ERR_UNSUPPORTED


def test_fixed_lpc_batch_ignores_the_flag(h):
    x = content(4, 4096, 16)
    got = h.fixed_lpc_batch(x, 16, _capi.make_frame_config(pcfg(8)))
    ref = h.fixed_lpc_batch(x, 16, _capi.make_frame_config(_capi.make_config(lpc_order=8)))
    assert all(np.array_equal(g, r) for g, r in zip(got, ref))


def test_fused_pack_is_ignored(h):
    x = content(4, 4096, 16).reshape(2, 2, 4096)
    got = gpu_stereo(h, frame_cfg(12, _capi.FLAG_FUSED_PACK), x, 16)
    assert got == gpu_stereo(h, frame_cfg(12), x, 16)
    assert got != gpu_stereo(h, frame_cfg(12, _capi.FLAG_FUSED_PACK, search=False), x, 16)


# ---- 7. slices and memory ----
def test_a_call_past_the_scratch_bound_runs_in_slices():
    b, order = 256, 12
    per = 264 + 12 * 15 * 144 + 4  # R[] of one window, C = 12 orders x 15 precisions = 180 records, the choice
    edge = (SCRATCH_CAP // per) & ~3
    rows = edge + 600
    assert rows * per > SCRATCH_CAP and per == 26188
    assert edge != (SCRATCH_CAP // (264 + 12 * 144 + 4)) & ~3  # (not the boundary of the order search alone)
    x = content(rows, b, 16, start=0)
    cfg = pcfg(order, OS)
    with _capi.Handle(0) as big:
        big.set_precision_floor(1)
        params, residual, R, A = big.qlpc_batch(x, 16, cfg, want_fp=True)
        for lo in (0, 13000, edge - 128, rows - 256):  # (the third straddles the boundary)
            p2, r2, R2, A2 = big.qlpc_batch(x[lo:lo + 256], 16, cfg, want_fp=True)
            assert np.array_equal(params[lo:lo + 256], p2) and np.array_equal(residual[lo:lo + 256], r2), lo
            assert np.array_equal(R[lo:lo + 256], R2) and np.array_equal(A[lo:lo + 256], A2), lo
    idx = [edge - 1, edge, edge + 1, rows - 1]
    es.check_rows(params[idx], residual[idx], R[idx], A[idx], x[idx], 16, ocfg(order), "slice edge",
                  pm.record_fn(1, (), True))
    assert searched_below(params[idx], 15)


def test_device_memory_comes_back_after_destroy():
    """Handles that ran the search give all their device memory back."""
    rows, b = 8192, 1152
    x = content(rows, b, 16)
    scratch = rows * (264 + 12 * 11 * 144 + 4)  # one call's search scratch (order search at P = 12, floor 5)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for _ in range(3):
        with _capi.Handle(0) as hh:
            hh.qlpc_batch(x, 16, pcfg(12, OS))
            torch.cuda.synchronize()
    free1 = torch.cuda.mem_get_info()[0]
    assert free0 - free1 < scratch, (free0, free1)
