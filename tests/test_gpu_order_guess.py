"""FLACENC_HIP_FLAG_ORDER_GUESS on the GPU: candidate records, residual rows, R[] and coefficients equal the model's
(tests/guess_model.py) byte for byte on the corpus (tests/guess_cases.py, each case first asserting from the model what it
reaches) and on music rows across block sizes, order buckets, precisions, widths and K, with and without the window
search; big calls run in slices; frames equal the model's bytes with and without wasted bits, the block-size search keeps
the fixed path's bodies; the rule's consequences hold on the device; the handle's K behaves as state should, the refused
configs are refused, and a flagged call replays from a graph."""
import numpy as np
import pytest
import torch

import extreme_signals as es
import guess_cases as gc
import guess_model as gm
import order_model as om
import window_cases as wc
import window_model as wm
from flacenc_rs_amd import _capi
from oracle import oracle as orc
from test_gpu_order_search import content, decode_check, gpu_channels, gpu_stereo
from test_gpu_variable_block import check as variable_check
from test_gpu_window_search_extremes import distinct_rows

pytestmark = pytest.mark.gpu
G = _capi.FLAG_ORDER_GUESS
WS = _capi.FLAG_WINDOW_SEARCH
OS = _capi.FLAG_ORDER_SEARCH
REF = _capi.FLAG_REFERENCE_SUM_ORDER
WASTED = _capi.FLAG_WASTED_BITS
SCRATCH_CAP = 768 << 20  # kSearchScratchCap


@pytest.fixture(scope="module")
def h():
    with _capi.Handle(0) as handle:
        yield handle


class state:
    """K and the extra-window list on a handle for one block; a fresh handle's values afterwards."""

    def __init__(self, handle, K=1, extras=None):
        self.h, self.K, self.extras = handle, K, extras

    def __enter__(self):
        self.h.set_order_guesses(self.K)
        if self.extras is not None:
            self.h.set_lpc_windows(self.extras)
        return self.h

    def __exit__(self, *exc):
        self.h.set_order_guesses(1)
        self.h.set_lpc_windows(wm.DEFAULT)


def gcfg(order, flags=0, windows=False, **kw):
    return _capi.make_config(lpc_order=order, flags=G | (WS if windows else 0) | flags, **kw)


def ocfg(order, q=15):
    return om.config(order=order, quant_precision=q)


def guess_record(K, extras=()):
    return lambda x, bps, cfg: gm.record(x, bps, cfg, K, extras)


def check_stereo(params, residual, x, bits, cfg, K, extras=(), frames=None):
    for f in (range(len(x)) if frames is None else frames):
        m, s = orc.stereo_to_midside(x[f, 0], x[f, 1])
        for k, sig in enumerate((x[f, 0], x[f, 1], m, s)):
            rec, resid, _, _ = gm.record(sig, bits + (1 if k == 3 else 0), cfg, K, extras)
            assert int(params[f, k]["status"]) == rec["status"] == 0, (f, k)
            assert es.params_record(params[f, k]) == rec, (f, k)
            assert np.array_equal(residual[f, k], resid), (f, k)


# ---- 1. records against the model ----
CORPUS = gc.all_cases()


@pytest.mark.parametrize("c", CORPUS, ids=gc.ids(CORPUS))
def test_corpus_records_equal_the_model(h, c):
    gc.claims(c)
    with state(h, c.K, c.extras if c.extras else None):
        cfg = gcfg(c.order, windows=bool(c.extras), quant_precision=c.q)
        x = c.x[None, :]
        got = h.qlpc_batch(x, c.bps, cfg, want_fp=True)
    es.check_rows(*got, x, c.bps, gc.config(c), c.name, guess_record(c.K, c.extras))


MUSIC_CASES = [
    # (block, order, precision, bits, K): every block size, MAXP bucket, precision, width and K of the issue at least once
    (64, 8, 15, 16, 1), (100, 12, 5, 16, 2), (256, 1, 15, 8, 1), (576, 2, 15, 16, 3), (4096, 12, 15, 16, 1),
    (4096, 13, 5, 24, 13), (4608, 24, 15, 16, 2), (8192, 32, 15, 24, 32), (20000, 8, 15, 16, 3), (32767, 32, 5, 24, 1),
    (4096, 32, 15, 16, 2), (4096, 8, 15, 8, 8), (20000, 13, 15, 24, 2),
]


@pytest.mark.parametrize("b,order,q,bits,K", MUSIC_CASES)
def test_music_records_equal_the_model(h, b, order, q, bits, K):
    rows = 4 if b <= 4608 else 2
    x = content(rows, b, bits, start=3 * b)
    with state(h, K):
        cfg = gcfg(order, quant_precision=q)
        got = h.qlpc_batch(x, bits, cfg, want_fp=True)
        frames = x[:2].reshape(1, 2, b)
        sp, sr = h.stereo_qlpc_batch(frames, bits, cfg)
    es.check_rows(*got, x, bits, ocfg(order, q), (b, order, q, bits, K), guess_record(K))
    check_stereo(sp, sr, frames, bits, ocfg(order, q), K)  # (the side role's w + 1 enters the cost)


def test_per_row_bits_per_sample_enter_the_cost(h):
    b, order = 4096, 12
    x = content(4, b, 16, start=5 * b)
    bps = np.array([16, 25, 17, 20], np.uint8)
    with state(h, 2):
        got = h.qlpc_batch(x, bps, gcfg(order), want_fp=True)
    es.check_rows(*got, x, bps, ocfg(order), "per-row bps", guess_record(2))


# ---- 2. with the window search ----
DEAD64 = (wc.DEAD[0], (wm.TUKEY, 0.2, 0, 0), wc.DEAD[2])  # entries 1 and 3 have no non-zero weight on 64 samples


@pytest.mark.parametrize("K", [1, 2])
@pytest.mark.parametrize("b,order,bits,lst", [(4096, 12, 16, "default"), (4096, 32, 16, "default"),
                                              (1152, 24, 24, "random"), (64, 8, 16, "dead")])
def test_window_search_records_equal_the_model(h, b, order, bits, lst, K):
    extras = {"default": wm.DEFAULT, "random": wm.random_extras(np.random.default_rng(b + order), b) or wc.E3,
              "dead": DEAD64}[lst]
    if lst == "dead":
        assert not np.any(wm.weights(DEAD64[0], b)) and not np.any(wm.weights(DEAD64[2], b))
    x = content(3, b, bits, start=7 * b)
    with state(h, K, extras):
        cfg = gcfg(order, windows=True)
        got = h.qlpc_batch(x, bits, cfg, want_fp=True)
        frames = x[:2].reshape(1, 2, b)
        sp, sr = h.stereo_qlpc_batch(frames, bits, cfg)
    es.check_rows(*got, x, bits, ocfg(order), (b, order, lst, K), guess_record(K, extras))
    check_stereo(sp, sr, frames, bits, ocfg(order), K, extras)


def test_window_search_without_extra_windows_is_the_guess_call(h):
    b, order = 4096, 12
    x = content(4, b, 16, start=13 * b)
    with _capi.Handle(0) as h0:
        h0.set_lpc_windows([])
        got = h0.qlpc_batch(x, 16, gcfg(order, windows=True), want_fp=True)
        ref = h0.qlpc_batch(x, 16, gcfg(order), want_fp=True)
    assert all(np.array_equal(g, r) for g, r in zip(got, ref))
    es.check_rows(*got, x, 16, ocfg(order), "no extra window", guess_record(1))


# ---- 3. slices ----
def test_stereo_slices_read_their_own_frames():
    # one batch past the scratch bound at the new bytes per subframe: R[] of 8 windows, 256 candidates of 144 + 8 bytes
    b, order, bits, K = 256, 32, 16, 2
    extras = wc.E7
    per = 8 * 264 + 8 * order * (144 + 8) + 4
    edge = (SCRATCH_CAP // per) & ~3
    nf = edge // 4 + 150
    assert 4 * nf * per > SCRATCH_CAP and edge % 4 == 0
    # (the old bytes per subframe would put the boundary elsewhere: the checks below sit on the new one)
    assert edge != (SCRATCH_CAP // (8 * 264 + 8 * order * 144 + 4)) & ~3
    x = distinct_rows(2 * nf, b, bits, 1).reshape(nf, 2, b)
    cfg = gcfg(order, windows=True)
    with _capi.Handle(0) as big:
        big.set_lpc_windows(extras)
        big.set_order_guesses(K)
        params, residual = big.stereo_qlpc_batch(x, bits, cfg)
        for lo in (0, edge // 4 - 32, nf - 64):  # (the middle one straddles the boundary)
            p2, r2 = big.stereo_qlpc_batch(x[lo:lo + 64], bits, cfg)
            assert np.array_equal(params[lo:lo + 64], p2) and np.array_equal(residual[lo:lo + 64], r2), lo
    for sf in (edge - 1, edge, edge + 1, edge + 3, 4 * nf - 1):
        f, k = divmod(sf, 4)
        m, s = orc.stereo_to_midside(x[f, 0], x[f, 1])
        sig = (x[f, 0], x[f, 1], m, s)[k]
        rec, resid, _, _ = gm.record(sig, bits + (1 if k == 3 else 0), ocfg(order), K, extras)
        assert int(params[f, k]["status"]) == 0 and es.params_record(params[f, k]) == rec, (sf, f, k)
        assert np.array_equal(residual[f, k], resid), (sf, f, k)


# ---- 4. frame-level calls ----
def frame_cfg(order, flags=0, windows=False, stereo=True, guess=True):
    qlpc = gcfg(order, flags, windows) if guess else _capi.make_config(lpc_order=order, flags=flags)
    return _capi.make_frame_config(qlpc, use_fixed=True, use_leftside=stereo, use_rightside=stereo, use_midside=stereo)


def ofc(order, stereo=True):
    return orc.make_frame_config(ocfg(order), use_leftside=stereo, use_rightside=stereo, use_midside=stereo)


@pytest.mark.parametrize("b,order,bits,K,windows", [(4096, 12, 16, 1, False), (4096, 32, 24, 2, False),
                                                    (1152, 12, 16, 1, True), (37, 8, 16, 1, False)])
def test_stereo_frame_bytes_equal_the_model(h, b, order, bits, K, windows):
    x = content(6, b, bits, start=9 * b).reshape(3, 2, b)
    with state(h, K):
        cfg = frame_cfg(order, windows=windows)
        got = gpu_stereo(h, cfg, x, bits)
        res, resid = h.encode_stereo_frames(x, bits, cfg)
        packed = h.pack_stereo_frames(x, res, resid, bits, 44100)
    assert packed == got  # (encode_stereo_frames + pack is the fused entry point's bytes)
    model = gm.Model(K, wm.DEFAULT if windows else ())
    for f in range(len(x)):
        assert got[f] == model.stereo_frame_bytes(x[f, 0], x[f, 1], bits, ofc(order), number=f), (b, order, f)
    decode_check(h, got, x, bits)


@pytest.mark.parametrize("C,b,order,K", [(1, 4096, 12, 1), (3, 1152, 24, 2), (3, 37, 8, 1)])
def test_independent_frame_bytes_equal_the_model(h, C, b, order, K):
    x = content(2 * C, b, 16, start=11 * b).reshape(2, C, b)
    with state(h, K):
        cfg = frame_cfg(order, stereo=False)
        got = gpu_channels(h, cfg, x, 16)
        res, resid = h.encode_frames(x, 16, cfg)
        assert h.pack_frames(x, res, resid, 16, 44100) == got
    model = gm.Model(K)
    for f in range(len(x)):
        assert got[f] == model.channel_frame_bytes(list(x[f]), 16, ofc(order, stereo=False), number=f), (C, b, f)
    decode_check(h, got, x, 16)


def shifted_frames(b):
    """16-bit music in a 24-bit container: every row shifted by 8 bits, one by 4 more, one frame left at full width."""
    x = content(8, b, 16, start=b).reshape(4, 2, b).astype(np.int64) << 8
    x[2, 0] >>= 4
    x[3] = content(2, b, 24, start=2 * b)
    return x.astype(np.int32)


@pytest.mark.parametrize("K,windows", [(1, False), (2, True)])
def test_stereo_frames_with_wasted_bits_equal_the_model(h, K, windows):
    b, order = 4096, 12
    x = shifted_frames(b)
    with state(h, K):
        got = gpu_stereo(h, frame_cfg(order, WASTED, windows), x, 24)
    model = gm.Model(K, wm.DEFAULT if windows else ())
    for f in range(len(x)):  # (rows shifted by 4 and 8 bits: w - k in the cost)
        assert got[f] == model.wasted_stereo_frame_bytes(x[f, 0], x[f, 1], 24, ofc(order), number=f), f
    decode_check(h, got, x, 24)


def test_independent_frames_with_wasted_bits_equal_the_model(h):
    b, order, K = 1152, 12, 2
    x = shifted_frames(b)[:, :1].repeat(3, axis=1)
    x[:, 1] = shifted_frames(b)[:, 1]
    x[:, 2] >>= 2
    with state(h, K):
        got = gpu_channels(h, frame_cfg(order, WASTED, stereo=False), x, 24)
    model = gm.Model(K)
    for f in range(len(x)):
        assert got[f] == model.wasted_channel_frame_bytes(list(x[f]), 24, ofc(order, stereo=False), number=f), f
    decode_check(h, got, x, 24)


def test_encode_variable_keeps_the_fixed_paths_bodies(h):
    S, levels = 4096, 2
    x = content(8, S, 16, start=9 * S).reshape(4, 2, S)
    with state(h, 2):
        variable_check(h, frame_cfg(12), x, 4 * S - 333, S, levels, 16)


# ---- 5. consequences on the device ----
@pytest.mark.parametrize("b,order,K,windows", [(4096, 12, 1, False), (4096, 32, 2, False), (1152, 24, 1, True)])
def test_frames_lie_between_the_exhaustive_search_and_the_reference_order(h, b, order, K, windows):
    x = content(16, b, 16).reshape(8, 2, b)
    ws = WS if windows else 0
    with state(h, K):
        got = gpu_stereo(h, frame_cfg(order, windows=windows), x, 16)
    plain = gpu_stereo(h, frame_cfg(order, REF, guess=False), x, 16)
    exhaustive = gpu_stereo(h, frame_cfg(order, OS | ws, guess=False), x, 16)
    assert all(len(e) <= len(g) <= len(p) for e, g, p in zip(exhaustive, got, plain))


@pytest.mark.parametrize("b,order,bits", [(4096, 12, 16), (4096, 8, 24), (1152, 13, 16)])
def test_k_equal_to_the_order_is_the_order_search_on_music(h, b, order, bits):
    x = content(4, b, bits, start=15 * b)
    for row in x:  # (every order has status 0 and is eligible: the premise, from the model)
        assert gm.search(row, bits, ocfg(order), order)[2][0]["eligible"] == order
    with state(h, order):
        got = h.qlpc_batch(x, bits, gcfg(order), want_fp=True)
    want = h.qlpc_batch(x, bits, _capi.make_config(lpc_order=order, flags=OS), want_fp=True)
    assert all(np.array_equal(g, w) for g, w in zip(got, want))


def test_order_1_without_extra_windows_changes_no_byte(h):
    x = content(8, 4096, 16).reshape(4, 2, 4096)
    assert gpu_stereo(h, frame_cfg(1), x, 16) == gpu_stereo(h, frame_cfg(1, REF, guess=False), x, 16)
    rows = x.reshape(8, 4096)
    got = h.qlpc_batch(rows, 16, gcfg(1), want_fp=True)
    want = h.qlpc_batch(rows, 16, _capi.make_config(lpc_order=1, flags=REF), want_fp=True)
    assert all(np.array_equal(g, w) for g, w in zip(got, want))


def test_ar2_and_golden_order_32_batches_are_strictly_smaller(h):
    """Fails where the flag's bit is ignored: the flagged call is then the unflagged one."""
    ar2 = np.stack([gc.ar2(4096, seed=s) for s in range(1, 5)]).astype(np.int32)
    got, _, _, _ = h.qlpc_batch(ar2, 16, gcfg(12))
    ref, _, _, _ = h.qlpc_batch(ar2, 16, _capi.make_config(lpc_order=12, flags=REF))
    assert (got["status"] == 0).all() and got["order"].tolist() == [2] * 4
    assert (got["subframe_bits"] < ref["subframe_bits"]).all()
    music = content(16, 4096, 16)  # the first two blocks of the eight fixture channels
    got, _, _, _ = h.qlpc_batch(music, 16, gcfg(32))
    ref, _, _, _ = h.qlpc_batch(music, 16, _capi.make_config(lpc_order=32, flags=REF))
    assert (got["subframe_bits"] <= ref["subframe_bits"]).all()
    assert int(got["subframe_bits"].sum()) < int(ref["subframe_bits"].sum())
    frames = music.reshape(8, 2, 4096)
    assert sum(map(len, gpu_stereo(h, frame_cfg(32), frames, 16))) < \
        sum(map(len, gpu_stereo(h, frame_cfg(32, REF, guess=False), frames, 16)))


# ---- 6. handle state and flag rules ----
def test_the_setter_affects_only_later_flagged_calls():
    b, order = 4096, 32
    x = content(4, b, 16, start=17 * b)
    cfg, oc = gcfg(order), ocfg(order)
    plain_cfg = _capi.make_config(lpc_order=order)
    with _capi.Handle(0) as fresh, _capi.Handle(0) as other:
        u0 = fresh.qlpc_batch(x, 16, plain_cfg, want_fp=True)
        k1 = fresh.qlpc_batch(x, 16, cfg, want_fp=True)
        es.check_rows(*k1, x, 16, oc, "fresh: K = 1", guess_record(1))
        fresh.set_order_guesses(3)
        k3 = fresh.qlpc_batch(x, 16, cfg, want_fp=True)
        es.check_rows(*k3, x, 16, oc, "K = 3", guess_record(3))
        assert not np.array_equal(k1[0], k3[0])  # (K changes these rows' records: the setter is seen to act)
        es.check_rows(*other.qlpc_batch(x, 16, cfg, want_fp=True), x, 16, oc, "another handle", guess_record(1))
        for bad in (0, 33, 1 << 31):
            with pytest.raises(_capi.FlacencHipError) as e:
                fresh.set_order_guesses(bad)
            assert e.value.code == _capi.ERR_BAD_ARGUMENT
        again = fresh.qlpc_batch(x, 16, cfg, want_fp=True)  # a refused setter keeps the value
        assert all(np.array_equal(p, q) for p, q in zip(again, k3))
        # without the flag no byte changes with K
        u3 = fresh.qlpc_batch(x, 16, plain_cfg, want_fp=True)
        assert all(np.array_equal(p, q) for p, q in zip(u0, u3))
        fr = x.reshape(2, 2, b)
        s3 = gpu_stereo(fresh, frame_cfg(order, OS, guess=False), fr, 16)
        assert s3 == gpu_stereo(other, frame_cfg(order, OS, guess=False), fr, 16)
        fresh.set_order_guesses(1)
        back = fresh.qlpc_batch(x, 16, cfg, want_fp=True)
        assert all(np.array_equal(p, q) for p, q in zip(back, k1))


def test_refused_configs_answer_their_codes(h):
    x = content(2, 4096, 16)
    fr = x.reshape(1, 2, 4096)
    for kw, code in ((dict(flags=OS), _capi.ERR_BAD_CONFIG), (dict(flags=OS | WS), _capi.ERR_BAD_CONFIG),
                     (dict(use_direct_mse=True), _capi.ERR_UNSUPPORTED)):
        flags = kw.pop("flags", 0)
        calls = (lambda: h.qlpc_batch(x, 16, gcfg(8, flags, **kw)),
                 lambda: h.stereo_qlpc_batch(fr, 16, gcfg(8, flags, **kw)),
                 lambda: h.encode_stereo_frames(fr, 16, _capi.make_frame_config(gcfg(8, flags, **kw))),
                 lambda: h.encode_frames(fr, 16, _capi.make_frame_config(gcfg(8, flags, **kw))),
                 lambda: h.encode_variable(fr, 16, _capi.make_frame_config(gcfg(8, flags, **kw)), levels=2))
        for call in calls:
            with pytest.raises(_capi.FlacencHipError) as e:
                call()
            assert e.value.code == code, (kw, flags)
    with pytest.raises(_capi.FlacencHipError) as e:  # the candidate batches have no field for wasted bits
        h.qlpc_batch(x, 16, gcfg(8, WASTED))
    assert e.value.code == _capi.ERR_UNSUPPORTED


def test_fixed_lpc_batch_ignores_the_flag(h):
    x = content(4, 4096, 16)
    got = h.fixed_lpc_batch(x, 16, _capi.make_frame_config(gcfg(8)))
    ref = h.fixed_lpc_batch(x, 16, _capi.make_frame_config(_capi.make_config(lpc_order=8)))
    assert all(np.array_equal(g, r) for g, r in zip(got, ref))


def test_fused_pack_is_ignored(h):
    x = content(4, 4096, 16).reshape(2, 2, 4096)
    assert gpu_stereo(h, frame_cfg(12, _capi.FLAG_FUSED_PACK), x, 16) == gpu_stereo(h, frame_cfg(12), x, 16)


def test_a_captured_call_replays_the_eager_bytes():
    b, order, nf, K = 4096, 12, 4, 2
    x = content(2 * nf, b, 16, start=19 * b).reshape(nf, 2, b)
    cfg = gcfg(order, windows=True)
    with _capi.Handle(0) as hh:
        hh.set_order_guesses(K)
        want_p, want_r = hh.stereo_qlpc_batch(x, 16, cfg)
        dx = torch.from_numpy(x).cuda()
        dp = torch.zeros(nf * 4 * _capi.PARAMS_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        dr = torch.zeros((nf * 4, b), dtype=torch.int32, device="cuda")

        def launch():
            hh.stereo_qlpc_batch_device(cfg, dx.data_ptr(), nf, b, b, 16, dp.data_ptr(), dr.data_ptr(), b,
                                        torch.cuda.current_stream().cuda_stream)

        launch()  # warm: scratch and window tables exist at this shape
        torch.cuda.synchronize()
        s, g = torch.cuda.Stream(), torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s, capture_error_mode="global"):
            launch()
        with torch.cuda.stream(s):
            dp.zero_()
            dr.zero_()
            g.replay()
        s.synchronize()
        got_p = dp.cpu().numpy().view(_capi.PARAMS_DTYPE).reshape(nf, 4)
        got_r = dr.cpu().numpy().reshape(nf, 4, b)
        del g
    assert np.array_equal(got_p, want_p) and np.array_equal(got_r, want_r)
    check_stereo(got_p, got_r, x, 16, ocfg(order), K, wm.DEFAULT, frames=[0])
