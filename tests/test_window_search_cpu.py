"""FLACENC_HIP_FLAG_WINDOW_SEARCH without a GPU: flacenc_hip_lpc_window_weights against the model's weights
(tests/window_model.py) bit for bit, its validation rules, the refusal of use_direct_mse, the model against the oracle
where the contract says they agree, and the new constants as every binding states them."""
import math
import os
import re

import numpy as np
import pytest

import order_model as om
import util
import window_model as wm
from flacenc_rs_amd import _capi
from oracle import oracle as orc

ROOT = os.path.dirname(os.path.abspath(__file__)) + "/.."
SIZES = (64, 100, 1152, 4096, 4608, 20000, 32767)


def same_bits(a, b):
    return a.dtype == b.dtype == np.float32 and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def random_entries(seed, count=40):
    rng = np.random.default_rng(seed)
    for _ in range(count):
        t = int(rng.integers(0, 4))
        alpha = float(np.float32(rng.choice([0.0, 0.2, 0.4, 1.0, rng.random()])))
        s = int(rng.integers(0, wm.UNIT))
        e = int(rng.integers(s + 1, wm.UNIT + 1))
        yield t, alpha, s, e


@pytest.mark.parametrize("n", SIZES)
def test_default_entries_equal_the_model(n):
    for e in _capi.DEFAULT_LPC_WINDOWS:
        assert same_bits(_capi.lpc_window_weights(*e, n), wm.weights(e, n)), (e, n)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("alpha", [0.0, 0.2, 0.4, 1.0])
def test_random_entries_equal_the_model(n, alpha):
    for t, _, s, e in random_entries(n + int(alpha * 10), 12):
        ent = (t, alpha, s, e)
        assert same_bits(_capi.lpc_window_weights(*ent, n), wm.weights(ent, n)), (ent, n)
    for ent in random_entries(7 * n, 8):
        assert same_bits(_capi.lpc_window_weights(*ent, n), wm.weights(ent, n)), (ent, n)


@pytest.mark.parametrize("m", [0, 1, 2, 3])
@pytest.mark.parametrize("alpha", [0.0, 0.2, 0.4, 1.0])
def test_pieces_of_zero_to_three_samples(m, alpha):
    n = 4096  # (s = start >> 4: every sample boundary is an exact start / end)
    for s in (0, 1000, n - 3):
        ent = (wm.PARTIAL_TUKEY, alpha, s << 4, (s + m) << 4)
        if m == 0:  # (start >= end is refused; an empty piece comes from rounding instead)
            ent = (wm.PARTIAL_TUKEY, alpha, s << 4, (s << 4) + 15)
        assert wm.piece(*ent[2:], n) == (s, s + m)
        w = _capi.lpc_window_weights(*ent, n)
        assert same_bits(w, wm.weights(ent, n))
        assert np.count_nonzero(w[:s]) == 0 and np.count_nonzero(w[s + m:]) == 0
        if m < 2:
            assert np.count_nonzero(w) == 0  # (the reference's formula would give NaN at 1 sample)
    for head in (0, 1, 2, 3):
        ent = (wm.PUNCHOUT_TUKEY, alpha, head << 4, (n - m) << 4)
        s, e = wm.piece(*ent[2:], n)
        assert (s, n - e) == (head, m)
        w = _capi.lpc_window_weights(*ent, n)
        assert same_bits(w, wm.weights(ent, n))
        assert np.count_nonzero(w[s:e]) == 0
        if head < 2:
            assert np.count_nonzero(w[:s]) == 0
        if m < 2:
            assert np.count_nonzero(w[e:]) == 0


@pytest.mark.parametrize("n", SIZES)
def test_tukey_and_rectangle_entries_equal_the_config_window(n):
    for alpha in (0.0, 0.2, 0.4, 0.5, 1.0):
        got = _capi.lpc_window_weights(_capi.WINDOW_TUKEY, alpha, 123, 45, n)  # (start / end ignored)
        assert same_bits(got, _capi.window_weights(_capi.make_config(window=("tukey", alpha)), n))
    got = _capi.lpc_window_weights(_capi.WINDOW_RECTANGLE, 0.7, 0, 0, n)
    assert same_bits(got, _capi.window_weights(_capi.make_config(window="rectangle"), n))


def _weights_rc(t, alpha, s, e, n=256):
    out = np.zeros(max(n, 1), np.float32)
    return _capi.load().flacenc_hip_lpc_window_weights(t, alpha, s, e, n, out.ctypes.data)


BAD_ENTRIES = [
    (4, 0.2, 0, 100), (99, 0.2, 0, 100),                                   # unknown type
    (1, -0.01, 0, 0), (1, 1.01, 0, 0), (2, math.nan, 0, 100), (0, math.inf, 0, 0), (3, -math.inf, 0, 10),  # alpha
    (2, 0.2, 100, 100), (2, 0.2, 200, 100), (3, 0.2, 0, 65537), (2, 0.2, 0, 1 << 31), (3, 0.2, 65536, 65536),  # pieces
]


@pytest.mark.parametrize("ent", BAD_ENTRIES)
def test_weights_validation(ent):
    assert _weights_rc(*ent) == _capi.ERR_BAD_CONFIG


def test_weights_accept_the_edges():
    for ent in [(2, 0.0, 0, 65536), (3, 1.0, 0, 1), (2, 0.2, 65535, 65536), (0, 0.5, 9, 3), (1, 0.0, 70000, 0)]:
        assert _weights_rc(*ent) == _capi.OK, ent
    assert _weights_rc(2, 0.2, 0, 65536, n=0) == _capi.OK
    assert _capi.load().flacenc_hip_lpc_window_weights(2, 0.2, 0, 100, 64, None) == _capi.ERR_BAD_ARGUMENT
    assert _weights_rc(2, 0.2, 0, 100, n=32768) == _capi.ERR_BAD_ARGUMENT


def test_setter_validation_without_a_handle_refuses_first():
    L = _capi.load()
    t = np.array([2], np.uint32)
    a = np.array([0.2], np.float32)
    s = np.array([0], np.uint32)
    e = np.array([100], np.uint32)
    assert L.flacenc_hip_set_lpc_windows(None, t.ctypes.data, a.ctypes.data, s.ctypes.data, e.ctypes.data, 1) == \
        _capi.ERR_BAD_ARGUMENT


def test_verify_config_refuses_direct_mse_with_the_flag():
    F = _capi.FLAG_WINDOW_SEARCH
    for flags in (F, F | _capi.FLAG_ORDER_SEARCH):
        assert _capi.verify_config(_capi.make_config(lpc_order=8, flags=flags)) == _capi.OK
        assert _capi.verify_config(_capi.make_config(lpc_order=32, flags=flags)) == _capi.OK
        assert _capi.verify_config(_capi.make_config(lpc_order=8, flags=flags, use_direct_mse=True)) == \
            _capi.ERR_UNSUPPORTED
        assert _capi.verify_config(_capi.make_config(lpc_order=8, flags=flags, use_direct_mse=True,
                                                     mae_optimization_steps=2)) == _capi.ERR_UNSUPPORTED
    assert _capi.verify_config(_capi.make_config(lpc_order=16, flags=F | _capi.FLAG_NIGHTLY_SUM_ORDER)) == \
        _capi.ERR_UNSUPPORTED


def _blocks(n, count=2):
    for name in ("sus109", "ras22"):
        for c in range(2):
            x = util.test_signal(name, c)
            for f in range(count):
                yield x[f * n:(f + 1) * n]


@pytest.mark.parametrize("n,order,nightly", [(4096, 8, False), (1152, 12, False), (100, 3, False), (4096, 32, False),
                                             (4096, 12, True)])
def test_the_config_window_alone_is_estimated_qlpc(n, order, nightly):
    cfg = om.config(order=order, nightly=nightly)
    for x in _blocks(n):
        ref = orc.estimated_qlpc(x, 16, cfg)
        rec, resid, ac, lc = wm.record(x, 16, cfg, extras=())
        assert np.array_equal(ac[:order + 1], ref["autocorr"])
        assert rec["subframe_bits"] == ref["subframe_bits"] and np.array_equal(resid, ref["residual"])
        # ... and with the order search, order_model's record
        got, gres, gac, glc = wm.record(x, 16, cfg, extras=(), orders=True)
        want, wres, wac, wlc = om.record(x, 16, cfg)
        assert got == want and np.array_equal(gres, wres) and np.array_equal(gac, wac) and np.array_equal(glc, wlc)


@pytest.mark.parametrize("order", [8, 12, 32])
def test_the_search_is_never_longer_and_picks_the_minimum(order):
    cfg = om.config(order=order)
    for x in _blocks(4096, 1):
        best, cands = wm.search(x, 16, cfg)
        ok = [c for c in cands if c["status"] == 0]
        assert best["subframe_bits"] == min(c["subframe_bits"] for c in ok)
        assert best["j"] == min(c["j"] for c in ok if c["subframe_bits"] == best["subframe_bits"])
        assert best["subframe_bits"] <= orc.estimated_qlpc(x, 16, cfg)["subframe_bits"]
        both, _ = wm.search(x, 16, cfg, orders=True)
        assert both["subframe_bits"] <= min(best["subframe_bits"], om.search(x, 16, cfg)[0]["subframe_bits"])


def test_golden_content_at_order_32_gets_strictly_shorter():
    cfg = om.config(order=32)
    got = ref = 0
    for x in _blocks(4096, 2):
        best, cands = wm.search(x, 16, cfg)
        got += best["subframe_bits"]
        ref += cands[0]["subframe_bits"]
    assert got < ref


def _read(path):
    with open(os.path.join(ROOT, path)) as f:
        return f.read()


def test_constants_agree_across_bindings():
    h, rs, hpp = _read("include/flacenc_hip.h"), _read("rust/flacenc_hip.rs"), _read("flacenc_rs_amd/host/flacenc.hpp")
    assert _capi.FLAG_WINDOW_SEARCH == 2048
    assert re.search(r"#define FLACENC_HIP_FLAG_WINDOW_SEARCH 2048u\b", h)
    assert re.search(r"pub const FLAG_WINDOW_SEARCH: u32 = 2048;", rs)
    for name, value in (("WINDOW_PARTIAL_TUKEY", 2), ("WINDOW_PUNCHOUT_TUKEY", 3), ("MAX_LPC_WINDOWS", 8),
                        ("WINDOW_UNIT", 65536)):
        assert getattr(_capi, name) == value
        assert re.search(r"#define FLACENC_HIP_%s %d\b" % (name, value), h), name
        assert re.search(r"pub const %s: u32 = %d;" % (name, value), rs), name
    for sym in ("flacenc_hip_set_lpc_windows", "flacenc_hip_lpc_window_weights"):
        assert sym in _capi.EXPORTED_SYMBOLS and sym in h and ("pub fn " + sym) in rs
        assert hasattr(_capi.load(), sym)
    assert "FLACENC_HIP_FLAG_WINDOW_SEARCH" in hpp and "flacenc_hip_set_lpc_windows" in hpp
    flags = [v for k, v in vars(_capi).items() if k.startswith("FLAG_")]
    assert len(flags) == len(set(flags))


def test_default_windows_agree_across_header_python_and_model():
    assert tuple(_capi.DEFAULT_LPC_WINDOWS) == wm.DEFAULT
    h = _read("include/flacenc_hip.h")
    names = {2: "PARTIAL_TUKEY", 3: "PUNCHOUT_TUKEY"}
    for t, alpha, s, e in wm.DEFAULT:
        assert "%s(%g) [%d, %d)" % (names[t], alpha, s, e) in h, (t, s, e)
    assert len(wm.DEFAULT) <= _capi.MAX_LPC_WINDOWS - 1
