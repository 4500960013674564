"""FLACENC_HIP_FLAG_PRECISION_SEARCH without a GPU: the model (tests/precision_model.py) against the oracle where the
contract says they agree, the minimum and tie rule of its winner, the saving on the golden fixtures at 256-sample blocks,
the refusal of use_direct_mse, the setter's null-handle answer, and the new constants as every binding states them."""
import os
import re

import numpy as np
import pytest

import extreme_signals as es
import guess_model as gm
import order_model as om
import precision_model as pm
import util
import window_model as wm
from flacenc_rs_amd import _capi
from oracle import oracle as orc

ROOT = os.path.dirname(os.path.abspath(__file__)) + "/.."
PS = _capi.FLAG_PRECISION_SEARCH
NAMES = ("ras103", "ras22", "sus109", "sus6")


def _blocks(n, count=2, names=("sus109", "ras22")):
    for name in names:
        for c in range(2):
            x = util.test_signal(name, c)
            for f in range(count):
                yield x[f * n:(f + 1) * n]


@pytest.mark.parametrize("nightly", [False, True])
@pytest.mark.parametrize("n", [256, 1152, 4096])
@pytest.mark.parametrize("order", [1, 8, 12])
def test_a_floor_at_or_above_the_precision_is_estimated_qlpc(n, order, nightly):
    for q0, floor in ((15, 15), (12, 12), (12, 15), (5, 5)):
        cfg = om.config(order=order, nightly=nightly, quant_precision=q0)
        assert pm.precisions(q0, floor) == [q0]
        for x in _blocks(n, 1):
            recs, residual, R, A = orc.qlpc_batch(x[None, :], 16, cfg)  # estimated_qlpc, as the device states a record
            rec, resid, ac, lc = pm.record(x, 16, cfg, floor)
            assert rec["status"] == int(recs[0]["status"]) == 0
            assert rec == es.params_record(recs[0]), (n, order, q0, floor)
            assert rec["precision"] == q0
            assert np.array_equal(resid, residual[0]) and np.array_equal(ac, R[0]) and np.array_equal(lc, A[0])


@pytest.mark.parametrize("q0,floor", [(15, 1), (15, 5), (5, 1), (1, 1), (1, 5), (12, 11)])
@pytest.mark.parametrize("n,order", [(256, 8), (1152, 12), (4096, 1)])
def test_the_winner_is_the_minimum_and_never_longer_than_the_top_precision(q0, floor, n, order):
    cfg = om.config(order=order, quant_precision=q0)
    qs = pm.precisions(q0, floor)
    assert qs[0] == q0 and qs[-1] == min(q0, floor) if floor < q0 else qs == [q0]
    for x in _blocks(n, 1):
        best, cands = pm.search(x, 16, cfg, floor)
        assert [c["q"] for c in cands] == qs and all(c["j"] == 0 and c["o"] == order for c in cands)
        ok = [c for c in cands if c["status"] == 0]
        assert len(ok) == len(cands)
        for c in cands:  # each is coded at its own precision, and the key's precision term is that precision
            assert int(c["qp"].precision) == c["q"]
            rbits = orc.residual_count_bits(n, c["qp"].order, c["rice_order"], c["rice_params"], c["sum_quotients"],
                                            int(np.sum(c["rice_params"][:1 << c["rice_order"]], dtype=np.int64)))
            assert c["subframe_bits"] == 8 + 16 * c["qp"].order + 4 + 5 + c["q"] * c["qp"].order + rbits
            assert np.array_equal(c["coefs"], cands[0]["coefs"])  # the unquantised coefficients do not depend on i
        low = min(c["subframe_bits"] for c in ok)
        assert best["subframe_bits"] == low
        assert best["q"] == max(c["q"] for c in ok if c["subframe_bits"] == low)  # ties: the higher precision
        top = orc.estimated_qlpc(x, 16, cfg)
        assert cands[0]["subframe_bits"] == int(top["subframe_bits"]) and best["subframe_bits"] <= int(top["subframe_bits"])


def test_the_other_search_flags_keep_their_candidates_and_are_never_longer():
    cfg = om.config(order=8)
    for x in _blocks(1152, 1):
        for extras, orders, K in (((), True, 0), (wm.DEFAULT, False, 0), ((), False, 2), (wm.DEFAULT[:1], True, 0),
                                  (wm.DEFAULT[:2], False, 1)):
            best, cands = pm.search(x, 16, cfg, 10, extras, orders, K)
            plain = gm.search(x, 16, cfg, K, extras)[0] if K else wm.search(x, 16, cfg, extras, orders)[0]
            assert best["subframe_bits"] <= plain["subframe_bits"]
            grid = [(c["j"], c["o"]) for c in cands if c["q"] == 15]
            assert [(c["j"], c["o"], c["q"]) for c in cands] == [(j, o, q) for j, o in grid for q in range(15, 9, -1)]
            key = lambda c: (c["subframe_bits"], c["j"], c["o"], -c["q"])  # noqa: E731
            assert key(best) == min(key(c) for c in cands if c["status"] == 0)


def test_golden_fixtures_at_256_samples_get_strictly_shorter():
    """All 32 blocks of every fixture channel, floor 5, q0 = 15 (run with -s for the figures: over six blocks the
    oracle gives 1.4 - 2.4 % on sus109.ch0 and ras22.ch1)."""
    for order in (8, 12):
        cfg = om.config(order=order)
        got = ref = below = blocks = 0
        saving = {}
        for name in NAMES:
            for ch in range(2):
                x = util.test_signal(name, ch)
                g = r = 0
                for f in range(len(x) // 256):
                    best, cands = pm.search(x[f * 256:(f + 1) * 256], 16, cfg)
                    g += best["subframe_bits"]
                    r += cands[0]["subframe_bits"]
                    below += best["q"] < 15
                    blocks += 1
                assert g <= r
                saving[(name, ch)] = 100.0 * (r - g) / r
                got += g
                ref += r
        print("order", order, "bits", got, "against", ref, "chosen below 15:", below, "of", blocks, saving)
        assert got < ref
        assert 2 * below > blocks


def test_verify_config_refuses_direct_mse_with_the_flag():
    assert _capi.verify_config(_capi.make_config(lpc_order=8, flags=PS)) == _capi.OK
    assert _capi.verify_config(_capi.make_config(lpc_order=8, flags=PS, use_direct_mse=True)) == _capi.ERR_UNSUPPORTED
    assert _capi.verify_config(_capi.make_config(lpc_order=8, flags=PS, use_direct_mse=True,
                                                 mae_optimization_steps=2)) == _capi.ERR_UNSUPPORTED
    for other in (_capi.FLAG_ORDER_SEARCH, _capi.FLAG_WINDOW_SEARCH, _capi.FLAG_ORDER_GUESS, _capi.FLAG_WASTED_BITS,
                  _capi.FLAG_ORDER_SEARCH | _capi.FLAG_WINDOW_SEARCH, _capi.FLAG_ORDER_GUESS | _capi.FLAG_WINDOW_SEARCH):
        for order in (1, 8, 32):
            assert _capi.verify_config(_capi.make_config(lpc_order=order, flags=PS | other)) == _capi.OK, (other, order)
        assert _capi.verify_config(_capi.make_config(lpc_order=8, flags=PS | other, use_direct_mse=True)) == \
            _capi.ERR_UNSUPPORTED
    for q in (1, 5, 15):
        assert _capi.verify_config(_capi.make_config(lpc_order=8, quant_precision=q, flags=PS)) == _capi.OK


def test_setter_validation_without_a_handle_refuses_first():
    L = _capi.load()
    for floor in (5, 0, 16):
        assert L.flacenc_hip_set_precision_floor(None, floor) == _capi.ERR_BAD_ARGUMENT


def _read(path):
    with open(os.path.join(ROOT, path)) as f:
        return f.read()


def test_constants_agree_across_bindings():
    h, rs, hpp = _read("include/flacenc_hip.h"), _read("rust/flacenc_hip.rs"), _read("flacenc_rs_amd/host/flacenc.hpp")
    assert _capi.FLAG_PRECISION_SEARCH == 8192
    assert re.search(r"#define FLACENC_HIP_FLAG_PRECISION_SEARCH 8192u\b", h)
    assert re.search(r"pub const FLAG_PRECISION_SEARCH: u32 = 8192;", rs)
    assert "FLACENC_HIP_FLAG_PRECISION_SEARCH" in hpp
    # the floor of a fresh handle
    assert _capi.DEFAULT_PRECISION_FLOOR == pm.DEFAULT_FLOOR == 5
    assert re.search(r"a fresh handle holds 5\b", h)
    assert re.search(r"pub const DEFAULT_PRECISION_FLOOR: u32 = 5;", rs)
    assert re.search(r"kDefaultPrecisionFloor = 5;", hpp)
    assert re.search(r"uint32_t precision_floor = 5;", _read("flacenc_rs_amd/csrc/api_internal.h"))
    sym = "flacenc_hip_set_precision_floor"
    assert sym in _capi.EXPORTED_SYMBOLS and sym in h and ("pub fn " + sym) in rs and sym in hpp
    assert hasattr(_capi.load(), sym) and hasattr(_capi.Handle, "set_precision_floor")
    # additive: the ABI revision stays
    assert _capi.ABI_VERSION == 6 and _capi.load().flacenc_hip_abi_version() == 6
    assert re.search(r"#define FLACENC_HIP_ABI_VERSION 6\b", h) and re.search(r"pub const ABI_VERSION: c_int = 6;", rs)
    flags = [v for k, v in vars(_capi).items() if k.startswith("FLAG_")]
    assert len(flags) == len(set(flags))
