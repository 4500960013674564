"""The order-search model (tests/order_model.py) on worst-case material without a GPU: its chosen key is the minimum,
its candidate P is estimated_qlpc's record, status included, for every max_rice_parameter the GPU tests use, and the
model composed with wasted bits reduces to wasted_model at order 1 and to order_model without wasted bits."""
import numpy as np
import pytest

import extreme_signals as es
import order_model as om
import wasted_model as wm
from oracle import oracle as orc

MAX_PS = [0, 1, 2, 4, 6, 14, 15, 30]


def corpus(seed, n, bits):
    """Worst-case rows: extreme_frames plus full-scale alternation and noise."""
    rows = list(es.extreme_frames(np.random.default_rng(seed), n, bits).reshape(-1, n)[:6])
    return rows + [es.alternation(n, bits), es.noise(n, bits, seed)]


@pytest.mark.parametrize("max_p", MAX_PS)
@pytest.mark.parametrize("n,bits,order", [(4096, 24, 8), (4097, 24, 12), (1000, 16, 32), (97, 8, 12)])
def test_the_key_is_minimal_and_candidate_p_is_estimated_qlpc(max_p, n, bits, order):
    cfg = om.config(order=order, max_rice_parameter=max_p, window="rectangle", quant_precision=12)
    for i, x in enumerate(corpus(n + max_p, n, bits)):
        x = np.ascontiguousarray(x, np.int32)
        best, R, keys = om.search(x, bits, cfg)
        ok = {o: k for o, k in keys.items() if k is not None}
        if ok:
            assert best["subframe_bits"] == min(ok.values()), i
            assert best["o"] == min(o for o, k in ok.items() if k == best["subframe_bits"]), i
        ref = orc.estimated_qlpc(x, bits, cfg)
        c = om.candidate(x, bits, R, order, cfg)
        assert c["status"] == ref["status"], i
        if ref["status"] == 0:
            assert c["subframe_bits"] == ref["subframe_bits"], i
            assert list(c["qp"].coefs[:c["qp"].order]) == list(ref["coefs"]), i
            assert np.array_equal(c["residual"], ref["residual"]), i
            if ok:
                assert best["subframe_bits"] <= ref["subframe_bits"], i


def test_the_corpus_reaches_the_saturated_and_widened_branches():
    """The material above reaches what the GPU tests rely on: saturated chosen levels at small max_p, codes of 2^27
    and more, partition sums of 2^32 and more."""
    got = set()
    for max_p in (0, 4):
        cfg = om.config(order=8, max_rice_parameter=max_p)
        for x in corpus(1, 4097, 24):
            got |= es.branches(x, 24, cfg)
    cfg = om.config(order=24, window="rectangle", quant_precision=12)
    got |= es.branches(es.alternation(4096, 24), 24, cfg)
    assert got >= {"clamp", "ksat", "wide", "rice2", "i24", "i64"}


def _shifted_frames(n, seed):
    x = es.extreme_frames(np.random.default_rng(seed), n, 16).astype(np.int64)
    for f in range(len(x)):
        x[f] <<= f % 4
    return x


@pytest.mark.parametrize("n", [4096, 1000])
def test_composed_model_reduces_to_its_parts(n):
    x = _shifted_frames(n, n)
    for max_p in (0, 4, 30):
        one = om.config(order=1, max_rice_parameter=max_p)
        fc1 = orc.make_frame_config(one, use_fixed=False)
        wfc = wm.frame_config(order=1, use_fixed=False, acorr=orc.ACORR_REFERENCE, max_rice_parameter=max_p)
        fc8 = orc.make_frame_config(om.config(order=8, max_rice_parameter=max_p), use_fixed=False)
        for f in range(len(x)):
            l, r = x[f, 0], x[f, 1]
            assert om.wasted_stereo_frame_bytes(l, r, 24, fc1, number=f) == wm.stereo_frame_bytes(l, r, 24, wfc, number=f)
            if f % 4 == 0 and all(wm.wasted_of(s, fc8) == 0 for s in wm.roles(l, r)):
                assert om.wasted_stereo_frame_bytes(l, r, 24, fc8, number=f) == om.stereo_frame_bytes(l, r, 24, fc8,
                                                                                                       number=f)
