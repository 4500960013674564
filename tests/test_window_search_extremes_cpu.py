"""The deterministic corpus of tests/test_gpu_window_search_extremes.py (tests/window_cases.py) through the model alone,
without a GPU: every case reaches the branches, regimes, winners and ties it names; candidate (0, P) of the window
model is order_model's order-P candidate and the one-window model is order_model.record; the windows that the corpus
calls empty have no non-zero weight in flacenc_hip_lpc_window_weights either; and the random extra-window lists of the
fuzz pass the setter's validation and cover what they promise.  So a drift of a fixture or of a model shows here, and
not as a GPU case that silently stops reaching its branch."""
import numpy as np
import pytest

import extreme_signals as es
import order_model as om
import window_cases as wc
import window_model as wm
from flacenc_rs_amd import _capi

CASES, IDS = wc.expand(wc.all_cases())


def same_bits(a, b):
    return a.dtype == b.dtype == np.float32 and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def check_against_order_model(c, found, orders):
    """Candidate (0, P) is order_model's order-P candidate, from estimated_qlpc's own R."""
    cfg = wc.config(c)
    for i, (_, cands) in enumerate(found):
        x, bps = c.rows[i], wc.row_bps(c, i)
        mine = next(k for k in cands if k["j"] == 0 and k["o"] == c.order)
        R = om.autocorr(x, bps, cfg)
        assert np.array_equal(mine["R"], R), (c.name, i)
        ref = om.candidate(x, bps, R, c.order, cfg)
        assert mine["status"] == ref["status"] == om.STATUS_OK, (c.name, i)
        assert mine["subframe_bits"] == ref["subframe_bits"] and np.array_equal(mine["residual"], ref["residual"])
        assert list(mine["qp"].coefs[:32]) == list(ref["qp"].coefs[:32]) and np.array_equal(mine["coefs"], ref["coefs"])
        if orders:  # ... and the one-window model is order_model.record
            got, gres, gac, glc = wm.record(x, bps, cfg, (), True)
            want, wres, wac, wlc = om.record(x, bps, cfg)
            assert got == want and np.array_equal(gres, wres) and np.array_equal(gac, wac) and np.array_equal(glc, wlc)


@pytest.mark.parametrize("c,orders", CASES, ids=IDS)
def test_case_reaches_what_it_names(c, orders):
    found = wc.claims(c, orders)
    check_against_order_model(c, found, orders)


def test_every_branch_is_won_by_a_window_above_0_somewhere():
    """Otherwise the GPU check of that branch reduces to the one-window one."""
    won = {}
    for c in wc.branch_cases():
        for orders in (False, True):
            for i, (best, _) in enumerate(wc.claims(c, orders)):
                if best["j"] > 0:
                    for b in es.candidate_branches(best, c.rows[i], wc.row_bps(c, i)):
                        won.setdefault(b, (c.name, orders, i))
            if c.avoid >= {"wide", "ksat", "clamp"} and any(b["j"] > 0 for b, _ in wc.claims(c, orders)):
                won.setdefault("proved", (c.name, orders))
    assert set(won) >= {"i24", "i64", "wide", "ksat", "clamp", "rice2", "proved"}, won


def test_regimes_change_in_both_directions_and_a_winner_follows_another_regime():
    pairs, follows = set(), []
    for c in wc.regime_cases():
        for orders in wc.settings(c):
            for i, (best, cands) in enumerate(wc.claims(c, orders)):
                reg = "".join(es.regime(b) for b in es.branches_by_candidate(c.rows[i], wc.row_bps(c, i), wc.config(c),
                                                                              c.extras, orders))
                assert len(reg) == len(cands)
                if c.name not in ("clamp_all", "clamp_none"):  # (every candidate in one regime: the two ends of a scale)
                    assert len(set(reg)) >= 2, (c.name, reg)
                pairs |= set(zip(reg, reg[1:]))
                w = next(k for k, cand in enumerate(cands) if cand is best)
                if w > 0 and reg[w - 1] != reg[w]:
                    follows.append((c.name, reg[w - 1], reg[w]))
    assert pairs >= {("W", "."), ("K", "."), ("C", "."), (".", "W"), (".", "K"), (".", "C")}, pairs
    assert follows, "no winner directly follows a candidate of another regime"


@pytest.mark.parametrize("n", wc.DEAD_SIZES)
def test_dead_entries_have_no_weight_in_the_library_either(n):
    for e in wc.DEAD:
        w = _capi.lpc_window_weights(*e, n)
        assert same_bits(w, wm.weights(e, n)) and not np.any(w), (e, n)
    for c in wc.dead_cases():
        for e in c.extras:
            m = c.rows.shape[1]
            assert same_bits(_capi.lpc_window_weights(*e, m), wm.weights(e, m)), (c.name, e)


@pytest.mark.parametrize("n", wc.SHAPES)
def test_shapes_through_the_model(n):
    c = wc.shape_case(n)
    for orders in (False, True):
        check_against_order_model(c, wc.claims(c, orders), orders)


@pytest.mark.parametrize("order", wc.BUCKET_EDGES)
def test_bucket_edges_through_the_model(order):
    for extras in (wc.E1, wc.E7):
        c = wc.bucket_case(order, extras)
        for orders in (False, True):
            check_against_order_model(c, wc.claims(c, orders), orders)


def test_random_extra_window_lists_are_valid_and_cover_the_degenerate_pieces():
    L = _capi.load()
    lengths, types, alphas, pieces = set(), set(), set(), set()
    for seed in range(200):
        rng = np.random.default_rng(seed)
        n = int(rng.choice(wc.SHAPES))
        extras = wm.random_extras(rng, n)
        assert len(extras) <= _capi.MAX_LPC_WINDOWS - 1
        lengths.add(len(extras))
        out = np.zeros(n, np.float32)
        for t, alpha, start, end in extras:
            assert L.flacenc_hip_lpc_window_weights(t, alpha, start, end, n, out.ctypes.data) == _capi.OK
            assert same_bits(out, wm.weights((t, alpha, start, end), n))
            types.add(t)
            alphas.add(alpha)
            s, e = wm.piece(start, end, n)
            if t == wm.PARTIAL_TUKEY and e - s < 2:
                pieces.add(("partial", e - s))
            if t == wm.PUNCHOUT_TUKEY:
                pieces |= {("head", s)} if s < 2 else set()
                pieces |= {("tail", n - e)} if n - e < 2 else set()
    assert lengths == set(range(8)) and types == {0, 1, 2, 3} and alphas == set(wm.ALPHAS)
    assert pieces == {("partial", 0), ("partial", 1), ("head", 0), ("head", 1), ("tail", 0), ("tail", 1)}
