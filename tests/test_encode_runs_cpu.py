"""The corpus of tests/encode_runs_cases.py without a GPU: the plan rebuilt by brute force from every case's table reaches
the runs the GPU test claims -- every kernel family by a tail run of several frames and by one of a single frame, both
sub-wave forms from mono and from stereo runs, runs of 1, 3 and 5 frames --, every case has a model that is not the
library, and the model's frames parse (tests/flac_parse.py: both CRCs, every field) to their index, their block size and
the input's samples."""
import numpy as np
import pytest

import encode_runs_cases as runs
import encode_streams_cases as cases
import encode_streams_model as model
import flac_parse
from flacenc_rs_amd import _capi

ROUTE_CASES = [c for c in runs.ROUTE_CASES if not c.chunk and not c.short]
FULL_ROUTES = {"A": "fused4608", "B": "subwave72", "C": "bigblock", "D": "bigblock", "E": "bigblock", "F": "bigblock",
               "G": "subwave64"}


def test_route_restates_the_dispatch_rule():
    r = runs.route
    assert [r(4096, o) for o in (1, 8, 12, 13, 32)] == ["fused4096"] * 3 + ["bigblock"] * 2
    assert [r(4608, o) for o in (8, 12, 13)] == ["fused4608", "fused4608", "generic"]
    assert {r(n, 10) for n in (256, 512, 1024, 2048)} == {"subwave64"}
    assert {r(n, 10) for n in (288, 576, 1152, 2304)} == {"subwave72"}
    assert {r(n, 13) for n in runs.SUBWAVE} == {"generic"}        # the sub-wave kernels stop at order 12
    assert {r(n, o) for n in (8192, 16384) for o in (1, 12, 13, 32)} == {"bigblock"}
    assert {r(n, 8) for n in (63, 64, 255, 257, 4095, 4097, 4607, 8191, 32767)} == {"generic"}
    assert r(32, 8) == r(63, 12) == "generic"
    assert set(runs.ROUTES) == {r(n, o) for n in (63, 256, 288, 4096, 4608, 8192) for o in (8, 13)}


def test_the_corpus_reaches_every_route_with_runs_of_several_frames_and_of_one():
    many, one, sizes, by_channels = set(), set(), set(), set()
    for c in ROUTE_CASES:
        plan = runs.brute_plan(c)
        for k, n, frames, tail in plan["runs"]:
            if tail:
                name = runs.route(n, c.order)
                (many if frames >= 2 else one).add(name)
                sizes.add(frames)
                by_channels.add((name, k[0]))
    assert many == set(runs.ROUTES) and one == set(runs.ROUTES), (many, one)
    assert {1, 3, 5} <= sizes
    for form in ("subwave64", "subwave72"):
        assert (form, 1) in by_channels and (form, 2) in by_channels, form


@pytest.mark.parametrize("case", ROUTE_CASES, ids=lambda c: c.name)
def test_a_route_case_holds_what_the_gpu_test_claims(case):
    ss = runs.streams(case)
    plan = runs.brute_plan(case)
    keys = {(s.channels, s.bps, s.width) for s in ss}
    assert (1, 16, 2) in keys and (2, 16, 2) in keys
    assert case.name == "F" or (2, 24, 3) in keys or (3, 16, 4) in keys
    assert any(0 < s.x.shape[1] < case.block for s in ss) and any(s.x.shape[1] == 2 * case.block for s in ss)
    assert all(s.x.shape[1] // case.block <= 2 for s in ss)
    assert case.name != "F" or (len(ss) <= 5 and keys == {(1, 16, 2), (2, 16, 2)})
    assert case.name != "D" or {r[1] for r in plan["runs"] if r[0][1] == 24 and r[3]} == {4096, 2304, 8191}   # 24-bit material
    # every listed tail length ends three streams of one class (F's 4096 is its run of one frame)
    listed = {t for t, _, n in case.groups if n >= 3}
    for t in listed:
        assert any(r[1] == t and r[2] >= 3 and r[3] for r in plan["runs"]), t
    # the full runs take the route the case is about, in every class
    full = {runs.route(n, case.order) for _, n, _, tail in plan["runs"] if not tail}
    assert full == {FULL_ROUTES[case.name[0]]} == {case.full_route}
    assert plan["full_runs"] == len(plan["classes"])
    # the plan agrees with the library's own count and the layout with what the GPU test needs
    lay = runs.layout(ss, case.block, seed=7)
    assert _capi.encode_streams_frames(lay.table, case.block) == plan["frames"]
    assert all(off % 2 == 1 for off, _ in lay.spans) and not runs.slot_map(lay.table, lay.out_bytes).all()


def test_the_chunked_and_the_cut_variant_share_their_streams():
    a, a2 = runs.BY_NAME["A"], runs.BY_NAME["A-chunk2"]
    assert runs.streams(a) is runs.streams(a2)
    p, p2 = runs.brute_plan(a), runs.brute_plan(a2)
    assert {r[2] for r in p["runs"] if r[3]} >= {1, 3, 5} and {r[2] for r in p2["runs"]} == {1, 2}
    assert p2["tail_runs"] > p["tail_runs"] and p2["full_runs"] > p["full_runs"]
    b = runs.BY_NAME["B-short"]
    assert runs.streams(b) is runs.streams(runs.BY_NAME["B"])
    assert any(s.x.shape[1] == b.block + b.short for s in runs.streams(b))


def test_the_config_cases_are_the_listed_ones():
    names = [c.name for c in runs.CONFIG_CASES]
    for order in (1, 10, 12, 16, 32):
        for kind in ("fixed", "lpc"):
            assert "order%d-%s" % (order, kind) in names
    assert runs.BY_NAME["order32-lpc"].flags == _capi.FLAG_ALLOW_ORDER_32 and not runs.BY_NAME["order16-fixed"].flags
    F = _capi
    want = {F.FLAG_WASTED_BITS, F.FLAG_ORDER_SEARCH, F.FLAG_WINDOW_SEARCH, F.FLAG_ORDER_GUESS, F.FLAG_PRECISION_SEARCH,
            F.FLAG_RICE_ESCAPE, F.FLAG_REFERENCE_SUM_ORDER, F.FLAG_GENERIC_KERNEL,
            F.FLAG_WASTED_BITS | F.FLAG_ORDER_GUESS | F.FLAG_WINDOW_SEARCH, F.FLAG_ORDER_SEARCH | F.FLAG_WINDOW_SEARCH,
            F.FLAG_PRECISION_SEARCH | F.FLAG_RICE_ESCAPE}
    flagged = [c for c in runs.CONFIG_CASES if c.material == "flagged"]
    assert {c.flags for c in flagged} == want and len(flagged) == len(want)
    for c in runs.CONFIG_CASES:
        ss = runs.streams(c)
        assert c.block == 576 and {s.x.shape[1] % 576 for s in ss} == {288, 256, 100, 17, 0}
        assert {s.channels for s in ss} >= {1, 2} and len({(s.channels, s.bps, s.width, s.rate) for s in ss}) == 3
        if c.material == "flagged":
            assert c.order == 8 and c.use_fixed and {s.rate for s in ss} == {44100}
            assert any(not (s.x & 15).any() for s in ss)                                   # low bits zero
            assert any((s.x[:, -(s.x.shape[1] % 576 or 576):] == 0).all(0).sum() >= 8 for s in ss)   # silence in a tail
            lo, hi = -(1 << 15), (1 << 15) - 1
            assert any(s.bps == 16 and (s.x == lo).any() and (s.x == hi).any() for s in ss)   # the full-scale block
    for name in runs.DEVICE_TOO + runs.PLANAR_TOO:
        assert name in runs.BY_NAME


@pytest.mark.parametrize("case", [c for c in runs.CASES if not c.chunk and not c.short], ids=lambda c: c.name)
def test_every_case_has_a_model_whose_frames_parse(case):
    """No case falls back to the library as its truth: the share of frames compared only with flacenc_hip_encode_pcm is 0."""
    cfg, mod = model.run_configs(case.order, case.use_fixed, case.flags)
    assert mod is not None, case.name
    assert cfg.qlpc.lpc_order == case.order and bool(cfg.use_fixed) == case.use_fixed
    assert cfg.qlpc.flags & ~_capi.FLAG_ALLOW_ORDER_32 == case.flags & ~_capi.FLAG_ALLOW_ORDER_32
    if case.flags & _capi.FLAG_FUSED_PACK:    # a kernel choice: the frames are the unflagged case's
        assert mod.key == model.run_configs(case.order, case.use_fixed, 0)[1].key
    wasted_ok = bool(case.flags & _capi.FLAG_WASTED_BITS)
    for s in runs.streams(case):
        fr = model.frames(mod, s, case.block)
        assert len(fr) == cases.n_frames(s, case.block)
        for i, f in enumerate(fr):
            p = flac_parse.parse_frame(f, stream_bps=s.bps, stream_rate=s.rate, wasted_ok=wasted_ok)
            x = s.x[:, i * case.block:(i + 1) * case.block]
            assert p["number"] == i and p["length"] == len(f) and p["block_size"] == x.shape[1], (s.name, i)
            assert np.array_equal(p["channels"], x), (s.name, i)


def test_every_flag_that_may_change_the_bytes_changes_them_on_this_material():
    """A batch call that dropped the flag would write the plain frames: they differ, so the GPU test would fail."""
    same_integers = (_capi.FLAG_REFERENCE_SUM_ORDER, _capi.FLAG_GENERIC_KERNEL)
    plain = model.run_configs(8, True, 0)[1]
    for c in runs.CONFIG_CASES:
        if c.material != "flagged" or c.flags in same_integers:
            continue
        mod = model.run_configs(c.order, c.use_fixed, c.flags)[1]
        ss = runs.streams(c)
        assert any(model.frames(mod, s, c.block) != model.frames(plain, s, c.block) for s in ss), c.name
    both = runs.BY_NAME["PRECISION_SEARCH+RICE_ESCAPE"]
    for one in ("PRECISION_SEARCH", "RICE_ESCAPE"):
        a, b = (model.run_configs(8, True, runs.BY_NAME[n].flags)[1] for n in (both.name, one))
        assert any(model.frames(a, s, 576) != model.frames(b, s, 576) for s in runs.streams(both)), one
    # and the orders and use_fixed are configs of their own
    ss = runs.streams(runs.BY_NAME["order10-fixed"])
    stated = {}
    for c in runs.CONFIG_CASES:
        if c.material == "plain":
            mod = model.run_configs(c.order, c.use_fixed, c.flags)[1]
            stated[c.name] = b"".join(b"".join(model.frames(mod, s, c.block)) for s in ss)
    assert len(set(stated.values())) == len(stated)


def test_the_models_of_the_chunked_and_cut_variants_are_their_cases_models():
    for name in ("A-chunk2", "B-short"):
        c, base = runs.BY_NAME[name], runs.BY_NAME[name[0]]
        assert (c.order, c.use_fixed, c.flags, c.block) == (base.order, base.use_fixed, base.flags, base.block)
        assert model.run_configs(c.order, c.use_fixed, c.flags)[1] is not None
