"""FLACENC_HIP_FLAG_ORDER_GUESS without a GPU: the corpus reaches every regime of the rule (tests/guess_cases.py), the
rule's consequences hold in the model (tests/guess_model.py) on the corpus and the golden fixtures, the host build of
flacenc_rs_amd/csrc/order_guess_core.h (g++, plain and under ASan + UBSan) gives the model's eligibility, costs and
guesses bit for bit, the calls of the trace suite (tests/guess_trace_cases.py, run on the GPU by
tests/test_gpu_order_guess_trace.py) reach what they name, and the C ABI's config rules and constants are the header's."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import guess_cases as gc
import guess_model as gm
import guess_trace_cases as tc
import order_model as om
import util
import window_model as wm
from flacenc_rs_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = gc.all_cases()
ALL_REGIMES = {"wins", "loses", "early", "none", "clipped", "short", "differ"}


# ---- 1. regimes ----
@pytest.fixture(scope="module")
def found():
    """claims() of every case, once for the module: {name: (winner, coded candidates, per-window guess records)}."""
    return {c.name: gc.claims(c) for c in CASES}


def test_the_corpus_reaches_every_regime(found):
    assert set().union(*(c.regimes for c in CASES)) == ALL_REGIMES
    assert len(found) == len(CASES)
    assert {c.q for c in CASES} >= {5, 15} and {c.bps for c in CASES} >= {8, 16, 24}


def test_the_chain_helper_is_order_models_candidate():
    # guess_model.levinson states the status and k_o of order_model.candidate without its Rice search
    for c in CASES[:8]:
        cfg = gc.config(c)
        R = wm.autocorr(c.x, wm.config_window(cfg, len(c.x)), cfg)
        for o in range(1, c.order + 1):
            cand = om.candidate(c.x, c.bps, R, o, cfg)
            st, k = gm.levinson(R, o)
            assert st == cand["status"], (c.name, o)
            if st == om.STATUS_OK:
                assert np.float64(k).tobytes() == np.float64(cand["coefs"][o - 1]).tobytes(), (c.name, o)


def test_x_below_the_smallest_normal_float_is_reached_and_costs_nothing():
    # e_o (0.5 / n) below 2^-126: x_o is a subnormal float, log2f is far below zero and b_o clips to +0.0
    tiny = np.float32(np.finfo(np.float32).tiny)
    R = np.array([3.0e-38, 1.5e-38, 0.5e-38], np.float64)
    g = gm.guesses_from_R(R, 2, 4096, 16, 15, 2)
    xs = [np.float32(e * (0.5 / 4096.0)) for e in g["e"]]
    assert g["eligible"] == 2 and all(0 < x < tiny for x in xs)
    assert [float(b) for b in g["b"]] == [0.0, 0.0] and g["cost"] == [31.0, 62.0] and g["guesses"] == [1, 2]


# ---- 2. consequences ----
def bits_of(c):
    return c["subframe_bits"] if c["status"] == om.STATUS_OK else None


@pytest.mark.parametrize("c", CASES, ids=gc.ids(CASES))
def test_between_the_exhaustive_search_and_the_reference_record(c, found):
    cfg = gc.config(c)
    best, cands, _ = found[c.name]
    ref = next(k for k in cands if k["j"] == 0 and k["o"] == c.order)
    exhaustive, every = wm.search(c.x, c.bps, cfg, c.extras, True)
    # the coded candidates are a subset of the exhaustive search's, bit for bit, and contain the reference record
    keys = {(k["j"], k["o"]): bits_of(k) for k in every}
    assert all(keys[(k["j"], k["o"])] == bits_of(k) for k in cands), c.name
    plain = om.candidate(c.x, c.bps, wm.autocorr(c.x, wm.config_window(cfg, len(c.x)), cfg), c.order, cfg)
    assert bits_of(ref) == bits_of(plain)
    if best["status"] == om.STATUS_OK:
        assert exhaustive["subframe_bits"] <= best["subframe_bits"]
        if ref["status"] == om.STATUS_OK:
            assert best["subframe_bits"] <= ref["subframe_bits"]


@pytest.mark.parametrize("name,x,bps,P", [("ar2", gc.ar2(4096), 16, 12), ("music", gc.golden(4096, 4096), 16, 8),
                                          ("white", gc.white(256, 24, 9), 24, 13)])
def test_k_covering_every_eligible_order_is_the_order_search(name, x, bps, P):
    cfg = om.config(order=P)
    x = np.asarray(x, np.int32)
    for extras in ((), wm.DEFAULT[:2]):
        _, _, per_window = gm.search(x, bps, cfg, P, extras)
        assert all(g["eligible"] == P for g in per_window), name  # every order has status 0 and is eligible
        got = gm.record(x, bps, cfg, P, extras)
        want = wm.record(x, bps, cfg, extras, True)
        assert got[0] == want[0] and all(np.array_equal(g, w) for g, w in zip(got[1:], want[1:])), (name, extras)


def test_order_1_without_extra_windows_is_the_reference_record():
    for c in CASES[:8]:
        cfg = om.config(order=1, quant_precision=c.q)
        got = gm.record(c.x, c.bps, cfg, 1)
        want = wm.record(c.x, c.bps, cfg, (), False)
        assert got[0] == want[0] and all(np.array_equal(g, w) for g, w in zip(got[1:], want[1:])), c.name


def test_golden_fixtures_at_order_32_are_strictly_shorter():
    """The first two 4096 blocks of the eight fixture channels, K = 1, Tukey(0.4), precision 15: the guessed records
    total strictly fewer bits than the REFERENCE_SUM_ORDER records (-0.079 % when this was written), and no block is
    longer."""
    cfg = om.config(order=32)
    guess = ref = 0
    for nm in ("ras103", "ras22", "sus109", "sus6"):
        for ch in (0, 1):
            sig = util.test_signal(nm, ch)
            for blk in range(2):
                x = sig[blk * 4096:(blk + 1) * 4096]
                best, cands, _ = gm.search(x, 16, cfg, 1)
                r = next(k for k in cands if k["o"] == 32)
                assert best["subframe_bits"] <= r["subframe_bits"]
                guess += best["subframe_bits"]
                ref += r["subframe_bits"]
    print("order 32, K = 1: %d against %d bits (%+.3f %%)" % (guess, ref, 100.0 * (guess - ref) / ref))
    assert guess < ref


# ---- 2b. the trace suite's calls reach what they name ----
TRACE_CALLS = tc.all_calls()
ALL_REACHED = {"full", "early", "none", "width", "clip_low", "clip_one", "clip_high", "large", "dead", "k_at", "k_below",
               "k_above", "all32", "windows"}


@pytest.mark.parametrize("c", TRACE_CALLS, ids=tc.ids(TRACE_CALLS))
def test_trace_calls_reach_what_they_name(c):
    tc.claims(c)


def test_trace_calls_cover_every_property_entry_and_log2f_table_index():
    assert set().union(*(c.reach for c in TRACE_CALLS)) == ALL_REACHED
    assert {c.entry for c in TRACE_CALLS} == set(tc.ENTRIES)
    assert tc.log2f_indices(TRACE_CALLS) == set(range(16))
    # K = 1 and K = P at every edge of an order bucket, and the ends of the block-size range
    names = {c.name for c in TRACE_CALLS}
    assert all({"bucket_%d_K1" % o, "bucket_%d_K%d" % (o, o)} <= names for o in (1, 2, 8, 9, 12, 13, 16, 17, 24, 25, 32))
    assert {"size_64", "size_65", "size_4096", "size_32767"} <= names


def test_the_side_role_and_the_shifted_rows_cost_what_their_own_width_costs():
    # role 3 of a stereo frame is searched at bits + 1 and a row with k wasted bits at w - k: the model's costs at the
    # frame's own width differ from them in every eligible entry, so a kernel that takes that width shows in the trace
    for c in TRACE_CALLS:
        if c.entry == "batch":
            continue
        cfg = tc.config(c)
        for (x, w), per_window in zip(tc.subframes(c), tc.model(c)):
            if w == c.bps:
                continue
            at_frame_width = gm.search(x, c.bps, cfg, c.K, c.extras)[2]
            for g, f in zip(per_window, at_frame_width):
                assert g["eligible"] == f["eligible"], c.name
                assert all(a != b for a, b in zip(g["cost"], f["cost"])), c.name


def test_the_clip_search_is_reproducible_on_its_first_trials():
    # the two seeds the corpus keeps are trials of clip_noise; a window of the search around them finds them again
    one, eps = np.float32(1.0), np.float32(2.0 ** -10)
    hits = {}
    for seed in (tc.CLIP_BOTH, tc.CLIP_ONE):
        x = tc.clip_noise(seed)
        c = tc.call("trial", "batch", [x], 16, 8)
        xs = tc.xs_of(tc.model(c)[0][0], len(x))
        hits[seed] = [("low" if one - eps < v < one else "one" if v == one else "high" if one < v < one + eps else "")
                      for v in xs]
    assert {"low", "high"} <= set(hits[tc.CLIP_BOTH]) and "one" in hits[tc.CLIP_ONE], hits


# ---- 3. the core header against the model ----
CASE_IN = np.dtype([("P", "<u4"), ("n", "<u4"), ("w", "<u4"), ("q", "<u4"), ("K", "<u4"), ("pad", "<u4"), ("r0", "<f8"),
                    ("k", "<f8", 32), ("status", "<i4", 32)])
CASE_OUT = np.dtype([("eligible", "<u4"), ("mask", "<u4"), ("cost", "<f8", 32)])


def build_driver(out_dir, sanitize):
    exe = os.path.join(out_dir, "order_guess_core_test" + ("_san" if sanitize else ""))
    cmd = ["g++", "-O1" if sanitize else "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Werror",
           "-I", os.path.join(ROOT, "flacenc_rs_amd", "csrc")]
    if sanitize:
        cmd += ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    subprocess.run(cmd + [os.path.join(ROOT, "tests", "host", "order_guess_core_test.cpp"), "-o", exe], check=True,
                   capture_output=True, text=True)
    return exe


def r_vectors(rng, P):
    """R[0..P] vectors of every kind the chain can meet at lpc_order P: autocorrelations of AR(2)-like rows, the same
    scaled far down (x_o subnormal or zero), perturbed until the recursion leaves its stable domain, all zero, and with
    a lag that fails levinson_quantize's status checks."""
    out = []
    for kind in range(7):
        x = np.cumsum(rng.standard_normal(200)) * 50 + rng.standard_normal(200) * float(rng.uniform(1, 400))
        R = np.array([float(np.dot(x[P:], x[P - lag:len(x) - lag])) for lag in range(P + 1)])
        if kind == 1:
            R *= 1e-40
        elif kind == 2:
            R *= 2.0 ** -1000
        elif kind == 3:
            R[1:] += rng.standard_normal(P) * R[0] * 0.3
        elif kind == 4:
            R[:] = 0.0
        elif kind == 5:
            R[int(rng.integers(0, P + 1))] = (np.nan, np.inf, -np.inf)[int(rng.integers(0, 3))]
        elif kind == 6:
            R[0] = -R[0] if rng.random() < 0.5 else 0.0
        out.append(R)
    return out


def model_cases():
    """-> (CASE_IN records, the model's (eligible, guesses, costs) per record)."""
    rows, want = [], []

    def add(R, P, n, w, q, K):
        lev = lev_cache.setdefault((R.tobytes(), P), [gm.levinson(R, o) for o in range(1, P + 1)])
        ks, sts = [k for _, k in lev], [st for st, _ in lev]
        key = (R.tobytes(), P, n, w, q)
        if key not in chain_cache:
            chain_cache[key] = gm.chain(R[0], ks, sts, n, w, q)
        m, _, _, costs = chain_cache[key]
        rec = np.zeros((), CASE_IN)
        rec["P"], rec["n"], rec["w"], rec["q"], rec["K"], rec["r0"] = P, n, w, q, K, R[0]
        rec["k"][:P] = ks
        rec["status"][:P] = sts
        rows.append(rec)
        want.append((m, gm.pick(costs, K), costs))

    lev_cache, chain_cache = {}, {}
    for c in CASES:  # the corpus, every window
        cfg = gc.config(c)
        for wts in gm.windows(cfg, len(c.x), c.extras):
            add(wm.autocorr(c.x, wts, cfg), c.order, len(c.x), c.bps, c.q, c.K)
    rng = np.random.default_rng(0x6E55)
    for P in range(1, 33):
        for R in r_vectors(rng, P):
            for n in (64, 4096, 32767):
                for w in (4, 16, 25):
                    for q in (1, 15):
                        for K in sorted({1, 2, P, 32}):
                            add(R, P, n, w, q, K)
    return np.array(rows, CASE_IN), want


@pytest.fixture(scope="module")
def core_cases():
    return model_cases()


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_core_header_gives_the_models_guesses_bit_for_bit(tmp_path, core_cases, sanitize):
    rows, want = core_cases
    exe = build_driver(str(tmp_path), sanitize)
    src, dst = str(tmp_path / "cases.bin"), str(tmp_path / "answers.bin")
    with open(src, "wb") as f:
        f.write(np.array([len(rows), 0], "<u4").tobytes())
        f.write(rows.tobytes())
    p = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    got = np.fromfile(dst, CASE_OUT)
    assert len(got) == len(rows)
    seen_early = seen_none = seen_full = 0
    for i, (m, guesses, costs) in enumerate(want):
        where = (i, int(rows[i]["P"]), int(rows[i]["n"]), int(rows[i]["w"]), int(rows[i]["q"]), int(rows[i]["K"]))
        assert int(got[i]["eligible"]) == m, where
        assert [o for o in range(1, 33) if (int(got[i]["mask"]) >> (o - 1)) & 1] == guesses, where
        assert got[i]["cost"][:m].tobytes() == np.array(costs, "<f8").tobytes(), where
        seen_none += m == 0
        seen_full += m == int(rows[i]["P"])
        seen_early += 0 < m < int(rows[i]["P"])
    assert seen_none and seen_full and seen_early


# ---- 4. config rules through the C ABI ----
def header_define(name):
    text = open(os.path.join(ROOT, "include", "flacenc_hip.h")).read()
    return int(re.search(r"#define\s+%s\s+(\d+)u?\b" % name, text).group(1))


def test_constants_are_the_headers():
    assert _capi.FLAG_ORDER_GUESS == header_define("FLACENC_HIP_FLAG_ORDER_GUESS") == 4096
    assert _capi.ABI_VERSION == header_define("FLACENC_HIP_ABI_VERSION") == 6
    assert "flacenc_hip_set_order_guesses" in _capi.EXPORTED_SYMBOLS
    others = [getattr(_capi, k) for k in dir(_capi) if k.startswith("FLAG_") and k != "FLAG_ORDER_GUESS"]
    assert all(_capi.FLAG_ORDER_GUESS & f == 0 for f in others)


def test_verify_config_rules():
    G, OS, WS = _capi.FLAG_ORDER_GUESS, _capi.FLAG_ORDER_SEARCH, _capi.FLAG_WINDOW_SEARCH
    ok = lambda **kw: _capi.verify_config(_capi.make_config(**kw))  # noqa: E731
    assert ok(lpc_order=12, flags=G) == _capi.OK
    assert ok(lpc_order=32, flags=G | WS) == _capi.OK
    assert ok(lpc_order=12, flags=G | _capi.FLAG_NIGHTLY_SUM_ORDER) == _capi.OK
    assert ok(lpc_order=12, flags=G | _capi.FLAG_WASTED_BITS | _capi.FLAG_FUSED_PACK) == _capi.OK
    assert ok(lpc_order=12, flags=G | OS) == _capi.ERR_BAD_CONFIG
    assert ok(lpc_order=12, flags=G | OS | WS) == _capi.ERR_BAD_CONFIG
    assert ok(lpc_order=12, flags=G, use_direct_mse=True) == _capi.ERR_UNSUPPORTED
    assert ok(lpc_order=12, flags=G | WS, use_direct_mse=True) == _capi.ERR_UNSUPPORTED
    # without the flag the sibling rules are what they were
    assert ok(lpc_order=12, flags=OS | WS) == _capi.OK and ok(lpc_order=12, flags=OS, use_direct_mse=True) == _capi.ERR_UNSUPPORTED


def test_the_setter_refuses_a_null_handle():
    lib = _capi.load()
    for k in (0, 1, 32, 33):
        assert lib.flacenc_hip_set_order_guesses(None, k) == _capi.ERR_BAD_ARGUMENT
