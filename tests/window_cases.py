"""The deterministic corpus of the window-search extremes suites (tests/test_gpu_window_search_extremes.py on the GPU,
tests/test_window_search_extremes_cpu.py through the model alone): every case names the rows, the configuration, the
extra-window list and what the model must say about it -- the branches of order_search_kernel it reaches, the regime of
every candidate in kernel order, the winning (window, order), the ties.  claims(case, orders) asserts all of it from
tests/window_model.py on the CPU, so a GPU case proves that it reaches what it names before it compares a byte."""
import collections

import numpy as np

import extreme_signals as es
import order_model as om
import util
import window_model as wm

E1 = ((wm.PARTIAL_TUKEY, 0.5, 0, 32768),)
E3 = ((wm.RECTANGLE, 0.0, 0, 0), (wm.PARTIAL_TUKEY, 0.5, 0, 40000), (wm.PUNCHOUT_TUKEY, 0.1, 20000, 30000))
E5 = wm.DEFAULT
E7 = wm.DEFAULT + ((wm.PARTIAL_TUKEY, 1.0, 16384, 49152), (wm.PUNCHOUT_TUKEY, 0.0, 100, 65000))
# windows a few weights away from the rectangle: a full-scale alternation's order-24 / 32 residual then wraps under some
# of them and not under others
NEAR = ((wm.TUKEY, 0.001, 0, 0), (wm.TUKEY, 0.004, 0, 0), (wm.TUKEY, 0.01, 0, 0), (wm.TUKEY, 0.02, 0, 0),
        (wm.PUNCHOUT_TUKEY, 0.0, 32768, 32784), (wm.PUNCHOUT_TUKEY, 0.0, 16, 32), (wm.PARTIAL_TUKEY, 0.0, 0, 65520))
# entries without a non-zero weight on blocks of 64, 65 and 127 samples: the piece is empty, or shorter than 2 samples,
# or two samples long (a Tukey table's end points are zero)
DEAD = ((wm.PARTIAL_TUKEY, 0.5, 0, 1000), (wm.PARTIAL_TUKEY, 0.5, 0, 1025), (wm.PARTIAL_TUKEY, 0.5, 30000, 31000),
        (wm.PUNCHOUT_TUKEY, 0.5, 0, 65536))
DEAD_SIZES = (64, 65, 127)

# name, rows [k][n], bps (one or per row), lpc_order, extra windows, config keywords, and the claims:
#   reach / avoid: branches in the union over every row and candidate / in none
#   rows_reach / rows_avoid: per row, branches of every candidate with status 0 / of none
#   win: {orders: [(window, order) per row]};  regime: {orders: [string per row]} (order search: windows joined by " ")
#   tie: the settings of the orders switch under which every row's minimum is shared between windows;  zero: windows whose R_j is all zero and whose candidates are the
#   zero predictor -- a tuple for every row (entries without a non-zero weight), or a list of tuples per row
Case = collections.namedtuple("Case", "name rows bps order extras kw reach avoid rows_reach rows_avoid win regime tie "
                                      "zero")


def case(name, rows, bps, order, extras, kw=None, reach=(), avoid=(), rows_reach=None, rows_avoid=None, win=None,
         regime=None, tie=(), zero=()):
    rows = np.ascontiguousarray(np.asarray(rows, np.int64).astype(np.int32))
    return Case(name, rows, bps, order, tuple(extras), dict(kw or {}), reach, set(avoid), rows_reach, rows_avoid,
                win, regime, tie, zero)


def sine(n, amp, period=37.0, phase=0.0):
    return np.round(np.sin(np.arange(n) * 2 * np.pi / period + phase) * amp).astype(np.int64)


def half_alternation(n):
    """The reverse of [zeros(n / 2), alternation(n - n / 2, 24)]: full scale first, then digital silence."""
    return np.r_[np.zeros(n // 2, np.int64), es.alternation(n - n // 2, 24)][::-1]


def impulse(n, t, v=8000000):
    x = np.zeros(n, np.int64)
    x[t] = v
    return x


# ---- a: one case per branch ----
def branch_cases():
    n = 4096
    lo24 = sine(n, (1 << 23) - 1)
    at24 = lo24.copy()
    at24[777] = -(1 << 23)
    out = [
        # maxabs < 2^23 with a small sum of |c| (precision 3): v_mad_i32_i24; one sample at -2^23: the i64 path
        case("i24_at_2_23", [lo24, at24], 24, 2, E7, dict(quant_precision=3, window="rectangle"),
             rows_reach=[{"i24"}, {"i64"}], rows_avoid=[{"i64"}, {"i24"}],
             win={False: [(7, 2), (7, 2)], True: [(7, 2), (7, 2)]}),
        # maxabs . sum|c| on both sides of 2^31 - 1 with maxabs < 2^23; no candidate leaves the proved window
        case("i24_product", [sine(n, 3000), sine(n, 1 << 22)], 24, 8, E5, avoid={"wide", "ksat", "clamp"},
             rows_reach=[{"i24"}, {"i64"}], rows_avoid=[{"i64"}, {"i24"}],
             win={False: [(1, 8), (4, 8)], True: [(1, 8), (1, 3)]}),
        # ordinary material, 16 and 24 bit: the window stays as proved in every window
        case("proved_window", [es.music(n, 16, start=0), es.music(n, 16, start=n), es.music(n, 24, start=0),
                               es.music(n, 24, start=5 * n)], np.array([16, 16, 24, 24], np.uint8), 8, E5,
             avoid={"wide", "ksat", "clamp"},
             win={False: [(0, 8), (0, 8), (0, 8), (4, 8)], True: [(0, 8), (0, 8), (0, 8), (4, 8)]}),
    ]
    # full-scale alternation: a high order's residual wraps i32, codes >= 2^27 -> the wide key's quotient pass, RICE2
    for bits, order, window, precision, win in [
            (24, 24, "rectangle", 12, {False: [(4, 24), (4, 24)], True: [(0, 2), (0, 2)]}),
            (24, 32, ("tukey", 0.0), 8, {False: [(1, 32), (3, 32)], True: [(4, 21), (4, 21)]}),
            (25, 32, ("tukey", 1.0), 5, {False: [(2, 32), (0, 32)], True: [(0, 1), (0, 1)]}),
            (25, 24, "rectangle", 3, {False: [(1, 24), (0, 24)], True: [(0, 2), (0, 1)]})]:
        x = es.alternation(n, bits)
        out.append(case("wide_%d_%d" % (bits, order), [x, -x - 1], bits, order, E5,
                        dict(window=window, quant_precision=precision),
                        # (25 bits under Tukey(1.0): only some lower orders' residuals wrap)
                        reach={False: {"rice2"}, True: {"wide", "rice2"}} if (bits, order) == (25, 32) else {"wide", "rice2"},
                        win=win))
    # every window wide, and a wide candidate of window 1 the shortest
    out.append(case("wide_winner", [-es.alternation(n, 24) - 1], 24, 24, (NEAR[6], NEAR[5]),
                    dict(window="rectangle", quant_precision=8), reach={"wide"}, win={False: [(1, 24)]},
                    regime={False: ["WWW"]}))
    # odd n: one partition; noise residuals sum past 2^32 with codes below 2^27 -> kSat alone, in every candidate
    for m, bits, win in [(4097, 22, {False: [(0, 8), (1, 8)], True: [(0, 1), (1, 1)]}),
                         (4095, 22, {False: [(0, 8), (0, 8)], True: [(3, 1), (3, 1)]}),
                         (32767, 20, None)]:
        out.append(case("ksat_%d" % m, [es.noise(m, bits, seed=m + k) for k in range(2)], 24, 8, E3,
                        reach={"ksat"}, avoid={"wide"}, rows_reach=[{"ksat"}] * 2, win=win))
    # 24- / 25-bit material with max_rice_parameter far below its scale: the chosen level's entries saturate
    clamp_win = {4096: {o: [(4, 8)] * 3 for o in (False, True)},
                 1000: {o: [(5, 8), (0, 8), (4, 8)] for o in (False, True)}}
    for m in (4096, 4097, 1000):
        for max_p in (0, 1, 2, 4):
            out.append(case("clamp_%d_%d" % (m, max_p),
                            [es.music(m, 24, start=0), es.music(m, 24, start=5 * m), es.noise(m, 24, seed=m)], 24, 8, E5,
                            dict(max_rice_parameter=max_p), reach={"clamp"}, avoid={"wide"},
                            rows_reach=[set(), set(), {"clamp"}], win=clamp_win.get(m)))
            out.append(case("clamp25_%d_%d" % (m, max_p), [es.noise(m, 25, seed=m + 1)], 25, 12, E3,
                            dict(max_rice_parameter=max_p), reach={"clamp"}))
    return out


# ---- b: candidates of one subframe in different regimes ----
def regime_cases():
    n = 4096
    m24 = [es.music(n, 24, start=0), es.music(n, 24, start=5 * n)]
    return [
        # the winner (window 1) directly follows a wide candidate
        case("wide_then_clean", [es.alternation(n, 24)], 24, 32, E5, dict(window=("tukey", 0.0), quant_precision=8),
             win={False: [(1, 32)]}, regime={False: ["W....."]}),
        # clean orders 1..16, then wide ones, then the next window's clean order 1
        case("clean_then_wide", [es.alternation(n, 24)], 24, 24, E5, dict(window="rectangle", quant_precision=12),
             win={True: [(0, 2)]}, regime={True: [" ".join(["." * 16 + "W" * 8] + ["." * 24] * 5)]}),
        case("wide_first_of_8", [half_alternation(4096)], 24, 12, E7, dict(window="rectangle", quant_precision=12),
             win={False: [(4, 12)]}, regime={False: ["W......."]}),
        case("ksat_last_of_8", [half_alternation(4097)], 24, 12, E7, dict(window="rectangle", quant_precision=12),
             win={False: [(6, 12)]}, regime={False: [".......K"]}),
        case("ksat_low_orders_32767", [es.music(32767, 24)], 24, 32, E7,
             # (kSat at orders 1..3 of the first seven windows, at all but order 10 under the alpha-0 punch-out)
             win={True: [(4, 31)]}, regime={True: [" ".join(["KKK" + "." * 29] * 7 + ["K" * 9 + "." + "K" * 22])]}),
        # wide, kSat and clean candidates side by side under near-rectangular windows
        case("near_24", [-es.alternation(n, 24) - 1], 24, 24, NEAR, dict(window="rectangle", quant_precision=12),
             win={False: [(3, 24)]}, regime={False: ["W.....KW"]}),
        case("near_25", [es.alternation(n, 25), -es.alternation(n, 25) - 1], 25, 24, NEAR,
             dict(window="rectangle", quant_precision=3), win={False: [(3, 24), (0, 24)]},
             regime={False: ["WK....WW", ".K.....K"]}),
        # every candidate saturated at max_rice_parameter 0, none at 2 on the same rows
        case("clamp_all", m24, 24, 8, E5, dict(max_rice_parameter=0),
             win={False: [(4, 8)] * 2, True: [(4, 8)] * 2},
             regime={False: ["CCCCCC"] * 2, True: [" ".join(["C" * 8] * 6)] * 2}),
        case("clamp_none", m24[:1], 24, 8, E5, dict(max_rice_parameter=2), avoid={"clamp"},
             win={False: [(4, 8)], True: [(4, 8)]}),
        # saturated low orders, clean high orders, in every window: clean -> clamp at each window's first candidate
        case("clamp_low_orders", [es.music(n, 24, start=0)], 24, 8, E5, dict(max_rice_parameter=1),
             win={True: [(4, 8)]}, regime={True: [" ".join(["CCCC...."] * 6)]}),
        case("clamp_order_1_only", [es.music(1000, 24, start=0), es.music(1000, 24, start=5000)], 24, 8, E5,
             dict(max_rice_parameter=0), win={True: [(5, 8), (0, 8)]}, regime={True: [" ".join(["C......."] * 6)] * 2}),
    ]


# ---- c: ties ----
TIED_MUSIC = ((65, 16, 16, 2, 2755), (65, 16, 12, 2, 42459), (97, 8, 32, 1, 83823), (127, 16, 16, 1, 92411))


def tie_cases():
    n = 4096
    # E7's last entry punches out samples [6, 4062) of 4096: impulses in its head, inside the punched-out piece (and
    # inside each of the default list's three), and in its tail
    rows = [np.zeros(n, np.int64), np.full(n, 1234), np.full(n, -(1 << 23)), impulse(n, 3), impulse(n, 100),
            impulse(n, 2000), impulse(n, 4000), impulse(n, 4090)]
    out = [case("degenerate_%s" % name, rows, 24, 8, E7, dict(window=window), tie=(False, True))
           for name, window in (("rectangle", "rectangle"), ("tukey", ("tukey", 0.4)))]
    # short blocks of music where several candidates tie exactly
    for n2, bits, P, prec, start in TIED_MUSIC:
        out.append(case("music_%d_%d" % (n2, P), [es.music(n2, bits, start=start)], bits, P, E5,
                        dict(quant_precision=prec), tie=(True,)))
    plateau = np.load(util.GOLDEN + "/cert_nonpd_plateau_24bit.npy").astype(np.int64).reshape(-1)[:n]
    out.append(case("plateau", [plateau, plateau[::-1]], 24, 12, E5))
    return out


# ---- d: windows without a non-zero weight ----
def dead_cases():
    out = []
    live = (wm.TUKEY, 0.2, 0, 0)
    for n in DEAD_SIZES:
        rows = [es.music(n, 16, start=7 * n), es.music(n, 16, start=900 * n), es.noise(n, 16, seed=n)]
        for k, e in enumerate(DEAD):
            out.append(case("dead_%d_alone_%d" % (n, k), rows, 16, 8, (e,), zero=(1,)))
        mixed = (DEAD[0], live, DEAD[1], E1[0], DEAD[2], E5[3], DEAD[3])
        out.append(case("dead_%d_mixed" % n, rows, 16, 8, mixed, zero=(1, 3, 5, 7)))
    # a partial window over the silent half of a half-silent block
    for n in (4096, 1000):
        x = es.music(n, 16, start=n)
        x[: n // 2] = 0
        out.append(case("silent_half_%d" % n, [x, x[::-1]], 16, 8, (E1[0], (wm.PARTIAL_TUKEY, 0.5, 32768, 65536)),
                        zero=[(1,), (2,)]))
    return out


# ---- e: shapes ----
SHAPES = [64, 65, 97, 127, 1000, 4095, 4096, 4097, 4160, 4608, 6144, 8192, 16383, 16384] + list(es.lds_edge()) + \
    [24576, 32767]
BUCKET_EDGES = [1, 2, 8, 9, 12, 13, 16, 17, 24, 25, 32]


def shape_case(n):
    """The order-search suite's shapes with three extra windows, order 32 from 8192 up and per-row bps."""
    rows = [es.music(n, 24, start=n), es.alternation(n, 24), es.noise(n, 24, seed=n), es.music(n, 16, start=2 * n),
            es.extreme_frames(np.random.default_rng(n), n, 16)[0, 0]]
    return case("shape_%d" % n, rows, np.array([24, 24, 24, 16, 17], np.uint8), 32 if n >= 8192 else 12, E3,
                dict(window="rectangle", quant_precision=12))


def bucket_case(order, extras):
    n = 4096
    rows = [es.music(n, 24, start=order * n), es.music(n, 16, start=3 * order * n), es.alternation(n, 24)]
    return case("bucket_%d_W%d" % (order, len(extras) + 1), rows, np.array([24, 16, 24], np.uint8), order, extras,
                dict(window="rectangle", quant_precision=12))


# ---- the claims ----
def config(c):
    return om.config(order=c.order, **c.kw)


def row_bps(c, i):
    return int(c.bps[i]) if np.ndim(c.bps) else c.bps


def split(reg, c, orders):
    return " ".join(reg[k:k + c.order] for k in range(0, len(reg), c.order)) if orders else reg


def claims(c, orders):
    """Assert from the model everything case c names under one setting of the orders switch; -> [(winner, every
    candidate)] per row."""
    cfg = config(c)
    assert (c.win or {}).keys() | (c.regime or {}).keys() <= {False, True}
    union, found = set(), []
    for i, x in enumerate(c.rows):
        bps = row_bps(c, i)
        best, cands = wm.search(x, bps, cfg, c.extras, orders)
        found.append((best, cands))
        assert all(k["status"] == om.STATUS_OK for k in cands), (c.name, i)  # (finite integer input: always 0)
        br = [es.candidate_branches(k, x, bps) for k in cands]
        union |= set().union(*br)
        if c.rows_reach:
            assert all(b >= c.rows_reach[i] for b in br), (c.name, orders, i)
        if c.rows_avoid:
            assert all(b.isdisjoint(c.rows_avoid[i]) for b in br), (c.name, orders, i)
        if c.win and c.win.get(orders):
            assert (best["j"], best["o"]) == c.win[orders][i], (c.name, orders, i, best["j"], best["o"])
        if c.regime and c.regime.get(orders):
            got = split("".join(es.regime(b) for b in br), c, orders)
            assert got == c.regime[orders][i], (c.name, orders, i, got)
        low = min(k["subframe_bits"] for k in cands)
        at_min = [(k["j"], k["o"]) for k in cands if k["subframe_bits"] == low]
        assert (best["j"], best["o"]) == min(at_min), (c.name, orders, i)
        if orders in c.tie:
            assert len({j for j, _ in at_min}) > 1, (c.name, orders, i, at_min)
        for j in (c.zero[i] if isinstance(c.zero, list) else c.zero):
            of_j = [k for k in cands if k["j"] == j]
            assert all(not np.any(k["R"]) and not np.any(k["qp"].coefs[:32]) for k in of_j), (c.name, i, j)
            if not isinstance(c.zero, list):
                assert not np.any(wm.weights(c.extras[j - 1], len(x))), (c.name, j)
    reach = c.reach[orders] if isinstance(c.reach, dict) else set(c.reach)
    assert union >= reach and union.isdisjoint(c.avoid), (c.name, orders, union)
    return found


def settings(c):
    """The settings of the orders switch a case is run under: both, or the ones its regime strings name."""
    return sorted(c.regime) if c.regime else [False, True]


def all_cases():
    return branch_cases() + regime_cases() + tie_cases() + dead_cases()


def expand(cases):
    """-> pytest parameters (case, orders) and their ids."""
    params = [(c, o) for c in cases for o in settings(c)]
    return params, ["%s-%s" % (c.name, "orders" if o else "P") for c, o in params]
