"""The corpus of tests/recover_long_cases.py without a GPU: the model (tests/recover_model.py) says that every batch
reaches the seam it is there for, and broken variants of rules 3 to 5 -- a prefix maximum that forgets what lies in front
of a workgroup, a running sum that restarts at element 1024, a chain walk that stops at jump level 6 -- written here as
plain loops, each give another expectation for the batch aimed at them: a kernel wrong in that way cannot pass
tests/test_gpu_recover_long.py.  The one variant no batch can reach, a maximum lost at element 262 144, is shown on the
reference of the scan's own test (tests/segmax_cases.py)."""
import functools
import os
import re

import numpy as np

import recover_long_cases as lc
import recover_model as model
import segmax_cases as sc
from flacenc_rs_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WG = 256       # frames per workgroup of the segmented max-scan
ROUND = 1024   # elements per round of the one-workgroup scans
PIECE = 4096
MANY_QUARTER = (150, 300)   # "about every 4th" of 1200, less the empty, junk and capacity-0 streams among them


def chain_frames(t):
    return t[0] + t[3]


def heads(want):
    """The sequence position of every stream's first chain frame (of a one-class batch): the running sum of
    totals[0] + totals[3] in table order."""
    return [int(v) for v in np.concatenate([[0], np.cumsum([chain_frames(t) for _, t, _ in want])])[:-1]]


@functools.lru_cache(None)
def chains(name):
    batch, _ = lc.all_batches()[name]
    return [model.chain(model.verified(s.data, s.channels, s.bps)) for s in batch.streams]


# ---------------------------------------------------------------- rules 3 to 5 as loops over the frame sequence
def placed_flags(name, reset=None, keep=None):
    """Rules 3 and 4 over the batch's frame sequence -> per stream, per chain frame: is it placed.  reset: the running
    maximum falls back to the origin at every sequence position that is a multiple of it and no head.  keep: a chain
    ends behind its first `keep` frames."""
    batch, origins = lc.all_batches()[name]
    out, m = [], 0
    for s, origin, frames in zip(batch.streams, origins, chains(name)):
        top, flags = origin, []
        for k, f in enumerate(frames[:keep]):
            if reset and k and m % reset == 0:
                top = origin
            P = f.number if f.variable else f.number * s.mbs
            flags.append(f.block <= s.mbs and P >= origin and P >= top)
            top = max(top, P + f.block)
            m += 1
        out.append(flags)
    return out


def placement(name, reset=None, keep=None):
    """-> per stream (frames placed, frames dropped) of a roomy batch."""
    return [(sum(f), len(f) - sum(f)) for f in placed_flags(name, reset, keep)]


def exclusive_sum(x, restart=None):
    out, at = [], 0
    for i, v in enumerate(x):
        if restart and i == restart:
            at = 0
        out.append(at)
        at += v
    return out + [at]


def written_by_scan(name, restart=None):
    """totals[0] of a roomy batch as the call forms it: pl[first + count] - pl[first], pl the exclusive sum of the
    placement flags over the frame sequence."""
    flags, first = [], [0]
    for f in placed_flags(name):
        flags += [int(x) for x in f]
        first.append(len(flags))
    pl = exclusive_sum(flags, restart)
    return [pl[b] - pl[a] for a, b in zip(first, first[1:])]


def records_by_scan(want, restart=None):
    """The gap table as the call fills it: stream s's k-th gap at gbase[s] + k, gbase the exclusive sum of the gaps per
    stream.  -> {index: record}"""
    gbase = exclusive_sum([len(g) for _, _, g in want], restart)
    out = {}
    for s, (_, _, gaps) in enumerate(want):
        for k, (a, n) in enumerate(gaps):
            out[gbase[s] + k] = (s, a, n)   # a later stream overwrites: what a table written in any order may end as
    return out


# ---------------------------------------------------------------- the corpus' claims
def test_seams_puts_heads_and_runs_where_the_scan_has_its_seams():
    batch, origins, names = lc.seams_batch()
    want = lc.wanted("seams")
    assert {s.channels for s in batch.streams} == {1} and not any(origins)
    at = dict(zip(names, heads(want)))
    assert set(lc.HEADS) <= set(at.values())
    assert {p % WG for p in at.values()} >= {0, 1, WG - 1}             # first, second and last element of a workgroup
    assert at["one at 1024"] == ROUND
    # roomy: nothing is cut
    assert all(t[6] == 0 for _, t, _ in want)
    # the spike: the hand-counted totals, a head that is no workgroup's first element, and a dropped run -- chain
    # frames 6 .. 701 -- that covers two whole workgroups, neither of which holds a head
    spike = names.index("spike")
    assert (want[spike][1], want[spike][2]) == lc.SPIKE_WANT
    head = at["spike"]
    assert head == lc.SPIKE_HEAD and head % WG
    run = range(head + 6, head + 6 + 696)
    dropped = [not x for x in placed_flags("seams")[spike]]
    assert sum(dropped) == 696 and all(dropped[6:702]) and not dropped[5] and not dropped[702]
    whole = [b for b in range(run[0] // WG, run[-1] // WG + 1) if b * WG >= run[0] and (b + 1) * WG - 1 <= run[-1]]
    assert len(whole) >= 2 and not any(b * WG <= p < (b + 1) * WG for b in whole for p in at.values())
    # ... whose placement hangs on a maximum from in front of them: the frame behind the run is placed against it
    assert want[spike][1][0] == 5 + 1 + 99
    # the long restart, the gap stream, the worn one and the undamaged one
    t = {n: w[1] for n, w in zip(names, want)}
    assert t["restart"][:4] == [900, 900 * lc.BLOCK, 0, 300]
    assert t["gap"][:4] == [703, 1400 * lc.BLOCK, 697 * lc.BLOCK, 0] and want[names.index("gap")][2] == [(48, 697 * 16)]
    assert chain_frames(t["worn"]) >= 1100 and t["worn"][3] >= 20 and len(want[names.index("worn")][2]) >= 10
    assert t["undamaged"] == [1100, 1100 * lc.BLOCK, 0, 0, 0, 0, 0, 0]
    # chains reach bit 10 of a frame's index: jump levels 6 to 10 are walked
    assert max(chain_frames(x) for x in t.values()) >= 1 << 10
    assert sum(chain_frames(x) >= 1 << 10 for x in t.values()) >= 3
    # placed frames, dropped frames and gaps on both sides of sequence position 1024
    for side in (lambda p: p < ROUND, lambda p: p >= ROUND):
        mine = [w for w, p in zip(want, heads(want)) if side(p)]
        assert sum(w[1][0] for w in mine) > 0 and sum(len(w[2]) for w in mine) > 0
    assert sum(len(w[2]) for w, p in zip(want, heads(want)) if p < ROUND and p + chain_frames(w[1]) <= ROUND) >= 3
    assert sum(chain_frames(w[1]) for w in want) < 10000


def test_cuts_bisect_over_the_plateau():
    sp = lc.spike_numbers()
    assert lc.PLATEAU == (sp[5] + 1) * lc.BLOCK
    want = dict(zip(lc.cut_capacities("spike"), lc.wanted("cuts spike")))
    # the slot ends on the plateau: the spike is written, and the cut lies behind all 696 equal elements
    for cap in (lc.PLATEAU, lc.PLATEAU + 1):
        assert want[cap][1] == [6, lc.PLATEAU, lc.SPIKE_WANT[0][2], 696, 0, 0, _capi.DECODE_NO_ROOM, 0]
    # one byte less, the last dropped frame's would-be end, a dropped frame's end far below: the cut is the spike
    for cap in (lc.PLATEAU - 1, 700 * lc.BLOCK, (sp[256] + 1) * lc.BLOCK):
        assert want[cap][1] == [5, 5 * lc.BLOCK, 0, 696, 0, 0, _capi.DECODE_NO_ROOM, 0]
    assert want[800 * lc.BLOCK - 1][1][:2] == [104, 799 * lc.BLOCK] and want[800 * lc.BLOCK - 1][1][6]
    assert want[800 * lc.BLOCK][1] == want[800 * lc.BLOCK + 1][1] == lc.SPIKE_WANT[0]
    # the cut as the bisection's answer: the first chain frame whose prefix maximum lies beyond the slot
    cuts = set()
    frames = chains("cuts spike")[0]
    emax = np.maximum.accumulate([(f.number + 1) * lc.BLOCK for f in frames])
    assert (emax[5:702] == lc.PLATEAU).all() and emax[4] < lc.PLATEAU < emax[702]
    for cap, (_, t, _) in want.items():
        cut = int(np.searchsorted(emax, cap, side="right"))
        assert sum(1 for k in range(cut) if k <= 5 or k >= 702) == t[0]
        cuts.add(cut)
    assert cuts == {5, 702, 800, 801}      # in front of the plateau, directly behind it, the last frame, none
    # the gap stream: every placed frame's end around chain index 256 and the last, to the sample
    gp = lc.gap_numbers()
    caps = lc.cut_capacities("gap")
    written = [t[0] for _, t, _ in lc.wanted("cuts gap")]
    assert written == [k + d for k in (255, 256, 257, 702) for d in (0, 1, 1)]
    assert caps[1] == (gp[255] + 1) * lc.BLOCK and len(set(written)) == 6
    for name in ("cuts spike", "cuts gap"):
        assert sum(chain_frames(t) for _, t, _ in lc.wanted(name)) < 10000


def test_many_has_live_data_on_both_sides_of_stream_1024():
    batch, origins = lc.many_batch()
    want = lc.wanted("many")
    assert len(batch.streams) >= 1100 and {s.channels for s in batch.streams} == {1}
    assert all(chain_frames(t) <= 2 for _, t, _ in want)
    for part in (want[:ROUND], want[ROUND:]):
        assert sum(len(g) for _, _, g in part) > 0 and sum(len(b) for b, _, _ in part) > 0
        assert sum(chain_frames(t) for _, t, _ in part) > 0
    assert sum(chain_frames(t) for _, t, _ in want) > ROUND      # the scans over frames pass their seam as well
    leading = sum(1 for _, _, g in want if g and g[0][0] == 0)
    assert MANY_QUARTER[0] <= leading <= MANY_QUARTER[1]
    assert sum(1 for s in batch.streams if len(s.data) == 0) >= 300                      # empty spans
    assert sum(1 for (_, t, _), s in zip(want, batch.streams) if t[4] == len(s.data) > 0) >= 50   # junk only
    zero = [t for (_, t, _), c in zip(want, batch.capacities) if c == 0]
    assert len(zero) >= 80 and any(t[6] == _capi.DECODE_NO_ROOM for t in zero) and not any(t[0] for t in zero)
    assert len(model.gap_records(want[:ROUND])) > 100


def test_pieces_cover_every_residue_and_the_exact_sizes():
    batch, origins = lc.pieces_batch()
    want = lc.wanted("pieces")
    mono = [i for i, s in enumerate(batch.streams) if s.name.startswith("pieces mono")]
    assert len(mono) == 16
    lo, staged, at = set(), set(), 0
    for i, (slot, t, gaps) in enumerate(want):
        s = batch.streams[i]
        W = s.channels * s.width
        assert len(gaps) == 1 and t[0] == 3 and t[6] == 0
        a, n = gaps[0]
        if i in mono:
            assert W == 1 and n * W == 5 * PIECE // 2
            lo.add((batch.out_offsets[i] + a * W) % 16)        # device memory: the caller's slots
            staged.add((at + a * W) % 16)                       # host memory: the defined prefixes packed
            edges = {(batch.out_offsets[i] + a * W + q * PIECE) % 16 for q in range(3)}
            assert len(edges) == 1
        at += len(slot)
    assert lo == set(range(16)) and staged == set(range(16))
    exact = [want[i][2][0][1] for i, s in enumerate(batch.streams) if s.name.startswith("pieces exact")]
    assert tuple(exact) == (PIECE - 1, PIECE, PIECE + 1, 2 * PIECE)
    wide = [(want[i][2][0][1] * 9, batch.out_offsets[i]) for i, s in enumerate(batch.streams) if s.channels == 3]
    assert len(wide) == 6 and all(s.width == 3 for s in batch.streams if s.channels == 3)
    assert all(2 * PIECE < n < 3 * PIECE and n % 9 == 0 and PIECE % 9 for n, _ in wide)
    assert len({(off + 16 * 9 + q * PIECE) % 16 for n, off in wide for q in range(3)}) >= 6
    for i in range(len(batch.streams) - 1):
        assert batch.out_offsets[i + 1] == batch.out_offsets[i] + batch.capacities[i] + 1


def test_wide_spans_decode_workgroups_with_idle_frames_between_live_ones():
    batch, origins = lc.wide_batch()
    want = lc.wanted("wide")
    for (_, t, gaps), s, least in zip(want, batch.streams, (200, 70)):
        assert chain_frames(t) >= least and t[3] >= least // 6 and len(gaps) >= least // 8 and t[6] == 0
        per = WG // s.channels
        assert chain_frames(t) > 2 * per        # three decode workgroups or more
    assert [s.channels for s in batch.streams] == [3, 8]


def test_the_undamaged_batch_passes_the_seams_of_the_plain_index():
    import streams_model
    batch = lc.undamaged_batch()
    want = streams_model.expected_batch(batch)
    assert len(batch.streams) >= 1100 + 2
    assert want[0][1] == [1100, 1100 * lc.BLOCK, len(batch.streams[0].data), 0] and want[-1][1] == want[0][1]
    assert all(t[3] == 0 for _, t in want)
    frames = [t[0] for _, t in want]
    assert sum(frames[:ROUND]) > ROUND and sum(frames[ROUND:]) > ROUND      # frames either side of stream 1024 ...
    assert sum(1 for f in frames[ROUND:] if f) > 100                         # ... in many streams
    # recovery's model gives the same bytes
    for (pcm, t), s, cap in zip(want[:40], batch.streams, batch.capacities):
        slot, rt, gaps = model.expected(s.data, s.channels, s.bps, s.mbs, s.width, cap)
        assert np.array_equal(slot, pcm) and rt == [t[0], t[1], 0, 0, 0, 0, 0, 0] and gaps == []


# ---------------------------------------------------------------- the cases discriminate
def test_a_maximum_lost_at_a_workgroup_edge_changes_seams():
    want = lc.wanted("seams")
    honest = placement("seams")
    assert honest == [(t[0], t[3]) for _, t, _ in want]          # the loop above is the model's rule
    broken = placement("seams", reset=WG)
    assert broken != honest
    names = lc.seams_batch()[2]
    changed = {n for n, a, b in zip(names, honest, broken) if a != b}
    assert {"spike", "restart"} <= changed                        # a dropped run across a workgroup edge
    assert "undamaged" not in changed and "gap" not in changed    # ascending numbers never ask the maximum
    # 262 144 lies beyond every batch: there the seam is held by the scan's own test
    assert placement("seams", reset=sc.ROUND) == honest


def test_a_maximum_lost_at_element_262144_changes_the_scan_cases():
    def broken(values, heads):
        out = sc.reference(values, heads).copy()
        for at in range(sc.ROUND, len(values), sc.ROUND):
            if heads[at]:
                continue
            nxt = np.flatnonzero(heads[at:])
            end = at + int(nxt[0]) if len(nxt) else len(values)
            end = min(end, at + sc.ROUND)
            out[at:end] = np.maximum.accumulate(values[at:end])
        return out

    caught, same = set(), set()
    for pattern, n in sc.all_cases():
        if "descending" not in pattern and not pattern.startswith(("a head", "one segment")):
            continue
        values, heads = sc.case(pattern, n)
        (caught if not np.array_equal(broken(values, heads), sc.reference(values, heads)) else same).add((pattern, n))
    assert all(n <= sc.ROUND or p == "a head at 262144" for p, n in same), same
    for n in (sc.ROUND + 1, 2 * sc.ROUND + 300):
        for p in ("one segment, element 0 its maximum", "sparse heads, descending", "heads at 256k + 1, descending",
                  "heads at 256k - 1, descending", "a head at 262143"):
            assert (p, n) in caught, (p, n)
    assert ("a head at 262145", 2 * sc.ROUND + 300) in caught
    assert set(sc.SIZES) >= {1, 255, 256, 257, sc.ROUND - 1, sc.ROUND, sc.ROUND + 1, 2 * sc.ROUND + 300}


def test_a_sum_that_restarts_at_1024_changes_seams_and_many():
    want = lc.wanted("seams")
    assert written_by_scan("seams") == [t[0] for _, t, _ in want]
    broken = written_by_scan("seams", restart=ROUND)
    assert broken != [t[0] for _, t, _ in want]
    # per stream: the gap records of `many` and where the truncated tables end
    want = lc.wanted("many")
    records = model.gap_records(want)
    honest = records_by_scan(want)
    assert [honest[k] for k in range(len(records))] == records
    broken = records_by_scan(want, restart=ROUND)
    total = len(records)
    low = len(model.gap_records(want[:ROUND])) - 7
    for max_gaps in lc.many_max_gaps():
        assert [broken.get(k) for k in range(min(max_gaps, total))] != records[:max_gaps]
    assert lc.many_max_gaps() == (total, total - 1, low) and 0 < low < len(model.gap_records(want[:ROUND]))


def test_a_chain_walk_without_level_6_changes_seams():
    honest = placement("seams")
    broken = placement("seams", keep=64)
    names = lc.seams_batch()[2]
    changed = {n for n, a, b in zip(names, honest, broken) if a != b}
    assert changed == {n for n, a in zip(names, honest) if sum(a) > 64} and len(changed) >= 8
    import streams_model
    batch = lc.undamaged_batch()
    assert streams_model.expected_batch(batch)[0][1][0] > 1 << 10


def test_the_hook_is_declared_bound_and_kept_out_of_the_product():
    name = "flacenc_hip_debug_segmax_scan"
    header = open(os.path.join(ROOT, "flacenc_rs_amd", "csrc", "flacenc_hip_debug.h")).read()
    assert re.search(r"\bint %s\s*\(" % name, header) and name in _capi.DEBUG_SYMBOLS
    assert name not in _capi.EXPORTED_SYMBOLS
    assert name not in open(os.path.join(ROOT, "include", "flacenc_hip.h")).read()
    lib = _capi.load()
    assert not hasattr(lib, name) and hasattr(_capi.load_hooks(), name)
