"""tests/scale_cases.py without a device: every case reaches the seams it names, fits the memory rule, its placement has
the properties the GPU file relies on, and the checkers find what they are there to find."""
import numpy as np
import pytest

import scale_cases as sc

CASES = sc.cases()
IDS = [c.name for c in CASES]


def test_case_names_are_unique_and_counts_odd_or_explained():
    assert len(set(IDS)) == len(IDS)
    for c in CASES:
        if c.extra.get("stereo"):
            assert c.n % 4 == 0  # whole stereo frames of four candidate rows
        else:
            assert c.n % 2 == 1, c.name  # a partial last workgroup wherever a workgroup takes several units


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_case_reaches_every_seam_it_names(case):
    assert case.seams
    bufs = {b.name: b for b in sc.buffers(case)}
    for (name, seam), (row, inside) in sc.seam_rows(case).items():
        b, s = bufs[name], sc.SEAMS[seam]
        start = row * b.stride_bytes
        assert row < b.rows and start + b.row_bytes <= b.nbytes
        if inside:  # one row has the seam strictly inside it, and a whole row lies beyond
            assert start < s < start + b.row_bytes and row + 1 < b.rows
        else:  # rows of a size that divides the seam: one ends at it, the next starts there
            assert start == s and s % b.stride_bytes == 0 and row >= 1
        assert b.nbytes > s


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_need_bytes_is_within_the_memory_rule(case):
    need = sc.need_bytes(case)
    assert need <= sc.MEMORY_RULE, (case.name, need / 2**30)
    # and it is no less than what the caller's buffers alone take
    assert need >= sum(b.nbytes for b in sc.buffers(case) if b.kind == "caller")


def test_the_window_and_order_search_case_runs_at_least_three_slices():
    assert sc.search_slices(sc.case("ORDER_SEARCH|WINDOW_SEARCH 4096/16/12")) >= 3


def test_the_wasted_bits_case_lists_tens_of_thousands_of_frames_within_its_bound():
    import wasted_model as wm
    case = sc.case("WASTED_BITS 4096/24/8")
    x = sc.base_frames(2, case.block, case.bps).astype(np.int64)
    fc = wm.frame_config(order=case.order)
    marked = [f for f in range(sc.K)
              if any(wm.wasted_of(v, fc) for v in (x[f, 0], x[f, 1], (x[f, 0] + x[f, 1]) >> 1, x[f, 0] - x[f, 1]))]
    m = int(np.isin(sc.case_idx(case), marked).sum())
    assert 20000 <= m <= case.extra["wasted_frames"]  # (the marked-list tests of the other suites stop at 1 300)


def test_ensure_growth_is_restated():
    assert sc.grown(0) == 0 and sc.grown(1000) == 1000 + 250 + 256


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_placement_properties(case):
    idx = sc.case_idx(case)
    n = case.n
    assert idx.shape == (n,) and idx.min() >= 0 and idx.max() < sc.K
    ends = set(idx[:16].tolist()) | set(idx[n - 16:].tolist())
    assert ends == set(range(sc.K))
    assert set(idx[0::2].tolist()) == set(range(sc.K)) and set(idx[1::2].tolist()) == set(range(sc.K))
    assert np.array_equal(idx, sc.case_idx(case))  # seeded
    # the frame at every seam of a per-frame buffer is one the certificate recomputes or marks, or one with wasted bits
    bufs = {b.name: b for b in sc.buffers(case)}
    special = set(sc.special_frames(case.bps))
    seen = 0
    for (name, _), (row, _) in sc.seam_rows(case).items():
        b = bufs[name]
        if b.rows != n * b.rows_per_frame:
            continue
        assert int(idx[row // b.rows_per_frame]) in special, (case.name, name)
        seen += 1
    assert seen or case.route in ("decode", "wasted")


def test_base_frames_hold_what_they_promise():
    x = sc.base_frames(2, 4096, 16)
    assert x.shape == (sc.K, 2, 4096) and x.dtype == np.int32
    assert not x[24].any() and (x[25] == x[25, 0, 0]).all() and x[25].any()
    assert len({x[i].tobytes() for i in range(sc.K)}) == sc.K  # distinct frames
    assert np.array_equal(x, sc.base_frames(2, 4096, 16))
    assert (x[22, 0, :100] == 32767).all() and (x[22, 1, :100] == -32768).all()  # the clipped plateau
    y = sc.base_frames(2, 4096, 24)
    assert (y[28] & 63 == 0).all() and y[28].any() and (y[29, 1] & 511 == 0).all()  # wasted bits
    assert len({y[i].tobytes() for i in range(sc.K)}) == sc.K
    z = sc.base_frames(3, 1152, 16)
    assert z.shape == (sc.K, 3, 1152) and len({z[i].tobytes() for i in range(sc.K)}) == sc.K


@pytest.mark.parametrize("seam", list(sc.SEAMS))
@pytest.mark.parametrize("row_bytes", [4 * 4096, 4 * 1152, 16928])
def test_sparse_stride_puts_the_seam_inside_one_row(seam, row_bytes):
    s = sc.SEAMS[seam]
    row = 33
    stride = sc.sparse_stride(s, row_bytes, row)
    assert stride % 16 == 0 and row * stride < s < row * stride + row_bytes
    assert (row - 1) * stride + row_bytes < s < (row + 1) * stride  # the rest lies on both sides
    total = sc.LEAD + 2 * sc.K * stride + sc.GUARD
    assert total <= sc.MEMORY_RULE


def test_aliases_and_canary_regions():
    # a write 100 bytes past 2^32 cut to 32 bits lands at 100; cut to a signed 32-bit offset past 2^31 it lands below 0
    assert (100, 116) in sc.aliases(sc.S32 + 100, 16)
    assert (-(1 << 31) + 8, -(1 << 31) + 24) in sc.aliases(sc.S31 + 8, 16)
    # element indices cut to 32 bits: 2^34 bytes + 40 lands at 40
    assert (40, 56) in sc.aliases(sc.E32 + 40, 16)
    assert sc.aliases(64, 16) == []
    stride = sc.sparse_stride(sc.S32, 16384, 33)
    regions = sc.canary_regions(64, 16384, stride)
    rows = [(r * stride, r * stride + 16384) for r in range(64)]
    for s, e in regions:
        assert s < e and s >= -sc.LEAD
        assert all(e <= rs or s >= re for rs, re in rows)  # never inside a row
    assert (16384, 16384 + sc.GUARD) in regions and (-sc.GUARD, 0) in regions
    # the straddling row's alias: its bytes beyond 2^32 cut to 32 bits lie at the buffer's start, row 0 cut out of them
    assert sc.subtract([(0, 10)], [(2, 4)]) == [(0, 2), (4, 10)]


def test_straddling_offsets():
    lens = np.full(sc.K, 9000)
    off = sc.straddling_offsets(lens, 16928)
    at = sc.K // 2
    assert off[at] < sc.S32 < off[at] + 9000 and (off[:at] + 16928 <= off[at]).all() and (off[at + 1:] > sc.S32).all()
    assert (np.diff(off) >= 9000).all()
    spans = [(int(o), int(o) + 9000) for o in off]
    regions = sc.canary_regions_for(spans)
    assert all(e <= a or s >= b for s, e in regions for a, b in spans)
    # the straddling frame's bytes beyond the seam, cut to 32 bits, would land in front of frame 0's guard or in it
    assert any(s < 9000 and e > 0 for s, e in sc.aliases(spans[at][0], 9000))


def test_check_tiled_finds_a_swapped_frame_and_a_stale_record():
    rng = np.random.default_rng(1)
    base = rng.integers(0, 256, (sc.K, 752), dtype=np.uint8)
    idx = sc.placement(1000, sc.K, 5)
    got = base[idx].copy()
    assert sc.check_tiled(got, base, idx) is None
    swapped = got.copy()
    a, b = 500, 501
    assert idx[a] != idx[b]
    swapped[[a, b]] = swapped[[b, a]]
    f, byte = sc.check_tiled(swapped, base, idx)
    assert f == a and swapped[a, byte] != base[idx[a], byte]
    stale = got.copy()
    stale[777] = 0  # a record the launch never wrote
    assert sc.check_tiled(stale, base, idx)[0] == 777
    one = got.copy()
    one[999, 751] ^= 1  # the last byte of the last frame
    assert sc.check_tiled(one, base, idx) == (999, 751)


def test_check_canaries_finds_a_hit():
    lead = 64
    regions = [(-16, 0), (32, 48)]
    buf = np.full(lead + 64, sc.SENTINEL, np.uint8)
    buf[lead:lead + 32] = 7  # the row itself
    assert sc.check_canaries(buf, regions, lead) is None
    buf[lead + 40] = 0
    assert sc.check_canaries(buf, regions, lead) == (1, 40)
    buf[lead - 3] = 1
    assert sc.check_canaries(buf, regions, lead) == (0, -3)
