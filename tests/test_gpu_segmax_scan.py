"""The segmented max-scan of flacenc_hip_recover_streams on its own, through flacenc_hip_debug_segmax_scan: the call's
three launches on the cases of tests/segmax_cases.py, against a plain numpy loop over segments.  Sizes either side of
256 (a workgroup), of 1024 * 256 = 262 144 (the carry kernel's second round) and two rounds and a bit; the launches
sized by the elements and by 262 149 more, as the call sizes them by max_frames and not by the chain.  Every comparison
is exact."""
import numpy as np
import pytest

import segmax_cases as sc
from flacenc_rs_amd import _capi

pytestmark = pytest.mark.gpu
SPARE = sc.ROUND + 5


@pytest.mark.parametrize("pattern,n", sc.all_cases(), ids=lambda v: str(v))
def test_the_scan_equals_the_loop_over_segments(hooks_handle, pattern, n):
    values, heads = sc.case(pattern, n)
    want = sc.reference(values, heads)
    if "descending" in pattern or pattern.startswith("a head"):
        first = np.flatnonzero(heads)[np.cumsum(heads) - 1]
        assert np.array_equal(want, values[first])      # every output is its segment's first value
    for room in (n, n + SPARE):
        got = hooks_handle.debug_segmax_scan(values, heads, room)
        bad = np.flatnonzero(got != want)
        assert len(bad) == 0, (pattern, n, room, len(bad), int(bad[0]), int(got[bad[0]]), int(want[bad[0]]))


def test_no_element_and_the_contract(hooks_handle):
    h = hooks_handle
    for room in (1, 256, 257, SPARE):
        assert len(h.debug_segmax_scan(np.zeros(0, np.uint64), np.zeros(0, np.uint8), room)) == 0
    v, hd = sc.case("heads at 256k + 1", 300)
    want = sc.reference(v, hd)
    assert np.array_equal(h.debug_segmax_scan(v, hd), want)
    no_head = hd.copy()
    no_head[0] = 0
    for values, heads, room in ((v, no_head, 300), (v, hd, 299), (v, hd, (1 << 30) + 1)):
        rc, out = h.debug_segmax_scan(values, heads, room, check=False)
        assert rc == _capi.ERR_BAD_ARGUMENT and not out.any()
    assert np.array_equal(h.debug_segmax_scan(v, hd, 300), want)   # the handle is as good as before
