"""The checker of the stream-seam suite (tests/stream_seam_cases.py) on the CPU: its statement of the chunk rule, its seam
frames, its packing of every container width against the oracle's le_bytes_to_i32s, and its CPU models' frames through the
test-side parser -- so that a GPU failure there points at the library and not at the checker."""
import numpy as np
import pytest

import stream_seam_cases as sc
from flacenc_rs_amd import _capi
from oracle import oracle as orc


def test_plan_of_restates_the_rule():
    assert sc.plan_of(0, 0, 0, 16384) == (0, 0)
    assert sc.plan_of(0, 0, 5, 16384) == (1, 1) and sc.plan_of(3, 0, 5, 16384) == (1, 1)
    assert sc.plan_of(0, 16684, 0, 4096 * 2 * 2) == (3072, 6)            # 48 MiB / frame bytes
    assert sc.plan_of(0, 4 * 8192 + 100, 17, 64) == (8192, 6)            # the clamp's upper end
    assert sc.plan_of(0, 2000, 1, 8 * 32767 * 4) == (768, 4)             # and its lower end
    assert sc.plan_of(0, 9, 0, 16384) == (9, 1)                          # never more than the call has
    assert sc.plan_of(2, 11, 1000, 16384) == (2, 7) and sc.plan_of(3, 2, 0, 16384) == (2, 1)


def test_seam_frames():
    assert sc.seam_frames(0, 1, False) == [] and sc.seam_frames(0, 1, True) == [0]
    assert sc.seam_frames(1, 1, False) == [0] and sc.seam_frames(7, 3, False) == [0, 2, 3, 5, 6]
    assert sc.seam_frames(16, 3, True) == [0, 2, 3, 5, 6, 8, 9, 11, 12, 14, 15, 16]
    assert sc.seam_frames(2 * 8192 + 5, 8192, False) == [0, 8191, 8192, 16383, 16384, 16388]


@pytest.mark.parametrize("bytes_ps,bps", [(1, 8), (2, 12), (2, 16), (3, 20), (3, 24), (4, 24)])
def test_pack_pcm_against_the_oracle(bytes_ps, bps):
    x = sc.material(5, 3, 100, bps, seed=bps)
    assert x.min() == -(1 << (bps - 1)) and x.max() == (1 << (bps - 1)) - 1      # full scale, both ends
    tail = x[4][:, :37]
    p = sc.pack_pcm(x[:4], tail, bytes_ps)
    assert p.dtype == np.uint8 and p.size == (400 + 37) * 3 * bytes_ps
    ints = orc.le_bytes_to_i32s(p.tobytes(), bytes_ps)
    assert np.array_equal(ints[:1200].reshape(4, 100, 3).transpose(0, 2, 1), x[:4])
    assert np.array_equal(ints[1200:].reshape(37, 3).T, tail)


@pytest.mark.parametrize("C,n,bps,flags", [(2, 1152, 16, 0), (1, 65, 8, 0), (3, 65, 20, 0), (8, 256, 24, 0),
                                           (2, 576, 24, _capi.FLAG_REFERENCE_SUM_ORDER),
                                           (2, 576, 24, _capi.FLAG_WASTED_BITS), (3, 576, 24, _capi.FLAG_WASTED_BITS),
                                           (2, 576, 24, _capi.FLAG_ORDER_SEARCH), (2, 576, 24, _capi.FLAG_WINDOW_SEARCH),
                                           (3, 576, 16, _capi.FLAG_ORDER_GUESS), (2, 576, 24, _capi.FLAG_GENERIC_KERNEL),
                                           (2, 576, 24, _capi.FLAG_WASTED_BITS | _capi.FLAG_ORDER_GUESS |
                                            _capi.FLAG_WINDOW_SEARCH)])
def test_model_frames_parse_back_to_their_input(C, n, bps, flags):
    cfg, model = sc.configs(8, use_fixed=True, flags=flags)
    assert cfg.qlpc.flags == flags and model is not None
    x = sc.material(5, C, n, bps, seed=n + C)
    if flags & _capi.FLAG_WASTED_BITS:
        x[1:3] &= ~0xFF
    kinds = set()
    for f, number in enumerate((0, 127, 128, (1 << 26) - 1, 1 << 31)):
        fr = model.frame(x[f], bps, sc.RATE, number)
        got = sc._parsed(fr, bps, sc.RATE, bool(flags & _capi.FLAG_WASTED_BITS))
        assert got[0] == number and got[1] == n and np.array_equal(got[2], x[f])
        kinds.add(len(fr))
    assert len(kinds) > 1
