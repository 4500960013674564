"""The two span policies of the frame index (stream_index.cpp) agree: on the same bytes, flacenc_hip_index_frames (one span
[0, n_bytes) with fixed parameters) returns the chain that flacenc_hip_decode_streams accepts for a table of one stream
that covers the whole buffer -- the frame count of totals[0], the same `consumed` end, offsets and lengths that tile
[0, consumed), and the same verdict on the chain.  Every comparison is exact."""
import numpy as np
import pytest

import decode_cases as dc
import streams_cases as cases
from flacenc_rs_amd import _capi

pytestmark = pytest.mark.gpu

ROOM = 1 << 21  # the slot: more than any of these streams decodes to, so that the cut never stops a chain


@pytest.fixture(scope="module")
def h():
    with _capi.Handle(0) as handle:
        yield handle


def tiny():
    _, data, offsets, _, channels, bps = dc.tiny_stream()
    return np.frombuffer(data, np.uint8), channels, bps, 576, offsets, True


def written(*a, **kw):
    s = cases.written_stream(*a, **kw)
    return s.data, s.channels, s.bps, s.mbs, cases.offsets_of(s)[:-1], True


def cut():
    s, left, why = cases.stops()[0]["cut in last frame"]
    assert why == _capi.DECODE_CHAIN
    return s.data, s.channels, s.bps, s.mbs, cases.offsets_of(s)[:left], False


CASES = {
    "mono 16, 3 frames of 16": lambda: written("mono 3x16", 41, 1, 16, [16, 16, 16]),
    "stereo with mid/side": lambda: written("mid/side", 42, 2, 16, [64, 48, 16], tags=(1, 10, 8)),
    "tiny frames": tiny,          # one lane's 16 candidate positions hold two frame starts
    "last frame cut short": cut,  # a chain error on both sides, with the same verified prefix
}


@pytest.mark.parametrize("name", list(CASES))
def test_one_span_equals_a_table_of_one_stream(h, name):
    data, channels, bps, mbs, starts, whole = CASES[name]()
    max_frames = len(data) // 9 + 1
    offsets, lengths, ok = h.index_frames(data, channels, bps, max_frames)
    table = np.zeros(1, _capi.STREAM_DESC_DTYPE)
    table[0] = (0, len(data), 0, ROOM, channels, bps, mbs, (bps + 7) // 8)
    totals, call, _ = h.decode_streams(data, table, max_frames, np.zeros(ROOM, np.uint8))
    frames, _, consumed, why = (int(v) for v in totals[0])
    assert call[0] == frames  # no INDEX_ERROR
    # the chain the corpus was written with
    assert np.array_equal(offsets, np.asarray(starts, np.uint64))
    # one chain on both sides
    assert len(offsets) == frames and frames > 0
    assert int(offsets[-1]) + int(lengths[-1]) == consumed
    assert offsets[0] == 0 and np.array_equal(offsets[1:], (offsets + lengths)[:-1])
    # and one verdict on it
    assert ok == whole and why == (0 if whole else _capi.DECODE_CHAIN)
    assert (consumed == len(data)) == whole
