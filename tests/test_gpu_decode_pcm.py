"""flacenc_hip_decode_pcm on the GPU: streams of the project's own encoders (flacenc_hip_encode_pcm at 8 / 16 / 24 bits and
1 / 2 / 3 / 8 channels, wasted bits, flacenc_hip_encode_variable, a run of digital silence) come back as exactly the PCM
bytes that went in, and as what flacenc_hip_index_frames_async + flacenc_hip_decode_frames + the numpy model of
flacenc_hip_pack_le_bytes give -- under the call's own plan and under hook plans that put window edges and group seams
after a handful of frames, with pinned and pageable buffers on either side.  Then the stops: a corrupted frame, a cut
stream, leading garbage, an output that ends inside a frame (and the second call that continues), a frame with a status,
the wrong bit depth.  Everything compared is bytes and integers: every comparison is exact."""
import functools

import numpy as np
import pytest

import pcm_pack_model as model
import stream_seam_cases as seams
from flacenc_rs_amd import _capi

pytestmark = pytest.mark.gpu
RATE, FILL, TAIL = 44100, 0xEE, 96


class Stream:
    def __init__(self, name, data, pcm, channels, bps, mbs):
        self.name, self.data, self.pcm, self.channels, self.bps, self.mbs = name, data, pcm, channels, bps, mbs
        self.width = (bps + 7) // 8


def fixed_stream(h, name, channels, bps, n, full, tail, flags=0, content_shift=0, silence=False):
    """`full` blocks of n samples + a last block of `tail` through flacenc_hip_encode_pcm."""
    width = (bps + 7) // 8
    x = seams.material(full + 1, channels, n, bps - content_shift, seed=len(name) + n)
    if silence:
        x[:] = 0
    x = x << content_shift   # (wasted bits: narrow content in a wide container)
    pcm = seams.pack_pcm(x[:full], x[full][:, :tail] if tail else None, width)
    cfg = _capi.make_frame_config(_capi.make_config(lpc_order=8, flags=flags), use_fixed=True)
    out, lens = h.encode_pcm(pcm, channels, cfg, width, bps, n, RATE)
    assert len(lens) == full + (1 if tail else 0)
    return Stream(name, np.array(out, copy=True), pcm, channels, bps, n)


def variable_stream(h):
    import stream_cases
    S, levels, bps, n_sb = 4096, 3, 16, 5
    total = n_sb * S - 777
    x = stream_cases.changing(n_sb, 2, S, bps, 1)
    x[-1, :, total % S:] = 0
    v = h.encode_variable(x, bps, stream_cases.frame_cfg(8), levels, total_samples=total, sample_rate=RATE)
    assert not v["overflow"] and len(set(v["block_sizes"].tolist())) > 1
    flat = x.transpose(1, 0, 2).reshape(2, -1)[:, :total]
    pcm = seams.pack_pcm(flat[None], None, 2)
    return Stream("variable levels 3", np.frombuffer(v["data"], np.uint8).copy(), pcm, 2, bps, S)


@pytest.fixture(scope="module")
def streams(hooks_handle):
    h = hooks_handle
    made = [fixed_stream(h, "16-bit stereo 4096", 2, 16, 4096, 12, 1000),
            fixed_stream(h, "8-bit mono 256", 1, 8, 256, 40, 17),          # a last block under 64 samples
            fixed_stream(h, "24-bit 3 channels 1152", 3, 24, 1152, 20, 500),
            fixed_stream(h, "16-bit 8 channels 256", 8, 16, 256, 24, 100),
            fixed_stream(h, "wasted bits 16 in 24", 2, 24, 1152, 14, 300, flags=_capi.FLAG_WASTED_BITS, content_shift=8),
            variable_stream(h),
            fixed_stream(h, "silence 300 frames", 2, 16, 256, 300, 33, silence=True)]
    return {s.name: s for s in made}


NAMES = ["16-bit stereo 4096", "8-bit mono 256", "24-bit 3 channels 1152", "16-bit 8 channels 256", "wasted bits 16 in 24",
         "variable levels 3", "silence 300 frames"]


@functools.lru_cache(None)
def frame_bound(channels, mbs, bps):
    """B of the call's window rule (include/flacenc_hip.h, csrc/flacenc_hip_debug.h)."""
    lib = _capi.load()
    b = int(lib.flacenc_hip_frame_bytes_bound(channels, mbs, bps))
    return max(b, int(lib.flacenc_hip_stereo_frame_bytes_bound(mbs, bps))) if channels == 2 else b


def indexed(h, s):
    off, ln, ok = h.index_frames(s.data, s.channels, s.bps, len(s.data) // 9 + 1)
    assert ok
    return off.astype(np.int64), ln.astype(np.int64)


def decode(h, s, data=None, in_kind="pageable", out_kind="pageable", capacity=None, bps=None, width=None, mbs=None):
    """One call into buffers of the given kinds; `out` is its capacity + TAIL bytes of FILL.  -> (bytes, totals); what
    lies behind the bytes returned, the tail included, must still be FILL."""
    data = s.data if data is None else data
    width = width or s.width
    src = seams.buffer_of(in_kind, len(data))
    src[:] = data
    cap = len(s.pcm) if capacity is None else capacity
    out = seams.buffer_of(out_kind, cap + TAIL)
    out[:] = FILL
    got, totals = h.decode_pcm(src, s.channels, bps or s.bps, mbs or s.mbs, bytes_per_sample=width, out=out,
                               out_capacity=cap)
    assert len(got) == totals[1] * s.channels * width
    assert (out[len(got):] == FILL).all(), "bytes behind totals[1] samples were written"
    return np.array(got, copy=True), totals


@pytest.mark.parametrize("name", NAMES)
def test_streams_come_back_as_the_pcm_that_went_in(hooks_handle, streams, name):
    h, s = hooks_handle, streams[name]
    off, ln = indexed(h, s)
    frames, samples = len(off), len(s.pcm) // (s.channels * s.width)
    want_totals = [frames, samples, len(s.data), 0]
    # the pieces the call is made of, on the whole stream at once: index + decode_frames + the model of the packer
    rows, bs, _, st = h.decode_frames(s.data, off, ln, s.channels, s.bps, s.mbs)
    assert not st.any()
    pieces, _, total = model.pack_le_bytes(rows, bs, s.width)
    assert total == samples and np.array_equal(pieces, s.pcm)
    # the call's own plan
    h.debug_set_decode_plan(0, 0)
    for kinds in (("pageable", "pageable"), ("pinned", "pinned+3")):
        got, totals = decode(h, s, in_kind=kinds[0], out_kind=kinds[1])
        assert totals == want_totals and np.array_equal(got, s.pcm), kinds
        window, n_windows, group, n_groups = h.debug_last_decode_plan()
        assert window == max(128 << 20, 2 * frame_bound(s.channels, s.mbs, s.bps)) and n_windows == 1 and n_groups >= 1
    # hook plans: windows of 2B, groups of 1, 2 and 3 frames (both slots reused twice and more)
    B = frame_bound(s.channels, s.mbs, s.bps)
    W = 2 * B
    edges = [k * (W - B) + W for k in range(len(s.data) // (W - B) + 1) if k * (W - B) + W < len(s.data)]
    assert any(o < e < o + n for e in edges for o, n in zip(off, ln)), "no frame straddles a window edge"
    try:
        for group, kinds in ((1, ("pageable", "pageable")), (2, ("pinned", "pageable")), (2, ("pageable", "pinned")),
                             (3, ("pinned+3", "pinned"))):
            h.debug_set_decode_plan(1, group)   # (below 2B: raised to 2B)
            got, totals = decode(h, s, in_kind=kinds[0], out_kind=kinds[1])
            assert totals == want_totals and np.array_equal(got, s.pcm), (group, kinds)
            window, n_windows, g, n_groups = h.debug_last_decode_plan()
            assert window == W and g == group and n_windows > 1 and n_groups > 2
            assert n_groups >= -(-frames // group)
    finally:
        h.debug_set_decode_plan(0, 0)


def test_a_wider_container_on_request(hooks_handle, streams):
    """bytes_per_sample above ceil(bits / 8): the same samples, sign-extended to the width asked for."""
    h, s = hooks_handle, streams["16-bit stereo 4096"]
    got, totals = decode(h, s, capacity=len(s.pcm) // 2 * 3, width=3)
    v = s.pcm.view("<i2").astype("<i4")
    want = np.ascontiguousarray(v.view(np.uint8).reshape(-1, 4)[:, :3]).reshape(-1)
    assert totals[3] == 0 and np.array_equal(got, want)


PLANS = [(0, 0), (1, 3)]


@pytest.mark.parametrize("plan", PLANS)
@pytest.mark.parametrize("k", [1, 7])
def test_a_corrupted_frame_stops_the_chain(hooks_handle, streams, plan, k):
    h, s = hooks_handle, streams["16-bit stereo 4096"]
    off, ln = indexed(h, s)
    bad = s.data.copy()
    bad[off[k] + ln[k] // 2] ^= 0x10
    try:
        h.debug_set_decode_plan(*plan)
        got, totals = decode(h, s, data=bad)
    finally:
        h.debug_set_decode_plan(0, 0)
    assert totals == [k, k * 4096, int(off[k]), _capi.DECODE_CHAIN]
    assert np.array_equal(got, s.pcm[:len(got)])


@pytest.mark.parametrize("plan", PLANS)
def test_a_cut_stream_and_leading_garbage(hooks_handle, streams, plan):
    h, s = hooks_handle, streams["24-bit 3 channels 1152"]
    off, ln = indexed(h, s)
    last = len(off) - 1
    try:
        h.debug_set_decode_plan(*plan)
        got, totals = decode(h, s, data=s.data[:off[last] + ln[last] // 2])
        assert totals == [last, last * 1152, int(off[last]), _capi.DECODE_CHAIN]
        assert np.array_equal(got, s.pcm[:len(got)])
        garbage = np.random.default_rng(5).integers(0, 256, 700).astype(np.uint8)
        got, totals = decode(h, s, data=np.concatenate([garbage, s.data]))
        assert totals == [0, 0, 0, _capi.DECODE_CHAIN] and got.size == 0
    finally:
        h.debug_set_decode_plan(0, 0)


@pytest.mark.parametrize("plan", PLANS)
@pytest.mark.parametrize("k", [2, 8])
def test_no_room_stops_before_the_frame_and_a_second_call_continues(hooks_handle, streams, plan, k):
    h, s = hooks_handle, streams["16-bit stereo 4096"]
    off, _ = indexed(h, s)
    frame_bytes = 4096 * 2 * 2
    try:
        h.debug_set_decode_plan(*plan)
        first, totals = decode(h, s, capacity=k * frame_bytes + frame_bytes // 2)   # ends inside frame k
        assert totals == [k, k * 4096, int(off[k]), _capi.DECODE_NO_ROOM]
        rest, totals2 = decode(h, s, data=s.data[totals[2]:], capacity=len(s.pcm) - len(first))
        assert totals2 == [len(off) - k, len(s.pcm) // 4 - k * 4096, len(s.data) - totals[2], 0]
        assert np.array_equal(np.concatenate([first, rest]), s.pcm)
        # no room at all: nothing written, the call still says where it stands
        none, totals3 = decode(h, s, capacity=0)
        assert totals3 == [0, 0, 0, _capi.DECODE_NO_ROOM] and none.size == 0
    finally:
        h.debug_set_decode_plan(0, 0)


def test_a_frame_with_a_status_and_the_wrong_bit_depth_stop_at_frame_0(hooks_handle, streams):
    h, s = hooks_handle, streams["16-bit stereo 4096"]
    # blocks of 4096 under a max_block_size of 2048: the frames chain, the decoder calls the first UNSUPPORTED
    got, totals = decode(h, s, mbs=2048)
    assert totals == [0, 0, 0, _capi.DECODE_UNSUPPORTED] and got.size == 0
    # 24 bits asked of a 16-bit stream: no header is this stream's, nothing chains
    got, totals = decode(h, s, bps=24, width=3, capacity=len(s.pcm) // 2 * 3)
    assert totals[:3] == [0, 0, 0] and totals[3] != 0 and got.size == 0


def test_arguments(hooks_handle, streams):
    h, s = hooks_handle, streams["8-bit mono 256"]
    got, totals = h.decode_pcm(b"", 1, 8, 256)
    assert totals == [0, 0, 0, 0] and got.size == 0
    out = np.full(64, FILL, np.uint8)
    for kw in (dict(channels=0), dict(channels=9), dict(bytes_per_sample=5), dict(max_block_size=0),
               dict(max_block_size=65537)):
        a = dict(channels=1, bits_per_sample=8, max_block_size=256, bytes_per_sample=1)
        a.update(kw)
        with pytest.raises(_capi.FlacencHipError) as e:
            h.decode_pcm(s.data, a["channels"], a["bits_per_sample"], a["max_block_size"],
                         bytes_per_sample=a["bytes_per_sample"], out=out)
        assert e.value.code == _capi.ERR_BAD_ARGUMENT, kw
    with pytest.raises(_capi.FlacencHipError) as e:   # 16 bits do not fit one byte
        h.decode_pcm(s.data, 1, 16, 256, bytes_per_sample=1, out=out)
    assert e.value.code == _capi.ERR_BAD_ARGUMENT
    for bps in (3, 25, 32):
        with pytest.raises(_capi.FlacencHipError) as e:
            h.decode_pcm(s.data, 1, bps, 256, bytes_per_sample=4, out=out)
        assert e.value.code == _capi.ERR_UNSUPPORTED
    assert (out == FILL).all()
