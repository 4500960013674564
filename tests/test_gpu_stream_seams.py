"""flacenc_hip_encode_pcm / _stereo at its chunk seams (csrc/api_stream.cpp: two slots of staging, three streams, four
event pairs, a two-step way out, a short last block that is a chunk of its own on a slot a full chunk has just used).
The test hook flacenc_hip_debug_set_stream_chunk brings a chunk down to one, two or three frames, so that every frame of
every case is held to the one-call device path, the frames next to every seam to the CPU oracle, and the whole stream to
the decoder and the index -- tests/stream_seam_cases.py states the checker once.

What these tests catch for certain is the bookkeeping: a chunk's source offset, its frame number, where its lengths and
bytes land, which slot's pending record the way out reads, what the call writes outside its own extent.  A missing or
misplaced event wait is a race: one-frame chunks, seven chunks over two slots, pinned and pageable buffers both ways and
every frame compared make it likely to show, not certain.  No case is repeated to make one show.

Shapes are the smallest at which the pipeline can still go wrong: at most 40 frames under the hook, except
test_host_threads' second shape (3601 frames of 256 samples in chunks of 1536: the copy pool slices a staging copy only
from 1 MiB on); the two cases of the rule itself (no hook) are 2 MB and 17 MB of PCM."""
import numpy as np
import pytest

import stream_seam_cases as sc
from flacenc_rs_amd import _capi
from stream_seam_cases import check_stream

pytestmark = pytest.mark.gpu
F_ = _capi


@pytest.fixture(scope="module")
def ref():
    """The handle of the one-call references: the handle under test runs no encode launch but its own stream calls
    (the checker's index and verify calls, the way back, do run on it)."""
    h = _capi.Handle(0)
    yield h
    h.close()


@pytest.fixture(scope="module")
def stereo4096():
    """17 stereo frames of 4096 16-bit samples: the full frames of the geometry cases are its prefixes, the short last
    blocks come from its last frame -- so the oracle's frames and their parses are shared among the cases."""
    return sc.material(17, 2, 4096, 16, seed=1)


# ---------------------------------------------------------------------------------------------------- seam geometry
def geometry_cases():
    out = []
    for c in (1, 2, 3):
        for F in sorted({0, 1, c - 1, c, c + 1, 2 * c, 2 * c + 1, 3 * c + 2, 5 * c, 5 * c + 1}):
            for tail in (0, 1, 63, 1000):
                out.append((c, F, tail))
    return out


@pytest.mark.parametrize("c,F,tail", geometry_cases())
def test_seam_geometry(hooks_handle, ref, stereo4096, c, F, tail):
    """Stereo, 16-bit in 2 bytes, block 4096, order 8 with fixed predictors: 0 .. 5c + 1 full frames in chunks of c, with
    and without a short last block.  F = 0 without one is total_samples == 0 (nothing written, plan (0, 0)); F = 0 with
    one is the n_full == 0 plan; 5c + 1 with one is seven chunks: each slot reused at least twice, the short block on a
    reused slot.  The memory kinds of the two buffers go round with the case."""
    cfg, model = sc.configs(8, use_fixed=True)
    k = geometry_cases().index((c, F, tail))
    data, lens = check_stream(hooks_handle, stereo4096[:F], stereo4096[16][:, :tail] if tail else None, 2, 16, cfg,
                              in_kind=sc.KINDS[k % 3], out_kind=sc.KINDS[(k // 3) % 3], ref=ref, chunk=c, model=model)
    assert lens.size == F + (1 if tail else 0)
    if F == 0 and not tail:
        assert data == b"" and hooks_handle.debug_last_stream_plan() == (0, 0)
    if F == 5 * c + 1 and tail:
        assert hooks_handle.debug_last_stream_plan() == (c, 7)


# ---------------------------------------------------------------------------------------------------- formats x channels
FORMATS = [(1, 8), (2, 12), (2, 16), (3, 20), (3, 24), (4, 24)]
# every format at 2 and at 8 channels, every other channel count at one format (the full cross product's 48 cases spend
# their time in the test-side parser: 36 channel-frames of 1152 samples per format)
FORMAT_CASES = [(C, f) for C in (2, 8) for f in FORMATS] + list(zip((1, 3, 4, 5, 6, 7), FORMATS))


@pytest.mark.parametrize("C,fmt", FORMAT_CASES)
def test_sample_formats_and_channel_counts(hooks_handle, ref, C, fmt):
    """c = 2, five full frames of 1152 samples + a short block of 777: every container width (the sign extension of 1, 2,
    3 and 4 bytes, full-scale content in frames 1 and 3) and every channel count across two seams and a reused slot."""
    bytes_ps, bps = fmt
    x = sc.material(6, C, 1152, bps, seed=10 * C + bps)
    cfg, model = sc.configs(8, use_fixed=True)
    got = check_stream(hooks_handle, x[:5], x[5][:, :777], bytes_ps, bps, cfg, rate=48000, ref=ref, chunk=2, model=model)
    if C == 2 and fmt == (2, 16):   # flacenc_hip_encode_pcm(channels = 2) is flacenc_hip_encode_pcm_stereo
        other = check_stream(hooks_handle, x[:5], x[5][:, :777], bytes_ps, bps, cfg, rate=48000, ref=ref, chunk=2,
                             model=model, entry="channels")
        assert other[0] == got[0] and np.array_equal(other[1], got[1])


# ---------------------------------------------------------------------------------------------------- blocks, pipelines
# (block, channels, bytes per sample, bits, order, short last block): the short block takes another kernel pipeline
# than the full frames; 65 x 1 byte x mono, 65 x 3 bytes x 3 channels and 4097 x 3 bytes x mono put every chunk's
# source at an odd byte offset
BLOCK_CASES = [(64, 2, 2, 16, 8, 17), (65, 1, 1, 8, 8, 64), (65, 3, 3, 20, 8, 33), (100, 2, 3, 24, 8, 64),
               (1152, 2, 2, 16, 8, 63), (4096, 2, 2, 16, 8, 576), (4097, 1, 3, 24, 8, 4096), (4608, 2, 2, 16, 12, 1152),
               (8192, 2, 3, 24, 24, 4096), (32767, 1, 2, 16, 8, 4096)]


@pytest.mark.parametrize("n,C,bytes_ps,bps,order,tail", BLOCK_CASES)
def test_block_sizes_and_pipelines_across_a_seam(hooks_handle, ref, n, C, bytes_ps, bps, order, tail):
    x = sc.material(6, C, n, bps, seed=n % 1000 + C)
    cfg, model = sc.configs(order, use_fixed=True)
    check_stream(hooks_handle, x[:5], x[5][:, :tail], bytes_ps, bps, cfg, first=7, step=3, ref=ref, chunk=2, model=model)


# ---------------------------------------------------------------------------------------------------- flags
W, S, WS, G, R, GEN = (F_.FLAG_WASTED_BITS, F_.FLAG_ORDER_SEARCH, F_.FLAG_WINDOW_SEARCH, F_.FLAG_ORDER_GUESS,
                       F_.FLAG_REFERENCE_SUM_ORDER, F_.FLAG_GENERIC_KERNEL)


@pytest.fixture(scope="module")
def shifted24():
    """Six stereo frames of 4096 24-bit samples + a short block of 500: chunk 0 (frames 0, 1) has eight wasted bits in
    every frame, chunk 1 in none, chunk 2 in one channel of one frame, the short block in its second half only -- the
    pass a flag can skip is skipped in one chunk and not in the next."""
    x = sc.material(7, 2, 4096, 16, seed=24, full_scale=False) << 8
    x[2:] |= sc.material(5, 2, 4096, 8, seed=25, full_scale=False) & 0xFF
    x[2:, :, 5] |= 1
    x[4, 1] &= ~0xFF
    tail = np.ascontiguousarray(x[6][:, :500])
    tail[:, 250:] &= ~0xFF
    tail[:, 7] |= 1
    return np.ascontiguousarray(x[:6]), tail


@pytest.mark.parametrize("flags", [W, S, WS, G, R, GEN, W | G | WS],
                         ids=["WASTED_BITS", "ORDER_SEARCH", "WINDOW_SEARCH", "ORDER_GUESS", "REFERENCE_SUM_ORDER",
                              "GENERIC_KERNEL", "WASTED_BITS+ORDER_GUESS+WINDOW_SEARCH"])
def test_flags_across_a_seam(hooks_handle, ref, shifted24, flags):
    """c = 2, six frames + a short block, 24 bits in 3 bytes.  Every case's seam frames are stated on the CPU: the oracle
    under REFERENCE_SUM_ORDER and GENERIC_KERNEL (whose launch computes the unflagged integers), tests/wasted_model.py,
    order_model.py, window_model.py and guess_model.py under the flags they model, the guess model's wasted-bits frames
    with the default extra windows under the combination."""
    x, tail = shifted24
    cfg, model = sc.configs(8, use_fixed=True, flags=flags)
    assert model is not None
    check_stream(hooks_handle, x, tail, 3, 24, cfg, ref=ref, chunk=2, model=model)


# ---------------------------------------------------------------------------------------------------- frame numbers
@pytest.mark.parametrize("first,step", [(125, 1), (2045, 1), (65533, 1), ((1 << 21) - 3, 1), ((1 << 26) - 3, 1), (3, 8)])
def test_frame_numbers_whose_coded_length_changes_at_a_seam(hooks_handle, ref, first, step):
    """c = 3, six frames: numbers first .. first + 2 take one byte less than first + 3 .. (2, 3, 4, 5 and 6 bytes of the
    header's UTF-8-like code), so chunk 1 starts with a longer header than chunk 0 ended with."""
    x = sc.material(6, 2, 1152, 16, seed=77)
    cfg, model = sc.configs(8, use_fixed=True)
    data, lens = check_stream(hooks_handle, x, None, 2, 16, cfg, first=first, step=step, ref=ref, chunk=3, model=model)
    if step == 1:
        coded = [len(orc_number(first + f)) for f in range(6)]
        assert coded[3] == coded[2] + 1 and coded[0] == coded[2] and coded[3] == coded[5]


def orc_number(v):
    from oracle import oracle as orc
    return orc.encode_to_utf8like(v)


# ---------------------------------------------------------------------------------------------------- memory kinds
@pytest.mark.parametrize("out_kind", sc.KINDS)
@pytest.mark.parametrize("in_kind", sc.KINDS)
def test_memory_kinds(hooks_handle, ref, stereo4096, in_kind, out_kind):
    """Pageable, page-locked and an unaligned interior pointer of a page-locked allocation, for either buffer: c = 2,
    seven frames + a short block of 1000 (five chunks)."""
    cfg, model = sc.configs(8, use_fixed=True)
    check_stream(hooks_handle, stereo4096[:7], stereo4096[16][:, :1000], 2, 16, cfg, in_kind=in_kind, out_kind=out_kind,
                 ref=ref, chunk=2, model=model)


# ---------------------------------------------------------------------------------------------------- host threads
@pytest.mark.parametrize("threads", [0, 1, 3, 8])
def test_host_threads(hooks_handle, ref, threads):
    """flacenc_hip_set_host_threads on pageable buffers.  c = 2, seven frames of 8192 x 3 bytes; and, because the copy
    pool slices a staging copy only from 1 MiB on (CopyPool::copy), chunks of 1536 frames of 256 x 4 bytes: 3 MiB in and
    more than 1 MiB out per chunk, over three chunks and a short block."""
    cfg, model = sc.configs(8, use_fixed=True)
    x = sc.material(8, 2, 8192, 24, seed=threads + 50)
    y = sc.material(3601, 2, 256, 24, seed=threads + 60)
    try:
        hooks_handle.set_host_threads(threads)
        check_stream(hooks_handle, x[:7], None, 3, 24, cfg, ref=ref, chunk=2, model=model)
        data, lens = check_stream(hooks_handle, y[:3600], y[3600][:, :100], 4, 24, cfg, ref=ref, chunk=1536, model=model)
        assert 1536 * 256 * 2 * 4 >= 1 << 20 and int(lens[:1536].astype(np.int64).sum()) >= 1 << 20
    finally:
        hooks_handle.set_host_threads(4)


# ---------------------------------------------------------------------------------------------------- one handle
def plan_calls():
    """(name, frames, tail, bytes per sample, bits, order, chunk)"""
    small = sc.material(6, 2, 256, 16, seed=91)
    large = sc.material(10, 2, 8192, 24, seed=92)
    eight = sc.material(6, 8, 1152, 16, seed=93)
    rule = sc.material(8, 2, 4096, 16, seed=94)
    return [("small", small[:5], small[5][:, :100], 2, 16, 8, 2),
            ("larger: the pinned staging grows", large[:9], large[9][:, :4096], 3, 24, 8, 4),
            ("small again", small[:5], small[5][:, :100], 2, 16, 8, 2),
            ("8 channels", eight[:5], eight[5][:, :777], 2, 16, 8, 2),
            ("stereo under the rule", rule[:7], rule[7][:, :1000], 2, 16, 8, 0)]


def test_one_handle_changing_plans(ref):
    """Staging that grows between calls (ensure_pinned frees and reallocates), shrinks back in use, changes channel
    count and returns to the rule: each call equals the same call on a fresh handle."""
    with _capi.Handle(0, hooks=True) as h:
        for name, x, tail, bytes_ps, bps, order, c in plan_calls():
            cfg, model = sc.configs(order, use_fixed=True)
            got = check_stream(h, x, tail, bytes_ps, bps, cfg, ref=ref, chunk=c, model=model)
            with _capi.Handle(0, hooks=True) as fresh:
                want = check_stream(fresh, x, tail, bytes_ps, bps, cfg, ref=ref, chunk=c, model=model)
            assert got[0] == want[0] and np.array_equal(got[1], want[1]), name
            if c == 0:
                assert h.debug_last_stream_plan() == (7, 2)


def test_the_call_after_a_too_small_out(ref, stereo4096):
    """out_capacity runs out at chunk 0's way out while chunk 1 is in flight: an error, the streams drained -- and the
    next call on the handle is right on every frame."""
    cfg, model = sc.configs(8, use_fixed=True)
    x, tail = stereo4096[:7], stereo4096[16][:, :1000]
    with _capi.Handle(0, hooks=True) as h:
        h.debug_set_stream_chunk(2)
        with pytest.raises(_capi.FlacencHipError) as ei:
            h.encode_pcm_stereo(sc.pack_pcm(x, tail, 2), cfg, 2, 16, 4096, sc.RATE, out=np.empty(1000, np.uint8))
        assert ei.value.code == _capi.ERR_BAD_ARGUMENT and h.debug_last_stream_plan() == (2, 5)
        check_stream(h, x, tail, 2, 16, cfg, ref=ref, chunk=2, model=model)


# ---------------------------------------------------------------------------------------------------- the rule itself
@pytest.mark.parametrize("C,bytes_ps,bps,n,F,tail,plan", [(1, 1, 8, 64, 4 * 8192 + 100, 17, (8192, 6)),
                                                          (2, 2, 16, 256, 2 * 8192 + 5, 0, (8192, 3))])
def test_the_rule_without_the_override(hooks_handle, ref, C, bytes_ps, bps, n, F, tail, plan):
    """The clamp's upper end, 8192 frames per chunk, on frames small enough that five (two) real seams cost 2 MB (17 MB)
    of PCM.  (Its 48 MiB regime starts at 100 MB: tests/test_gpu_stream_path.py holds that one to the one-call path.)"""
    x = sc.material(F + 1, C, n, bps, seed=n + C)
    cfg, model = sc.configs(8, use_fixed=True)
    check_stream(hooks_handle, x[:F], x[F][:, :tail] if tail else None, bytes_ps, bps, cfg, ref=ref, chunk=0, model=model)
    assert hooks_handle.debug_last_stream_plan() == plan


# ---------------------------------------------------------------------------------------------------- the hook
def test_the_hook_itself(ref):
    with _capi.Handle(0, hooks=True) as h:
        assert h.debug_last_stream_plan() == (0, 0)
        h.debug_set_stream_chunk(8192)
        with pytest.raises(_capi.FlacencHipError) as ei:
            h.debug_set_stream_chunk(8193)   # would pass the frame limit of flacenc_hip_fill_le_bytes_async
        assert ei.value.code == _capi.ERR_BAD_ARGUMENT
    with pytest.raises(RuntimeError):
        ref.debug_set_stream_chunk(2)        # the product library has no such symbol
