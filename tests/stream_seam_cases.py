"""The one checker of tests/test_gpu_stream_seams.py: a call of flacenc_hip_encode_pcm / _stereo (packed PCM in host memory
in, frame bytes in host memory out, chunked over two staging slots and three streams -- csrc/api_stream.cpp) is held, on
EVERY frame, to the one-call device path, and on the frames next to every chunk seam to the CPU oracle.

The chunk plan comes from the test hook flacenc_hip_debug_set_stream_chunk (hooks library only), which brings a seam
down to a handful of frames; flacenc_hip_debug_last_stream_plan says what the call really ran, so a case that claims
seven chunks cannot pass as one.

check_stream asserts, in this order:
  plan        the call ran the (frames per chunk, chunks) the case expects (plan_of restates the rule) and took each
              buffer as the memory kind it is (flacenc_hip_debug_last_stream_buffers);
  own bytes   `out` keeps its 0xAB behind the bytes the call returns, `out_len` its sentinel behind the frame count;
  one call    lengths element by element and all bytes equal one flacenc_hip_encode_pack_*_async launch over the full
              frames (numbers first, first + step, ..) and a second over the short last block (first + F * step);
  seams       frame 0, the last frame of every chunk, the first of the next, the last full frame and the short last
              block equal the CPU model byte for byte (class Model: the oracle's controller + bit writer, and the
              project's models of wasted bits, the order search, the window search and the order guess) and parse (tests/flac_parse.py:
              sync, both CRCs, every field) to their number, block size and the input's samples;
  way back    flacenc_hip_index_frames_async finds exactly the offsets and lengths of `lens`; flacenc_hip_verify_frames_async
              reports 0 for every frame against the input (the short last block in a call of its own: the decoder takes
              one max_block_size).

Everything compared is integers and bytes: every comparison is exact."""
import functools

import numpy as np

import flac_parse
from flacenc_rs_amd import _capi
from oracle import oracle as orc

RATE = 44100
CANARY = 64                 # bytes of 0xAB behind the exact need of `out`
LEN_SENTINEL = 0xA5A5A5A5   # what the entries of `out_len` behind the frame count hold
LEN_GUARD = 8
KINDS = ("pageable", "pinned", "pinned+3")
RES, CRES = _capi.FRAME_RESULT_DTYPE.itemsize, _capi.CHANNEL_RESULT_DTYPE.itemsize
_W, _S, _WS, _G = (_capi.FLAG_WASTED_BITS, _capi.FLAG_ORDER_SEARCH, _capi.FLAG_WINDOW_SEARCH, _capi.FLAG_ORDER_GUESS)
# the oracle's summation orders for the flags that choose one; the generic kernel's launch computes the unflagged integers
ORACLE_FLAGS = {0: (orc.ACORR_CANONICAL, orc.SUMABS_CANONICAL),
                _capi.FLAG_GENERIC_KERNEL: (orc.ACORR_CANONICAL, orc.SUMABS_CANONICAL),
                _capi.FLAG_REFERENCE_SUM_ORDER: (orc.ACORR_REFERENCE, orc.SUMABS_STABLE)}


class Model:
    """What states a seam frame's bytes on the CPU.  Without a search flag: the oracle's controller + bit writer in the
    summation order the flags choose, under FLACENC_HIP_FLAG_WASTED_BITS tests/wasted_model.py on top of it.  With
    FLACENC_HIP_FLAG_ORDER_SEARCH, _WINDOW_SEARCH, _ORDER_GUESS or a combination: tests/order_model.py, window_model.py,
    guess_model.py (a fresh handle's K = 1 and extra windows), configured as the flags' own GPU suites configure them --
    the search's R[] is the reference's own.  A frame is stated once per (model, block, number) and shared by every case
    that holds it."""

    def __init__(self, search, wasted, ofc):
        self.search, self.wasted, self.ofc, self.key = search, wasted, ofc, (search, wasted, bytes(ofc))

    def frame(self, x, bps, rate, number):
        return _model_frame(self.key, x.tobytes(), x.shape[0], x.shape[1], bps, rate, number)


def configs(order=8, use_fixed=True, flags=0):
    """-> (the library's frame config, the Model of its seam frames; None for flags nothing here models)."""
    cfg = _capi.make_frame_config(_capi.make_config(lpc_order=order, flags=flags), use_fixed=use_fixed)
    search, wasted = flags & (_S | _WS | _G), bool(flags & _W)
    base = flags & ~(_S | _WS | _G | _W)
    if search:
        if base or search == (_S | _G):
            return cfg, None
        import order_model
        return cfg, Model(search, wasted, orc.make_frame_config(order_model.config(order), use_fixed=use_fixed))
    if base not in ORACLE_FLAGS:
        return cfg, None
    acorr, sums = ORACLE_FLAGS[base]
    return cfg, Model(0, wasted, orc.make_frame_config(orc.make_config(lpc_order=order, acorr=acorr), use_fixed=use_fixed,
                                                       fixed=orc.make_fixed_config(sum_mode=sums)))


def material(F, C, n, bps, seed, full_scale=True):
    """int32 [F, C, n]: tones + noise; with full_scale, frame 1 alternates between the width's two ends in channel 0 and
    frame 3 is uniform over the whole width in the last channel (the sign extension of every container width)."""
    x = _capi.sigen_frames(max(F, 1), C, n, bps, 57.0 + seed % 11, 0.35, 0.03, seed=4000 + seed, nthreads=2)[:F]
    lo, hi = -(1 << (bps - 1)), (1 << (bps - 1)) - 1
    if full_scale and F > 1:
        x[1, 0, 0::2] = lo
        x[1, 0, 1::2] = hi
    if full_scale and F > 3:
        x[3, C - 1] = np.random.default_rng(seed).integers(lo, hi + 1, n)
    return np.ascontiguousarray(x)


def pack_pcm(frames, tail, bytes_ps):
    """int32 [F, C, n] + [C, m] or None -> interleaved little-endian bytes, `bytes_ps` per sample."""
    parts = [np.ascontiguousarray(frames.transpose(0, 2, 1)).reshape(-1)]
    if tail is not None:
        parts.append(np.ascontiguousarray(tail.T).reshape(-1))
    flat = np.concatenate(parts).astype("<i4")
    return np.ascontiguousarray(flat.view(np.uint8).reshape(-1, 4)[:, :bytes_ps]).reshape(-1)


def buffer_of(kind, nbytes):
    """uint8 [nbytes] in ordinary memory, in page-locked memory, or 3 bytes into a page-locked allocation."""
    if kind == "pageable":
        return np.empty(nbytes, np.uint8)
    if kind == "pinned":
        return _capi.pinned_array(max(nbytes, 1))[:nbytes]
    assert kind == "pinned+3", kind
    return _capi.pinned_array(nbytes + 3)[3:]


def plan_of(chunk, F, tail_len, frame_in_bytes):
    """(frames per chunk, chunks) of a call with F full frames: the rule of api_stream.cpp, restated."""
    if F == 0 and not tail_len:
        return 0, 0
    c = chunk or min(max((48 << 20) // frame_in_bytes, 768), 8192)
    if c > F:
        c = F or 1
    return c, -(-F // c) + (1 if tail_len else 0)


def seam_frames(F, chunk, has_tail):
    """Indices (F: the short last block) of frame 0, both sides of every chunk seam, the last full frame, the tail."""
    s = set()
    if F:
        s |= {0, F - 1}
        for edge in range(chunk, F, chunk):
            s |= {edge - 1, edge}
    if has_tail:
        s.add(F)
    return sorted(s)


@functools.lru_cache(None)
def slot_bytes(C, n, bps):
    lib = _capi.load()
    b = int(lib.flacenc_hip_stereo_frame_bytes_bound(n, bps) if C == 2 else lib.flacenc_hip_frame_bytes_bound(C, n, bps))
    return (b + 15) & ~15


def one_call(ref, x, bps, cfg, rate, first, step):
    """One flacenc_hip_encode_pack_stereo_frames_async / _frames_async launch over x int32 [F, C, n] -> (bytes of the
    frames back to back, lengths uint32 [F])."""
    import torch
    F, C, n = x.shape
    if F == 0:
        return b"", np.zeros(0, np.uint32)
    stride = (n + 3) & ~3
    rows = np.zeros((F, C, stride), np.int32)
    rows[:, :, :n] = x
    d = torch.from_numpy(rows).cuda()
    slot = slot_bytes(C, n, bps)
    res = torch.empty(F * (RES if C == 2 else C * CRES), dtype=torch.uint8, device="cuda")
    out = torch.empty(F * slot, dtype=torch.uint8, device="cuda")
    lens = torch.zeros(F, dtype=torch.int32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    if C == 2:
        ref.encode_pack_stereo_frames_device(cfg, d.data_ptr(), F, n, stride, bps, rate, first, step, res.data_ptr(),
                                             out.data_ptr(), slot, lens.data_ptr(), s)
    else:
        ref.encode_pack_frames_device(cfg, d.data_ptr(), F, C, n, stride, bps, rate, first, step, res.data_ptr(),
                                      out.data_ptr(), slot, lens.data_ptr(), s)
    torch.cuda.synchronize()
    ln = lens.cpu().numpy().view(np.uint32)
    assert int(ln.max()) <= slot
    o = out.cpu().numpy().reshape(F, slot)
    keep = np.arange(slot)[None, :] < ln[:, None]
    return o[keep].tobytes(), ln


def _oracle_subframe(x, bps, ofc):
    """encode_subframe -> the bit writer's description of the subframe, from the oracle's own decision."""
    w = orc.encode_subframe(x, bps, ofc)
    d = dict(kind=w["kind"], bps=bps, samples=x)
    if w["kind"] == 0:
        d["dc_offset"] = int(x[0])
    elif w["kind"] == 2:
        d.update(order=int(w["fixed"].order), rice_order=int(w["fixed"].rice_order), rice_params=w["rice_params"],
                 residual=w["residual"])
    elif w["kind"] == 3:
        qp = w["lpc"].qp
        d.update(order=int(qp.order), shift=int(qp.shift), precision=int(qp.precision),
                 coefs=np.array(qp.coefs[:], np.int16), rice_order=int(w["lpc"].rice_order),
                 rice_params=w["rice_params"], residual=w["residual"])
    return d


def _search_model(search):
    """The frame-level model of a combination of search flags (a fresh handle: K = 1, the default extra windows)."""
    import guess_model
    import order_model
    import window_model
    if search == _S:
        return order_model
    if search & _G:
        return guess_model.Model(1, window_model.DEFAULT if search & _WS else ())
    return window_model.Model(window_model.DEFAULT, bool(search & _S))


@functools.lru_cache(4096)
def _model_frame(key, xbytes, C, n, bps, rate, number):
    search, wasted, ofc_bytes = key
    x = np.frombuffer(xbytes, np.int32).reshape(C, n)
    ofc = orc.FrameConfig.from_buffer_copy(ofc_bytes)
    assert not wasted or rate == 44100   # (flac_write, the writer of frames with wasted bits: its default rate code)
    if search:
        model = _search_model(search)
        if not wasted:
            if C == 2:
                return model.stereo_frame_bytes(x[0], x[1], bps, ofc, number=number, sample_rate=rate)
            return model.channel_frame_bytes(list(x), bps, ofc, number=number, sample_rate=rate)
        if C == 2:
            return model.wasted_stereo_frame_bytes(x[0], x[1], bps, ofc, number=number)
        return model.wasted_channel_frame_bytes(list(x), bps, ofc, number=number)   # (order and guess models only)
    if wasted:
        import wasted_model
        if C == 2:
            return wasted_model.stereo_frame_bytes(x[0], x[1], bps, ofc, number=number)
        return wasted_model.channel_frame_bytes(list(x), bps, ofc, number=number)
    if C == 2:
        want, wres = orc.encode_stereo_frames_cfg(x[None], bps, ofc)
        return orc.write_stereo_frame(want[0], x[0], x[1], bps, rate, number, wres[0, 0], wres[0, 1])
    return orc.write_frame(n, 0, bps, rate, number, [_oracle_subframe(x[c], bps, ofc) for c in range(C)])


@functools.lru_cache(4096)
def _parsed(frame, bps, rate, wasted_ok):
    p = flac_parse.parse_frame(frame, stream_bps=bps, stream_rate=rate, wasted_ok=wasted_ok)
    assert p["length"] == len(frame)
    return p["number"], p["block_size"], p["channels"]


def check_stream(h, frames, tail, bytes_ps, bps, cfg, rate=RATE, first=0, step=1, in_kind="pageable",
                 out_kind="pageable", *, ref, chunk, model=None, entry=None):
    """frames int32 [F, C, n], tail int32 [C, m] (m < n) or None, through encode_pcm (`entry` "stereo": encode_pcm_stereo,
    the default for C == 2; "channels": encode_pcm with channels = C) on the hooks handle `h` with `chunk` frames per chunk
    (0: the rule) and buffers of the memory kinds `in_kind` / `out_kind`; the one-call reference runs on `ref`, another
    handle.  `model`: the Model of `cfg` (configs()), None where it has none.
    -> (bytes, lengths) of the stream."""
    frames = np.ascontiguousarray(frames, np.int32)
    F, C, n = frames.shape
    m = 0 if tail is None else tail.shape[1]
    assert m < n and (tail is None or tail.shape[0] == C)
    total_frames = F + (1 if m else 0)
    entry = entry or ("stereo" if C == 2 else "channels")
    wasted_ok = bool(cfg.qlpc.flags & _capi.FLAG_WASTED_BITS)

    # the reference first: the exact need of `out` comes from it
    want, want_lens = one_call(ref, frames, bps, cfg, rate, first, step)
    if m:
        t_bytes, t_lens = one_call(ref, np.ascontiguousarray(tail[None], np.int32), bps, cfg, rate, first + F * step, step)
        want, want_lens = want + t_bytes, np.concatenate([want_lens, t_lens])
    assert len(want) == int(want_lens.astype(np.int64).sum())

    packed = pack_pcm(frames, tail, bytes_ps)
    pcm = buffer_of(in_kind, packed.size)
    pcm[:] = packed
    out = buffer_of(out_kind, len(want) + CANARY)
    out[:] = 0xAB
    out_len = np.full(total_frames + LEN_GUARD, LEN_SENTINEL, np.uint32)
    h.debug_set_stream_chunk(chunk)
    try:
        if entry == "stereo":
            got, lens = h.encode_pcm_stereo(pcm, cfg, bytes_ps, bps, n, rate, out=out, first_frame_number=first,
                                            frame_number_step=step, out_len=out_len)
        else:
            got, lens = h.encode_pcm(pcm, C, cfg, bytes_ps, bps, n, rate, first_frame_number=first,
                                     frame_number_step=step, out=out, out_len=out_len)
    finally:
        h.debug_set_stream_chunk(0)

    # the plan is the one the case claims
    plan = plan_of(chunk, F, m, n * C * bytes_ps)
    assert h.debug_last_stream_plan() == plan, (h.debug_last_stream_plan(), plan)
    if total_frames:   # and the buffers were taken as what they are: an interior pointer of a pinned allocation is pinned
        assert h.debug_last_stream_buffers() == (in_kind != "pageable", out_kind != "pageable"), (in_kind, out_kind)
    # nothing else written
    assert (out[got.size:] == 0xAB).all(), "bytes of `out` behind out_total were written"
    assert (out_len[total_frames:] == LEN_SENTINEL).all(), "entries of `out_len` behind the frame count were written"
    assert np.array_equal(pcm, packed), "the input was written"
    # whole-stream equality with the one-call device path
    assert lens.size == total_frames
    assert np.array_equal(lens, want_lens), np.flatnonzero(lens != want_lens)[:8]
    data = got.tobytes()
    if data != want:
        a, b = np.frombuffer(data, np.uint8), np.frombuffer(want, np.uint8)
        k = min(a.size, b.size)
        at = int(np.flatnonzero(a[:k] != b[:k])[0]) if (a[:k] != b[:k]).any() else k
        starts = np.cumsum(want_lens.astype(np.int64)) - want_lens
        raise AssertionError("bytes differ from the one-call path at byte %d (frame %d), sizes %d / %d"
                             % (at, int(np.searchsorted(starts, at, side="right")) - 1, a.size, b.size))
    if total_frames == 0:
        assert got.size == 0
        return data, lens
    offs = (np.cumsum(lens.astype(np.uint64)) - lens).astype(np.uint64)

    # seam frames against the CPU oracle and the test-side parser
    for f in seam_frames(F, plan[0], bool(m)):
        x = frames[f] if f < F else np.ascontiguousarray(tail, np.int32)
        fr = data[int(offs[f]):int(offs[f]) + int(lens[f])]
        number = first + f * step
        if model is not None:
            assert fr == model.frame(x, bps, rate, number), f
        p_number, p_block, p_channels = _parsed(fr, bps, rate, wasted_ok)
        assert p_number == number and p_block == x.shape[1], (f, p_number, p_block)
        assert p_channels.shape == x.shape and np.array_equal(p_channels, x), f

    # the way back, on every frame
    i_off, i_len, ok = h.index_frames(got, C, bps, total_frames + 4)
    assert ok and np.array_equal(i_off, offs) and np.array_equal(i_len, lens)
    if F:
        st = h.verify_frames(got, offs[:F], lens[:F], C, bps, n, frames)
        assert not st.any(), (np.flatnonzero(st)[:8], st[st != 0][:8])
    if m:
        st = h.verify_frames(got, offs[F:], lens[F:], C, bps, m, np.ascontiguousarray(tail[None], np.int32))
        assert not st.any(), st
    return data, lens
