"""flacenc_hip_encode_streams on the GPU: batches of the corpus of tests/encode_streams_cases.py against
flacenc_hip_encode_pcm on every stream alone (same handle, same config, frame numbers from 0) -- slot bytes, lengths and
totals --, a subset against the model of tests/encode_streams_model.py (the oracle's controller and bit writer with the
frame's own number), and the way back through flacenc_hip_decode_streams_md5.  PCM spans lie at odd offsets with gaps
between them, slots in shuffled order with FILL between them; whatever a call may not touch must still be FILL.  Every
comparison is exact."""
import hashlib
import importlib.util
import os
import subprocess
import sys
import wave

import numpy as np
import pytest

import encode_streams_cases as cases
import encode_streams_model as model
import flac_parse
import stream_seam_cases as seams
from flacenc_rs_amd import _capi

pytestmark = pytest.mark.gpu
FILL = cases.FILL
LEN_SENTINEL, TOTAL_SENTINEL = 0xA5A5A5A5, 0x5A5A5A5A5A5A5A5A
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_alone = {}


def alone(h, s, cfg, block):
    """flacenc_hip_encode_pcm on the stream alone -> (bytes, lengths); stated once per (stream, config, block)."""
    key = (s.name, s.x.shape, s.x.tobytes()[:64], bytes(cfg), block)
    if key not in _alone:
        if s.x.shape[1] == 0:
            _alone[key] = (b"", np.zeros(0, np.uint32))
        else:
            got, lens = h.encode_pcm(cases.pack(s.x, s.width), s.channels, cfg, s.width, s.bps, block, s.rate)
            _alone[key] = (got.tobytes(), np.array(lens, copy=True))
    return _alone[key]


def run(h, lay, cfg, block, in_kind="pageable", out_kind="pageable"):
    pcm = seams.buffer_of(in_kind, lay.pcm.size)
    pcm[:] = lay.pcm
    out = seams.buffer_of(out_kind, lay.out_bytes)
    out[:] = FILL
    F = _capi.encode_streams_frames(lay.table, block)
    lens = np.full(F + 8, LEN_SENTINEL, np.uint32)
    totals = np.full((len(lay.table) + 2, 4), TOTAL_SENTINEL, np.uint64)
    got_lens, got_totals, call, _ = h.encode_streams(pcm, lay.table, cfg, block, out, frame_lengths=lens, totals=totals)
    assert np.array_equal(pcm, lay.pcm), "the input was written"
    assert (lens[F:] == LEN_SENTINEL).all() and (totals[len(lay.table):] == TOTAL_SENTINEL).all()
    return np.array(out, copy=True), np.array(got_lens, copy=True), np.array(got_totals, copy=True), call


def check(h, streams, lay, cfg, block, out, lens, totals, call):
    """Every slot, length and total against encode_pcm on the stream alone and the cut rule; FILL everywhere else."""
    assert (out[~cases.slot_map(lay.table, lay.out_bytes)] == FILL).all(), "bytes in no slot were written"
    first = frames = nbytes = 0
    for i, s in enumerate(streams):
        want, wlens = alone(h, s, cfg, block)
        d = lay.table[i]
        off, cap = int(d["out_offset"]), int(d["out_capacity"])
        assert [int(v) for v in totals[i]] == model.totals(wlens, cap, first), (s.name, totals[i])
        j, used = model.cut(wlens, cap)
        assert np.array_equal(lens[first:first + len(wlens)], wlens), s.name
        assert out[off:off + used].tobytes() == want[:used], s.name
        assert (out[off + used:off + cap] == FILL).all(), s.name + ": bytes behind the stream's frames were written"
        first += len(wlens)
        frames += j
        nbytes += used
    assert first == lens.size and call == [frames, nbytes]


@pytest.mark.parametrize("block", [4096, 1152, 192])
def test_a_mixed_batch_equals_encode_pcm_per_stream_and_the_model(hooks_handle, block):
    """4096: the fused kernel at order 8; 1152: the sub-wave kernel; 192: the generic path."""
    h = hooks_handle
    cfg, mod = model.configs(8)
    streams = cases.mixed(block)
    lay = cases.layout(streams, block, seed=block)
    out, lens, totals, call = run(h, lay, cfg, block)
    check(h, streams, lay, cfg, block, out, lens, totals, call)
    assert (totals[:, 3] == 0).all()
    plan = h.debug_last_encode_streams_plan()
    assert plan["classes"] == 5 and plan["syncs"] == 2 and plan["transfers"] == 4
    # a subset against the oracle: a stereo tail below 64, the uncoded rate in a 4-byte container, a mono tail, hand-made rows
    for i in (3, 5, 6, 11):
        s = streams[i]
        want = b"".join(model.frames(mod, s, block))
        off = int(lay.table[i]["out_offset"])
        assert out[off:off + int(totals[i][1])].tobytes() == want, s.name


def test_the_coded_number_grows_at_frames_128_and_2048(hooks_handle):
    h = hooks_handle
    cfg, _ = model.configs(8)
    block = 64
    streams = (cases.stream("130 frames", 130 * block, 1, 16, 2, 44100, 21),
               cases.stream("2050 frames", 2050 * block, 1, 16, 2, 44100, 22))
    lay = cases.layout(streams, block, seed=5)
    out, lens, totals, call = run(h, lay, cfg, block)
    check(h, streams, lay, cfg, block, out, lens, totals, call)
    assert [int(t[0]) for t in totals] == [130, 2050] and h.debug_last_encode_streams_plan()["calls"] == 1
    for i, s in enumerate(streams):
        first, off = int(totals[i][2]), int(lay.table[i]["out_offset"])
        mine = lens[first:first + int(totals[i][0])].astype(np.int64)
        starts = np.concatenate([[0], np.cumsum(mine)])
        for f in (0, 127, 128, 129, 2047, 2048, 2049):
            if f >= len(mine):
                continue
            frame = out[off + int(starts[f]):off + int(starts[f + 1])].tobytes()
            p = flac_parse.parse_frame(frame, stream_bps=16, stream_rate=44100)   # asserts both CRCs
            assert p["number"] == f and p["length"] == len(frame) and p["block_size"] == block
            assert np.array_equal(p["channels"], s.x[:, f * block:(f + 1) * block])
            # sync and codes, the coded number, one byte for a block size of 64 (no code of its own), CRC-8
            assert p["header_bits"] // 8 == 4 + model.coded_number_bytes(f) + 1 + 1


def test_the_way_back_gives_the_digests_of_the_input_spans(hooks_handle):
    h = hooks_handle
    cfg, _ = model.configs(8)
    block = 192
    streams = cases.mixed(block)
    lay = cases.layout(streams, block, seed=11)
    out, lens, totals, call = run(h, lay, cfg, block)
    # the PCM as the digest is defined over it: ceil(bits / 8) bytes per sample
    spans = [cases.pack(s.x, (s.bps + 7) // 8) for s in streams]
    flat = np.concatenate(spans)
    offs = np.concatenate([[0], np.cumsum([len(p) for p in spans])])
    want = h.md5_spans(flat, offs[:-1], [len(p) for p in spans])
    for i, p in enumerate(spans):
        assert want[i].tobytes() == hashlib.md5(p.tobytes()).digest()
    order = np.argsort(lay.table["out_offset"], kind="stable")
    table = np.zeros(len(streams), _capi.STREAM_DESC_DTYPE)
    pcm_at = 0
    for k, i in enumerate(order):
        s = streams[i]
        table[k] = (int(lay.table[i]["out_offset"]), int(totals[i][1]), pcm_at, len(spans[i]), s.channels, s.bps, block,
                    (s.bps + 7) // 8)
        pcm_at += len(spans[i])
    back = np.zeros(max(1, pcm_at), np.uint8)
    t, c, _, digests = h.decode_streams_md5(out, table, int(call[0]), back)
    assert (t[:, 3] == 0).all() and c[0] == call[0]
    # the spans of the call's own input, where they lie (odd offsets, gaps): the STREAMINFO digest for every stream whose
    # container is ceil(bits / 8) bytes wide
    of_input = h.md5_spans(lay.pcm, [o for o, _ in lay.spans], [n for _, n in lay.spans])
    for k, i in enumerate(order):
        assert digests[k].tobytes() == want[i].tobytes(), streams[i].name
        o = int(table[k]["out_offset"])
        assert np.array_equal(back[o:o + len(spans[i])], spans[i])
        if streams[i].width == (streams[i].bps + 7) // 8:
            lo, n = lay.spans[i]
            assert of_input[i].tobytes() == digests[k].tobytes() == hashlib.md5(lay.pcm[lo:lo + n].tobytes()).digest()


def test_a_slot_one_byte_short_of_frame_j_holds_j_frames(hooks_handle):
    h = hooks_handle
    cfg, _ = model.configs(8)
    block = 192
    streams = cases.mixed(block)
    caps, cut_at = [], []
    for i, s in enumerate(streams):
        _, wlens = alone(h, s, cfg, block)
        j = i % len(wlens) if len(wlens) else 0
        if i == 1:
            caps.append(0)      # no room at all
            j = 0
        elif len(wlens) == 0 or i == 9:
            caps.append(None)   # the empty stream; one stream with room for everything next to the cut ones
            j = len(wlens)
        else:
            caps.append(int(wlens[:j + 1].sum()) - 1)
        cut_at.append(j)
    lay = cases.layout(streams, block, capacities=caps, seed=13)
    out, lens, totals, call = run(h, lay, cfg, block)
    check(h, streams, lay, cfg, block, out, lens, totals, call)
    assert [int(t[0]) for t in totals] == cut_at
    for i, s in enumerate(streams):
        full = cut_at[i] == cases.n_frames(s, block)
        assert int(totals[i][3]) == (0 if full else _capi.ENCODE_NO_ROOM), s.name
    assert int(totals[1][0]) == 0 and int(totals[1][1]) == 0 and int(totals[1][3]) == _capi.ENCODE_NO_ROOM


def test_memory_kinds_and_a_second_call_give_the_same_bytes(hooks_handle):
    import torch
    h = hooks_handle
    cfg, _ = model.configs(8)
    block = 192
    streams = cases.mixed(block)
    lay = cases.layout(streams, block, seed=17)
    base = run(h, lay, cfg, block)
    check(h, streams, lay, cfg, block, *base)
    for kinds in (("pinned", "pinned"), ("pinned+3", "pageable"), ("pageable", "pageable")):
        got = run(h, lay, cfg, block, *kinds)
        for a, b in zip(got[:3], base[:3]):
            assert np.array_equal(a, b), kinds
        assert got[3] == base[3]
    # device pointers: the PCM buffer ends with the last span's last byte
    F = _capi.encode_streams_frames(lay.table, block)
    d_pcm = torch.from_numpy(lay.pcm).cuda()
    d_out = torch.full((lay.out_bytes,), FILL, dtype=torch.uint8, device="cuda")
    d_lens = torch.full((F + 8,), LEN_SENTINEL - (1 << 32), dtype=torch.int32, device="cuda")
    d_totals = torch.full((len(streams) + 2, 4), TOTAL_SENTINEL, dtype=torch.int64, device="cuda")
    call, _ = h.encode_streams_device(d_pcm.data_ptr(), lay.pcm.size, lay.table, cfg, block, d_out.data_ptr(),
                                      lay.out_bytes, d_lens.data_ptr(), F, d_totals.data_ptr())
    plan = h.debug_last_encode_streams_plan()
    assert plan["syncs"] == 1 and plan["transfers"] == 2
    lens = d_lens.cpu().numpy().view(np.uint32)
    totals = d_totals.cpu().numpy().view(np.uint64)
    assert (lens[F:] == LEN_SENTINEL).all() and (totals[len(streams):] == TOTAL_SENTINEL).all()
    assert np.array_equal(d_out.cpu().numpy(), base[0]) and np.array_equal(lens[:F], base[1])
    assert np.array_equal(totals[:len(streams)], base[2]) and call == base[3]
    assert np.array_equal(d_pcm.cpu().numpy(), lay.pcm)


def test_three_frames_per_call_give_the_same_bytes_and_more_runs(hooks_handle):
    h = hooks_handle
    cfg, _ = model.configs(8)
    block = 192
    streams = cases.mixed(block)
    lay = cases.layout(streams, block, seed=19)
    base = run(h, lay, cfg, block)
    rule = h.debug_last_encode_streams_plan()
    h.debug_set_encode_streams_chunk(3)
    try:
        got = run(h, lay, cfg, block)
        cut = h.debug_last_encode_streams_plan()
    finally:
        h.debug_set_encode_streams_chunk(0)
    for a, b in zip(got[:3], base[:3]):
        assert np.array_equal(a, b)
    assert got[3] == base[3]
    check(h, streams, lay, cfg, block, *got)
    assert rule["full_runs"] == 5 and cut["full_runs"] > rule["full_runs"] and cut["calls"] > rule["calls"]
    for key in ("launches", "syncs", "transfers", "classes"):
        assert cut[key] == rule[key], key


def one_plus_tail(count, tails, block=192):
    x = cases.material(block + max(tails), 1, 16, 31)
    return tuple(cases.Stream("s%d" % i, x[:, :block + tails[i % len(tails)]], 1, 16, 2, 44100) for i in range(count))


def test_the_plan_depends_on_classes_and_tail_lengths_not_on_streams(hooks_handle):
    h = hooks_handle
    cfg, _ = model.configs(8)
    block = 192
    plans = {}
    for count, tails in ((4, (10, 70, 130)), (400, (10, 70, 130)), (400, (10, 70, 130, 150))):
        streams = one_plus_tail(count, tails)
        lay = cases.layout(streams, block, seed=count)
        out, lens, totals, call = run(h, lay, cfg, block)
        assert call[0] == 2 * count and (totals[:, 0] == 2).all() and (totals[:, 3] == 0).all()
        for i in (0, 1, 2, 3, count - 1):   # bytes: one stream per tail length and the last one
            check_one = alone(h, streams[i], cfg, block)
            off = int(lay.table[i]["out_offset"])
            assert out[off:off + int(totals[i][1])].tobytes() == check_one[0], i
        plans[(count, len(tails))] = h.debug_last_encode_streams_plan()
    a, b, c = plans[(4, 3)], plans[(400, 3)], plans[(400, 4)]
    assert a == b and a["classes"] == 1 and a["full_runs"] == 1 and a["tail_runs"] == 3 and a["calls"] == 4
    assert c["tail_runs"] == b["tail_runs"] + 1 and c["calls"] == b["calls"] + 1
    for key in ("launches", "syncs", "transfers", "classes", "full_runs"):
        assert c[key] == b[key], key


@pytest.mark.parametrize("flag", ["WASTED_BITS", "RICE_ESCAPE", "ORDER_GUESS"])
def test_a_flag_is_honoured_as_by_encode_pcm(hooks_handle, flag):
    h = hooks_handle
    cfg, _ = model.configs(8, flags=getattr(_capi, "FLAG_" + flag))
    block = 192
    a = cases.stream("stereo a", 2 * block + 17, 2, 16, 2, 44100, 41)
    b = cases.stream("stereo b", block + 17, 2, 16, 2, 44100, 42)
    # low bits all zero in one stream, digital silence in the middle of the other: what the first two flags act on
    a = a._replace(x=np.ascontiguousarray((a.x >> 4) << 4))
    b.x[:, 40:140] = 0
    streams = (a, b)
    lay = cases.layout(streams, block, seed=23)
    out, lens, totals, call = run(h, lay, cfg, block)
    check(h, streams, lay, cfg, block, out, lens, totals, call)
    assert call[0] == 5 and (totals[:, 3] == 0).all()
    plain, _ = model.configs(8)
    if flag == "WASTED_BITS":   # low bits all zero in every channel: the flag changes the bytes, the batch did not drop it
        assert any(alone(h, s, cfg, block)[0] != alone(h, s, plain, block)[0] for s in streams)


def raw_call(h, cfg, pcm, pcm_bytes, table, n, block, out, out_bytes, lens, max_frames, totals, call, kind=_capi.MEM_HOST):
    import ctypes as C
    ptr = lambda a: None if a is None else a.ctypes.data
    return h._lib.flacenc_hip_encode_streams(h._h, None if cfg is None else C.byref(cfg), ptr(pcm), pcm_bytes, ptr(table),
                                             n, block, ptr(out), out_bytes, ptr(lens), max_frames, ptr(totals), ptr(call),
                                             kind)


def test_bad_arguments_are_refused_and_nothing_is_written(hooks_handle):
    h = hooks_handle
    cfg, _ = model.configs(8)
    block = 192
    streams = cases.mixed(block)[1:4]
    lay = cases.layout(streams, block, seed=29)
    F = _capi.encode_streams_frames(lay.table, block)
    state = {}

    def fresh():
        state.update(pcm=lay.pcm.copy(), table=lay.table.copy(), out=np.full(lay.out_bytes, FILL, np.uint8),
                     lens=np.full(F + 4, LEN_SENTINEL, np.uint32), totals=np.full((4, 4), TOTAL_SENTINEL, np.uint64),
                     call=np.full(2, TOTAL_SENTINEL, np.uint64))
        return dict(cfg=cfg, pcm=state["pcm"], pcm_bytes=lay.pcm.size, table=state["table"], n=3, block=block,
                    out=state["out"], out_bytes=lay.out_bytes, lens=state["lens"], max_frames=F, totals=state["totals"],
                    call=state["call"])

    def refused(**change):
        kw = fresh()
        for k, v in change.items():
            if k.startswith("desc_"):
                kw["table"][1][k[5:]] = v
            else:
                kw[k] = v
        assert raw_call(h, **kw) == _capi.ERR_BAD_ARGUMENT, change
        assert (state["out"] == FILL).all() and (state["lens"] == LEN_SENTINEL).all(), change
        assert (state["totals"] == TOTAL_SENTINEL).all() and (state["call"] == TOTAL_SENTINEL).all(), change

    assert raw_call(h, **fresh()) == _capi.OK and int(state["call"][0]) == F   # the unchanged arguments pass
    for name in ("cfg", "pcm", "table", "out", "lens", "totals", "call"):
        refused(**{name: None})
    refused(kind=2)
    refused(n=(1 << 24) + 1)
    refused(pcm_bytes=lay.pcm.size - 1)           # the last span ends at the buffer's last byte
    refused(desc_offset=lay.pcm.size)
    refused(desc_total_samples=1 << 62)
    refused(out_bytes=int((lay.table["out_offset"] + lay.table["out_capacity"]).max()) - 1)
    refused(desc_out_offset=(1 << 64) - 2)
    refused(max_frames=F - 1)
    refused(block=63)
    refused(block=32768)
    for field, values in (("channels", (0, 9)), ("bytes_per_sample", (0, 5)), ("bits_per_sample", (7, 25))):
        for v in values:
            refused(**{"desc_" + field: v})
    # a stream of 2^31 frames (its span would be 128 GiB: the table is checked before anything is touched)
    kw = fresh()
    kw["table"][1]["total_samples"] = (1 << 31) * 64
    kw["table"][1]["channels"], kw["table"][1]["bytes_per_sample"], kw["table"][1]["bits_per_sample"] = 1, 1, 8
    kw.update(block=64, pcm_bytes=1 << 40, max_frames=1 << 40)
    assert raw_call(h, **kw) == _capi.ERR_BAD_ARGUMENT and (state["out"] == FILL).all()
    # no stream at all, and streams without samples, are fine
    kw = fresh()
    kw.update(n=0)
    assert raw_call(h, **kw) == _capi.OK and state["call"].tolist() == [0, 0] and (state["out"] == FILL).all()
    empty = tuple(cases.stream("e%d" % i, 0, 1 + i, 16, 2, 44100, i) for i in range(3))
    lay0 = cases.layout(empty, block, seed=31)
    out, lens, totals, call = run(h, lay0, cfg, block)
    assert call == [0, 0] and lens.size == 0 and (totals == 0).all() and (out == FILL).all()


@pytest.mark.parametrize("channels,width", [(c, b) for c in range(1, 9) for b in range(1, 5)])
def test_the_fill_kernel_equals_fill_le_bytes(hooks_handle, channels, width):
    """Every (channels, bytes per sample) instance on three frames and a tail, from each byte alignment: rows equal
    flacenc_hip_fill_le_bytes, the rest of a row up to the stride is zero, the bytes around the span are not looked at."""
    import torch
    h = hooks_handle
    block, total = 150, 3 * 150 + 37    # a block that is no multiple of 4, a tail that ends inside a group of four
    stride = (block + 3) & ~3
    rng = np.random.default_rng(channels * 8 + width)
    span = rng.integers(0, 256, total * channels * width, dtype=np.uint8)
    want = torch.zeros((4, channels, block), dtype=torch.int32, device="cuda")
    d_span = torch.from_numpy(span).cuda()
    h.fill_le_bytes_device(d_span.data_ptr(), total, channels, width, 4, block, want.data_ptr(), block)
    want = want.cpu().numpy()
    for skew in range(4):
        buf = torch.from_numpy(np.concatenate([np.full(skew, 0xEE, np.uint8), span])).cuda()   # ends with the span
        rows = torch.full((4, channels, stride), 0x55555555, dtype=torch.int32, device="cuda")
        h.debug_streams_fill(buf.data_ptr() + skew, total, channels, width, 4, block, rows.data_ptr(), stride)
        got = rows.cpu().numpy()
        assert np.array_equal(got[:, :, :block], want), skew
        assert (got[:, :, block:] == 0).all() and (got[3, :, 37:] == 0).all()


def test_encode_many_writes_files_that_decode_back(tmp_path):
    wavs = []
    for i, (ch, width, rate, n) in enumerate(((2, 2, 44100, 3 * 4096 + 500), (1, 2, 16000, 4096), (2, 3, 48000, 5000))):
        x = cases.material(n, ch, 8 * width, 50 + i)
        path = str(tmp_path / ("in%d.wav" % i))
        with wave.open(path, "wb") as w:
            w.setnchannels(ch)
            w.setsampwidth(width)
            w.setframerate(rate)
            w.writeframes(cases.pack(x, width).tobytes())
        wavs.append((path, cases.pack(x, width).tobytes(), ch, width, rate))
    out_dir = str(tmp_path / "flacs")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "encode_many.py")] + [w[0] for w in wavs]
                       + ["--out-dir", out_dir], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert "3 files" in p.stdout and "one encode call" in p.stdout
    # tools/decode_flac.py's own functions, in this process: one interpreter start is what the test is about, not four
    spec = importlib.util.spec_from_file_location("decode_flac", os.path.join(ROOT, "tools", "decode_flac.py"))
    decode_flac = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(decode_flac)
    with _capi.Handle(0) as h:
        for i, (path, payload, ch, width, rate) in enumerate(wavs):
            data = open(os.path.join(out_dir, "in%d.flac" % i), "rb").read()
            pcm, info = decode_flac.decode(data, h)
            assert decode_flac.md5_status(pcm, info) == "MD5 OK", path
            assert (info["channels"], info["bits_per_sample"], info["sample_rate"]) == (ch, 8 * width, rate)
            assert info["total_samples"] * ch * width == len(payload) and info["max_block_size"] == 4096
            back = str(tmp_path / ("back%d.wav" % i))
            decode_flac.write_wav(back, pcm, info)
            with wave.open(back, "rb") as w:
                assert (w.getnchannels(), w.getsampwidth(), w.getframerate()) == (ch, width, rate)
                assert w.readframes(w.getnframes()) == payload
