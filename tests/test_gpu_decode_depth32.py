"""32-bit FLAC streams through the nine decode calls with flacenc_hip_set_max_bits_per_sample(h, 32), against ground
truth that is none of the code under test: the frames of depth32_cases (written by flac_write from the samples they must
decode to, read back by flac_parse), numpy's little-endian packing, hashlib's MD5 and np.float32 arithmetic.  Every test
makes handles of its own -- never a shared fixture's -- so the limit it sets is gone with it."""
import hashlib
import os
import subprocess
import sys
import wave

import numpy as np
import pytest

import depth32_cases as d32
import flac_write as fw
import recover_model
from flacenc_rs_amd import _capi, decode_cpu

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAXBS = 128


@pytest.fixture(scope="module")
def cases():
    return d32.frame_cases()


@pytest.fixture(scope="module")
def mixed():
    return d32.mixed_streams()


@pytest.fixture(scope="module")
def cpu():
    return decode_cpu.DecoderCpu(decode_cpu.build())


def deep_handle(hooks=False):
    h = _capi.Handle(0, hooks=hooks)
    h.set_max_bits_per_sample(32)
    return h


def group_buffers(group, extra=()):
    blobs = [c["data"] for c in group] + list(extra)
    lengths = np.array([len(b) for b in blobs], np.uint32)
    return b"".join(blobs), (np.cumsum(lengths) - lengths).astype(np.uint64), lengths


def le_pcm(xs, width=4):
    """numpy's packing of frames of int64 [nch, n]: interleaved little-endian samples, the low `width` bytes each."""
    inter = np.concatenate([x.T for x in xs]).astype("<i4")
    return np.ascontiguousarray(inter.reshape(-1).view(np.uint8).reshape(-1, 4)[:, :width]).reshape(-1)


def test_the_setter_and_the_default():
    with _capi.Handle(0) as h:
        for bad in (0, 16, 25, 33):
            with pytest.raises(_capi.FlacencHipError) as e:
                h.set_max_bits_per_sample(bad)
            assert e.value.code == _capi.ERR_BAD_ARGUMENT
        h.set_max_bits_per_sample(32)
        h.set_max_bits_per_sample(24)
    assert _capi.load().flacenc_hip_set_max_bits_per_sample(None, 32) == _capi.ERR_BAD_ARGUMENT


def test_without_the_setter_nothing_changes(cases):
    c = cases[0]  # mono, sample-size code 7
    data, off, ln = group_buffers([c])
    for reset in (False, True):
        with _capi.Handle(0) as h:
            if reset:  # 32 and back: the default again
                h.set_max_bits_per_sample(32)
                h.set_max_bits_per_sample(24)
            for call in (lambda: h.decode_frames(data, off, ln, 1, 32, MAXBS),
                         lambda: h.verify_frames(data, off, ln, 1, 32, MAXBS, np.zeros((1, 1, MAXBS), np.int32)),
                         lambda: h.index_frames(data, 1, 32, 8),
                         lambda: h.decode_pcm(data, 1, 32, MAXBS, 4)):
                with pytest.raises(_capi.FlacencHipError) as e:
                    call()
                assert e.value.code == _capi.ERR_UNSUPPORTED
            out = np.zeros(4096, np.uint8)
            row = [(0, len(data), 0, out.size, 1, 32, MAXBS, 4)]
            assert h.decode_streams(data, row, 8, out, check=False)[2] == _capi.ERR_UNSUPPORTED
            assert h.decode_streams_md5(data, row, 8, out, check=False)[2] == _capi.ERR_UNSUPPORTED
            assert h.recover_streams(data, row, 8, out, check=False)[-1] == _capi.ERR_UNSUPPORTED
            assert h.decode_ranges(data, row, [(0, 8, 0, 0)], 8, out, check=False)[2] == _capi.ERR_UNSUPPORTED
            assert h.decode_ranges_planar(data, row, [(0, 8, 0, 0)], 8, out, _capi.SAMPLE_I32,
                                          check=False)[2] == _capi.ERR_UNSUPPORTED
            # the frame: a header with sample-size code 7 in a 24-bit stream
            st = h.decode_frames(data, off, ln, 1, 24, MAXBS)[3]
            assert st[0] == _capi.DECODE_UNSUPPORTED | _capi.DECODE_STREAM_MISMATCH
            assert not h.index_frames(data, 1, 24, 8)[2]
    with deep_handle() as h:  # with the limit at 32 the same frame is a mismatch in a 24-bit stream, and nothing else
        assert h.decode_frames(data, off, ln, 1, 24, MAXBS)[3][0] == _capi.DECODE_STREAM_MISMATCH


def test_decode_verify_index_and_pcm_of_every_case(cases, cpu):
    with deep_handle() as h:
        for (nch, bps), group in d32.by_shape(cases).items():
            data, off, ln = group_buffers(group)
            out, bs, num, st = h.decode_frames(data, off, ln, nch, bps, MAXBS)
            want = np.zeros((len(group), nch, MAXBS), np.int32)
            for f, c in enumerate(group):
                n = c["x"].shape[1]
                assert (int(st[f]), int(bs[f]), int(num[f])) == (0, n, c["number"]), c["name"]
                assert np.array_equal(out[f, :, :n], c["x"]), c["name"]
                want[f, :, :n] = c["x"]
            assert np.array_equal(out, want)  # zeros behind every block
            # field for field what the host build gives
            cout, cbs, cnum, cst = cpu.decode_frames(data, off, ln, nch, bps, MAXBS, max_bits_per_sample=32)
            assert np.array_equal(out, cout) and np.array_equal(bs, cbs) and np.array_equal(num, cnum)
            assert np.array_equal(st, cst)
            # verify: clean, and one changed expected sample is a MISMATCH of that frame alone
            assert not h.verify_frames(data, off, ln, nch, bps, MAXBS, want).any()
            for f in (0, len(group) - 1):
                wrong = want.copy()
                wrong[f, nch - 1, group[f]["x"].shape[1] - 1] ^= 1
                st = h.verify_frames(data, off, ln, nch, bps, MAXBS, wrong)
                assert st[f] == _capi.DECODE_MISMATCH and int(st.sum()) == _capi.DECODE_MISMATCH
            # the index finds every frame, as the host build does
            ioff, iln, ok = h.index_frames(data, nch, bps, len(group) + 8)
            assert ok and np.array_equal(ioff, off) and np.array_equal(iln, ln)
            coff, cln, cok = cpu.index_frames(data, nch, bps, len(group) + 8, max_bits_per_sample=32)
            assert cok and np.array_equal(ioff, coff) and np.array_equal(iln, cln)
            # decode_pcm: numpy's packing of the inputs
            pcm, totals = h.decode_pcm(data, nch, bps, MAXBS, 4)
            assert totals == [len(group), sum(c["x"].shape[1] for c in group), len(data), 0]
            assert np.array_equal(pcm, le_pcm([c["x"] for c in group]))


def test_broken_frames_give_the_host_builds_statuses(cases, cpu):
    broken = d32.broken_copies(cases)
    with deep_handle() as h:
        for (nch, bps), group in d32.by_shape(cases).items():
            extra = [b for _, b, ch, depth in broken if (ch, depth) == (nch, bps)]
            data, off, ln = group_buffers(group, extra)
            out, bs, num, st = h.decode_frames(data, off, ln, nch, bps, MAXBS)
            cout, cbs, cnum, cst = cpu.decode_frames(data, off, ln, nch, bps, MAXBS, max_bits_per_sample=32)
            assert np.array_equal(st, cst) and np.array_equal(bs, cbs) and np.array_equal(num, cnum)
            assert np.array_equal(out, cout)
            assert not st[: len(group)].any() and (st[len(group):] != 0).all()


def test_invalid_streams_with_valid_crcs_follow_the_value_rule(cpu):
    """Frames whose values leave 32 bits and whose sums leave 64, with valid CRCs, so that they reach reconstruction:
    the device gives the low 32 bits of the 64-bit computation (Python integers in depth32_cases), as the host build
    does, through the row writer and through the packed-PCM writer."""
    invalid = d32.invalid_cases()
    with deep_handle() as h:
        for nch in (1, 2):
            group = [c for c in invalid if c["channels"] == nch]
            data, off, ln = group_buffers(group)
            out, bs, _, st = h.decode_frames(data, off, ln, nch, 32, MAXBS)
            cout, cbs, _, cst = cpu.decode_frames(data, off, ln, nch, 32, MAXBS, max_bits_per_sample=32)
            assert not st.any() and np.array_equal(out, cout) and np.array_equal(bs, cbs)
            for f, c in enumerate(group):
                n = c["want"].shape[1]
                assert int(bs[f]) == n and np.array_equal(out[f, :, :n], c["want"]), c["name"]
            pcm, totals = h.decode_pcm(data, nch, 32, MAXBS, 4)
            assert totals[0] == len(group) and totals[3] == 0
            assert np.array_equal(pcm, le_pcm([c["want"] for c in group]))


def stream_rows(mixed, width_of=lambda s: 4 if s["bps"] > 24 else (s["bps"] + 7) // 8, room=0):
    """The mixed corpus back to back, 5 bytes between streams: (data, descriptor rows, slot offsets, widths)."""
    data, rows, at, out_at, slots = b"", [], 0, 0, []
    for s in mixed:
        raw = b"".join(s["frames"])
        width = width_of(s)
        cap = len(s["frames"]) * s["n"] * s["channels"] * width + room
        rows.append((len(data), len(raw), out_at, cap, s["channels"], s["bps"], s["n"], width))
        slots.append((out_at, cap, width))
        data += raw + b"\xAA" * 5
        out_at += cap + 3
    return data, rows, slots, out_at


def test_decode_streams_and_md5_on_the_mixed_corpus(mixed):
    data, rows, slots, out_bytes = stream_rows(mixed)
    n_frames = sum(len(s["frames"]) for s in mixed)
    with deep_handle() as h:
        out = np.full(out_bytes, 0x5A, np.uint8)
        totals, call, _ = h.decode_streams(data, rows, n_frames + 8, out)
        out5 = np.full(out_bytes, 0x5A, np.uint8)
        totals5, call5, _, digests = h.decode_streams_md5(data, rows, n_frames + 8, out5)
        assert np.array_equal(out, out5) and np.array_equal(totals, totals5) and call == call5
        assert call == [n_frames, sum(len(s["frames"]) * s["n"] for s in mixed)]
        for i, (s, (at, cap, width)) in enumerate(zip(mixed, slots)):
            want = le_pcm(s["x"], width)
            assert want.size == cap and np.array_equal(out[at:at + cap], want), i
            raw = b"".join(s["frames"])
            assert totals[i].tolist() == [len(s["frames"]), len(s["frames"]) * s["n"], len(raw), 0]
            assert digests[i].tobytes() == hashlib.md5(want.tobytes()).digest()
            # the stream decoded alone: the same bytes and totals
            alone = np.zeros(cap, np.uint8)
            t1, c1, _ = h.decode_streams(raw, [(0, len(raw), 0, cap) + rows[i][4:]], 16, alone)
            assert np.array_equal(alone, want) and t1[0].tolist() == totals[i].tolist()
            assert (out[at + cap:at + cap + 3] == 0x5A).all()


def test_decode_ranges_packed_and_planar_inside_a_mid_side_frame(mixed):
    data, rows, _, _ = stream_rows(mixed)
    si = next(i for i, s in enumerate(mixed) if s["bps"] == 32 and s["channels"] == 2)
    s = mixed[si]
    n, total = s["n"], len(s["frames"]) * s["n"]
    whole = np.concatenate(s["x"], axis=1)  # int64 [2, total]
    s16 = next(i for i, t in enumerate(mixed) if t["bps"] == 16 and t["channels"] == 1)
    whole16 = np.concatenate(mixed[s16]["x"], axis=1)
    # (first sample, samples): inside frame 1; from frame 0 into frame 2; the stream's tail and 37 samples behind its end
    spans = [(n + 5, 40), (n - 3, n + 9), (total - 21, 58)]
    with deep_handle() as h:
        # ---- packed ----
        ranges, at = [], 0
        for a, k in spans:
            ranges.append((a, k, at, si))
            at += k * 8 + 1
        ranges.append((7, 50, at, s16))  # a 16-bit range in the same call
        out = np.full(at + 50 * 2 + 4, 0x5A, np.uint8)
        totals, call, _ = h.decode_ranges(data, rows, ranges, 64, out)
        for r, (a, k) in enumerate(spans):
            got = min(k, total - a)
            assert int(totals[r][0]) == got and int(totals[r][1]) == (0 if got == k else _capi.DECODE_RANGE_END)
            o = ranges[r][2]
            assert np.array_equal(out[o:o + got * 8], le_pcm([whole[:, a:a + got]])), r
            assert (out[o + got * 8:o + k * 8 + 1] == 0x5A).all()  # packed slots are not zero-filled
        assert np.array_equal(out[at:at + 100], le_pcm([whole16[:, 7:57]], 2))
        # ---- planar int32 and float32 ----
        for fmt in (_capi.SAMPLE_I32, _capi.SAMPLE_F32):
            ranges, at = [], 0
            for a, k in spans:
                ranges.append((a, k, at, si))
                at += 2 * k * 4 + 4  # rows of 4-byte elements; a slot starts on a multiple of 4 and nothing more
            ranges.append((7, 50, at, s16))
            buf = np.full(at // 4 + 50 + 1, 0x5A5A5A5A, np.uint32)
            totals, call, _ = h.decode_ranges_planar(data, rows, ranges, 64, buf, fmt)
            for r, (a, k) in enumerate(spans):
                got = min(k, total - a)
                assert int(totals[r][0]) == got
                o = ranges[r][2] // 4
                rows_got = buf[o:o + 2 * k].reshape(2, k)
                v = whole[:, a:a + got].astype(np.int32)
                if fmt == _capi.SAMPLE_I32:
                    want = v.view(np.uint32)
                else:  # float(v), rounded to nearest even, times 2^-31 (exact: a power of two): compared as bit patterns
                    want = (v.astype(np.float32) * np.float32(2.0 ** -31)).view(np.uint32)
                assert np.array_equal(rows_got[:, :got], want), (fmt, r)
                assert not rows_got[:, got:].any()  # zeros behind the stream's end
                assert buf[o + 2 * k] == 0x5A5A5A5A
            v16 = whole16[:, 7:57].astype(np.int32)
            want16 = v16.view(np.uint32) if fmt == _capi.SAMPLE_I32 else (v16.astype(np.float32) * np.float32(2.0 ** -15)).view(np.uint32)
            assert np.array_equal(buf[at // 4:at // 4 + 50], want16[0])
        # full scale rounds to 1.0: 2^31 - 1 is not a float32
        assert np.float32(d32.HI) * np.float32(2.0 ** -31) == np.float32(1.0)


def test_float32_of_the_extremes(cases):
    c = next(c for c in cases if c["name"] == "code 10 verbatim extremes n=16")
    n = c["x"].shape[1]
    with deep_handle() as h:
        buf = np.zeros(2 * n, np.uint32)
        h.decode_ranges_planar(c["data"], [(0, len(c["data"]), 0, 0, 2, 32, n, 4)], [(0, n, 0, 0)], 4, buf, _capi.SAMPLE_F32)
        got = buf.view(np.float32).reshape(2, n)
        want = c["x"].astype(np.int32).astype(np.float32) * np.float32(2.0 ** -31)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
        assert got.max() == 1.0 and got.min() == -1.0


def test_recover_streams_through_a_broken_crc(mixed):
    s = next(s for s in mixed if s["bps"] == 32 and s["channels"] == 2)
    n, k = s["n"], len(s["frames"])
    frames = list(s["frames"])
    hit = 1
    bad = bytearray(frames[hit])
    bad[-1] ^= 0x40  # the CRC-16
    frames[hit] = bytes(bad)
    data = b"".join(frames)
    cap = k * n * 8
    # the model's answer for a 16-bit stream of the same shape with the same frame broken
    rng = np.random.default_rng(9)
    twin = [fw.frame(np.stack([d32.sinusoid(rng, n, bps=16), d32.sinusoid(rng, n, bps=16)]), 10, 16,
                     [dict(kind="fixed", order=2)] * 2, number=f) for f in range(k)]
    tb = bytearray(twin[hit])
    tb[-1] ^= 0x40
    twin[hit] = bytes(tb)
    _, model_totals, model_gaps = recover_model.expected(np.frombuffer(b"".join(twin), np.uint8), 2, 16, n, 2, k * n * 4)
    assert model_gaps == [(hit * n, n)] and model_totals[:4] == [k - 1, k * n, n, 0]
    with deep_handle() as h:
        out = np.full(cap + 8, 0x5A, np.uint8)
        _, totals, gaps, call = h.recover_streams(data, [(0, len(data), 0, cap, 2, 32, n, 4)], 16, out, max_gaps=4)
        got = [int(v) for v in totals[0]]
        assert got[:4] == model_totals[:4] and got[5:] == model_totals[5:]
        assert got[4] == len(frames[hit])  # the bytes no frame covers: the broken frame's
        assert [tuple(int(v) for v in g) for g in gaps] == [(0,) + g for g in model_gaps]
        assert call == [k - 1, k * n, 1, 0]
        xs = [x if f != hit else np.zeros_like(x) for f, x in enumerate(s["x"])]
        assert np.array_equal(out[:cap], le_pcm(xs)) and (out[cap:] == 0x5A).all()


def test_device_memory_forms_on_the_mixed_corpus(mixed):
    import torch

    data, rows, slots, out_bytes = stream_rows(mixed)
    n_frames = sum(len(s["frames"]) for s in mixed)
    with deep_handle() as h:
        d_in = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()
        d_out = torch.full((out_bytes,), 0x5A, dtype=torch.uint8, device="cuda")
        d_tot = torch.zeros(len(rows) * 4, dtype=torch.int64, device="cuda")
        call, _ = h.decode_streams_device(d_in.data_ptr(), len(data), rows, n_frames + 8, d_out.data_ptr(), out_bytes,
                                          d_tot.data_ptr())
        torch.cuda.synchronize()
        out = d_out.cpu().numpy()
        assert call[0] == n_frames
        for s, (at, cap, width) in zip(mixed, slots):
            assert np.array_equal(out[at:at + cap], le_pcm(s["x"], width))


def test_decode_flac_tool_writes_the_wav_of_a_32_bit_file(mixed, tmp_path):
    s = next(s for s in mixed if s["bps"] == 32 and s["channels"] == 2)
    pcm = le_pcm(s["x"])
    total = len(s["frames"]) * s["n"]
    flac = d32.streaminfo(32, 2, s["n"], total, hashlib.md5(pcm.tobytes()).digest()) + b"".join(s["frames"])
    src, dst = tmp_path / "deep.flac", tmp_path / "deep.wav"
    src.write_bytes(flac)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "decode_flac.py"), str(src), str(dst)],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    with wave.open(str(dst), "rb") as w:
        assert (w.getnchannels(), w.getsampwidth(), w.getnframes()) == (2, 4, total)
        assert w.readframes(total) == pcm.tobytes()
