"""The frame decoder on the GPU (flacenc_hip_decode_frames / _verify_frames_async / _index_frames_async): round trips
through every encoder pipeline, the same samples and statuses as the host build of the core on crafted and mutated
frames, verify, and indexing past a planted header."""
import os
import subprocess
import sys

import numpy as np
import pytest

import test_decode_core_cpu as corpora
from flacenc_rs_amd import _capi, decode_cpu

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def h():
    with _capi.Handle(0) as handle:
        yield handle


def cpu():
    return decode_cpu.DecoderCpu(decode_cpu.build())


def strided(frames_bytes):
    """The layout of the strided pack output: frame f at f * stride."""
    stride = max(len(b) for b in frames_bytes) + 16
    buf = np.zeros(stride * len(frames_bytes), np.uint8)
    for f, b in enumerate(frames_bytes):
        buf[f * stride:f * stride + len(b)] = np.frombuffer(b, np.uint8)
    return buf, np.arange(len(frames_bytes), dtype=np.uint64) * stride, np.array([len(b) for b in frames_bytes],
                                                                                  np.uint32)


def check_round_trip(h, frames_bytes, x, bps, max_block_size=None):
    buf, off, ln = strided(frames_bytes)
    nf, nch, n = x.shape
    mbs = max_block_size or n
    out, bs, num, st = h.decode_frames(buf, off, ln, nch, bps, mbs)
    assert not st.any(), np.flatnonzero(st)[:8]
    assert (bs == n).all() and np.array_equal(num, np.arange(nf))
    assert np.array_equal(out[:, :, :n], x) and not out[:, :, n:].any()
    assert not h.verify_frames(buf, off, ln, nch, bps, mbs, np.pad(x, ((0, 0), (0, 0), (0, mbs - n)))).any()


@pytest.mark.parametrize("n,bps,order,headline", [(4096, 16, 8, True), (4096, 16, 10, False), (1152, 16, 8, True),
                                                  (256, 16, 8, True), (2304, 16, 12, True), (8192, 24, 32, True),
                                                  (16384, 24, 32, True)])
def test_stereo_pipeline_round_trip(h, n, bps, order, headline):
    nf = 24 if n <= 4096 else 6
    x = _capi.sigen_frames(nf, 2, n, bps, 200.0, 0.4, 0.3, seed=0xDEC + n)
    cfg = _capi.make_frame_config(_capi.make_config(lpc_order=order), use_fixed=True) if headline else \
        _capi.make_frame_config(_capi.make_config(lpc_order=order))
    res, resid = h.encode_stereo_frames(x, bps, cfg)
    check_round_trip(h, h.pack_stereo_frames(x, res, resid, bps, 44100), x, bps)


@pytest.mark.parametrize("nch", [1, 8])
def test_independent_channel_round_trip(h, nch):
    x = _capi.sigen_frames(10, nch, 4096, 16, 150.0, 0.5, 0.2, seed=77 + nch)
    cfg = _capi.make_frame_config(_capi.make_config(lpc_order=8), use_fixed=True)
    res, resid = h.encode_frames(x, 16, cfg)
    check_round_trip(h, h.pack_frames(x, res, resid, 16, 48000), x, 16)


def pcm_stream(h, seconds, n=4096, seed=5):
    rate = 44100
    total = int(seconds * rate)
    nf = (total + n - 1) // n
    x = _capi.sigen_frames(nf, 2, n, 16, 300.0, 0.5, 0.2, seed=seed)
    inter = np.ascontiguousarray(x.transpose(0, 2, 1)).reshape(-1, 2)[:total]
    pcm = np.ascontiguousarray(inter.astype("<i2")).view(np.uint8).reshape(-1)
    cfg = _capi.make_frame_config(_capi.make_config(lpc_order=8), use_fixed=True)
    data, lens = h.encode_pcm_stereo(pcm, cfg, 2, 16, n, rate)
    return bytes(data), lens, inter


def test_encode_pcm_stereo_short_last_frame_round_trip(h):
    data, lens, inter = pcm_stream(h, 3.3)
    off = np.concatenate([np.zeros(1, np.uint64), np.cumsum(lens[:-1], dtype=np.uint64)])
    out, bs, _, st = h.decode_frames(data, off, lens, 2, 16, 4096)
    assert not st.any() and bs[-1] == len(inter) % 4096 and (bs[:-1] == 4096).all()
    got = np.concatenate([out[f, :, :bs[f]].T for f in range(len(lens))])
    assert np.array_equal(got, inter)


def test_device_equals_host_on_crafted_and_mutated_frames(h):
    c = cpu()
    for data, nch, bps, x, number in corpora.crafted_corpus():
        want = c.decode_frames(data, [0], [len(data)], nch, bps, 32768)
        got = h.decode_frames(data, [0], [len(data)], nch, bps, 32768)
        for a, b in zip(want, got):
            assert np.array_equal(a, b)
        assert got[3][0] == 0 and got[2][0] == number
    # the host build has run this corpus under ASan + UBSan (test_decode_core_cpu); only then does it go to the device
    data, offsets, lengths, _ = corpora.mutation_corpus()
    want = c.decode_frames(data, offsets, lengths, 1, 16, 32768, threads=8)
    got = h.decode_frames(data, offsets, lengths, 1, 16, 32768)
    for a, b in zip(want, got):
        assert np.array_equal(a, b)
    assert (got[3] != 0).sum() > 0.8 * len(offsets)


def test_verify_flags_exactly_the_damaged_frame(h):
    x = _capi.sigen_frames(16, 2, 4096, 16, 200.0, 0.4, 0.3, seed=99)
    cfg = _capi.make_frame_config(_capi.make_config(lpc_order=8), use_fixed=True)
    res, resid = h.encode_stereo_frames(x, 16, cfg)
    frames = h.pack_stereo_frames(x, res, resid, 16, 44100)
    buf, off, ln = strided(frames)
    assert not h.verify_frames(buf, off, ln, 2, 16, 4096, x).any()
    bad = buf.copy()
    bad[int(off[5]) + int(ln[5]) // 2] ^= 0x10          # one bit in frame 5's residual
    st = h.verify_frames(bad, off, ln, 2, 16, 4096, x)
    assert st[5] & _capi.DECODE_FRAME_CRC and not np.delete(st, 5).any()
    exp = x.copy()
    exp[9, 1, 1234] += 1                                # one expected sample of frame 9
    st = h.verify_frames(buf, off, ln, 2, 16, 4096, exp)
    assert st[9] == _capi.DECODE_MISMATCH and not np.delete(st, 9).any()


def test_index_equals_the_encoders_offsets(h):
    data, lens, _ = pcm_stream(h, 60.0, seed=6)
    want = np.concatenate([np.zeros(1, np.uint64), np.cumsum(lens[:-1], dtype=np.uint64)])
    off, ln, ok = h.index_frames(data, 2, 16, len(lens) + 8)
    assert ok and np.array_equal(off, want) and np.array_equal(ln, lens)
    # a Verbatim frame whose samples spell a valid header, spliced in after frame 40
    x = np.zeros((2, 1152), np.int64)
    fake = corpora.fw.header(4096, 10, 16, 7)
    fake = fake + b"\0" * (len(fake) % 2)
    x[0, 10:10 + len(fake) // 2] = np.frombuffer(fake, ">i2")
    plant = corpora.fw.frame(x, 1, 16, [dict(kind="verbatim"), dict(kind="verbatim")], number=41)
    cut = int(want[41])
    spliced = data[:cut] + plant + data[cut:]
    assert spliced.count(fake[:6]) >= 1
    want2 = np.concatenate([want[:41], [cut], want[41:] + len(plant)]).astype(np.uint64)
    off, ln, ok = h.index_frames(spliced, 2, 16, len(lens) + 8)
    assert ok and np.array_equal(off, want2)
    off, _, ok = h.index_frames(spliced[:-3], 2, 16, len(lens) + 8)
    assert not ok and np.array_equal(off, want2[:-1])     # the frames before the cut one, as the host core gives them
    c_off, _, c_ok = cpu().index_frames(spliced, 2, 16, len(lens) + 8)
    assert c_ok and np.array_equal(c_off, want2)


def test_decode_flac_tool_round_trips_encode_flac(tmp_path):
    flac, wav = str(tmp_path / "a.flac"), str(tmp_path / "a.wav")
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "encode_flac.py"), flac, "--seconds", "4"],
                   check=True, timeout=600)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "decode_flac.py"), flac, wav], check=True,
                       timeout=600, capture_output=True, text=True)
    assert "MD5 OK" in p.stdout
    import wave
    with wave.open(wav, "rb") as w:
        assert w.getnchannels() == 2 and w.getsampwidth() == 2 and w.getnframes() == int(4 * 44100)
