"""flacenc_hip_md5_spans and flacenc_hip_decode_streams_md5 on the GPU.  Every expected digest comes from hashlib.md5 over
the bytes themselves, never from the library; bytes, totals and plans are compared with flacenc_hip_decode_streams on the
same input.  Every comparison is exact."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import streams_cases as cases
import stream_seam_cases as seams
from flacenc_rs_amd import _capi

pytestmark = pytest.mark.gpu
FILL = cases.FILL
EMPTY = bytes.fromhex("d41d8cd98f00b204e9800998ecf8427e")
SEAMS = (0, 1, 3, 55, 56, 57, 63, 64, 65, 119, 120, 127, 128, 129, 1000)


def want_digests(data, offsets, lengths):
    raw = bytes(data)
    return np.array([np.frombuffer(hashlib.md5(raw[int(o):int(o) + int(n)]).digest(), np.uint8)
                     for o, n in zip(offsets, lengths)], np.uint8).reshape(-1, 16)


def torch_dev():
    import torch
    return torch, torch.device("cuda:0")


def device_digests(h, data, offsets, lengths, guard=48, shift=0):
    """md5_spans on device pointers -> (digests, the guard bytes in front of and behind them).  `shift`: the digest
    array starts that many bytes off its allocation's alignment."""
    torch, dev = torch_dev()
    d_in = torch.from_numpy(np.ascontiguousarray(data)).to(dev) if len(data) else torch.zeros(1, dtype=torch.uint8, device=dev)
    n = len(offsets)
    d_out = torch.full((guard + shift + 16 * n + guard,), 0xC3, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    h.md5_spans_device(d_in.data_ptr(), len(data), offsets, lengths, d_out.data_ptr() + guard + shift)
    raw = d_out.cpu().numpy()
    lo = guard + shift
    return raw[lo:lo + 16 * n].reshape(n, 16).copy(), np.concatenate([raw[:lo], raw[lo + 16 * n:]])


def seam_layout():
    """Every length of SEAMS at every start alignment 0..7, with gaps of 1..13 bytes between the spans."""
    offsets, lengths, at = [], [], 0
    for k, n in enumerate(SEAMS):
        for align in range(8):
            at += 1 + (5 * k + 3 * align) % 13
            at += (align - at) % 8
            offsets.append(at)
            lengths.append(n)
            at += n
    return np.array(offsets, np.uint64), np.array(lengths, np.uint64), at + 9


@pytest.mark.parametrize("kind", ["device", "pageable", "pinned", "pinned+3"])
def test_padding_seams_and_alignment(hooks_handle, kind):
    h = hooks_handle
    offsets, lengths, size = seam_layout()
    assert sorted({int(o) % 8 for o in offsets}) == list(range(8)) and len(offsets) == 8 * len(SEAMS)
    rng = np.random.default_rng(0x5EA)
    data = rng.integers(0, 256, size).astype(np.uint8)
    want = want_digests(data, offsets, lengths)
    in_span = np.zeros(size, bool)
    for o, n in zip(offsets, lengths):
        in_span[int(o):int(o) + int(n)] = True
    assert (~in_span).sum() > len(offsets)
    other = data.copy()
    other[~in_span] ^= rng.integers(1, 256, int((~in_span).sum())).astype(np.uint8)   # every gap byte changes
    for buf in (data, other):
        if kind == "device":
            got, guards = device_digests(h, buf, offsets, lengths)
            assert (guards == 0xC3).all()
        else:
            src = seams.buffer_of(kind, size)
            src[:] = buf
            got = h.md5_spans(src, offsets, lengths)
        assert np.array_equal(got, want), kind


def test_lane_wave_and_workgroup_edges(hooks_handle):
    h = hooks_handle
    rng = np.random.default_rng(0xED6E)
    data = rng.integers(0, 256, 400_000).astype(np.uint8)
    for n in (1, 63, 64, 65, 257):
        lengths = rng.integers(0, 300, n).astype(np.uint64)
        offsets = rng.integers(0, 1000, n).astype(np.uint64) * 3 + np.arange(n, dtype=np.uint64) * 5
        want = want_digests(data, offsets, lengths)
        assert np.array_equal(h.md5_spans(data, offsets, lengths), want), n
        got, guards = device_digests(h, data, offsets, lengths)
        assert np.array_equal(got, want) and (guards == 0xC3).all(), n
    # one long span among short ones in the same wave
    lengths = rng.integers(0, 131, 64).astype(np.uint64)
    offsets = (rng.integers(0, 5000, 64) + 7).astype(np.uint64)
    lengths[17], offsets[17] = 300_000, 1001
    want = want_digests(data, offsets, lengths)
    assert np.array_equal(h.md5_spans(data, offsets, lengths), want)
    got, _ = device_digests(h, data, offsets, lengths)
    assert np.array_equal(got, want)
    # overlapping and repeated spans: equal ranges, equal digests
    offsets = np.array([10, 10, 11, 10, 0, 70, 10, 3], np.uint64)
    lengths = np.array([100, 100, 99, 101, 400_000, 40, 100, 0], np.uint64)
    got = h.md5_spans(data, offsets, lengths)
    assert np.array_equal(got, want_digests(data, offsets, lengths))
    assert np.array_equal(got[0], got[1]) and np.array_equal(got[0], got[6]) and not np.array_equal(got[0], got[2])
    assert got[7].tobytes() == EMPTY
    assert h.md5_spans(data, [], []).shape == (0, 16)


def test_nothing_is_written_outside_the_digest_array(hooks_handle):
    h = hooks_handle
    rng = np.random.default_rng(0x6A2D)
    data = rng.integers(0, 256, 9000).astype(np.uint8)
    for n, shift in ((1, 0), (63, 1), (64, 2), (65, 3), (130, 4)):
        lengths = rng.integers(0, 200, n).astype(np.uint64)
        offsets = rng.integers(0, 8000, n).astype(np.uint64)
        got, guards = device_digests(h, data, offsets, lengths, guard=64, shift=shift)
        assert (guards == 0xC3).all(), (n, shift)
        assert np.array_equal(got, want_digests(data, offsets, lengths)), (n, shift)


def test_arguments(hooks_handle):
    h = hooks_handle
    lib, E = h._lib, _capi
    data = np.arange(64, dtype=np.uint8)
    digests = np.full((2, 16), 0x5A, np.uint8)
    good = (np.array([0, 8], np.uint64), np.array([8, 56], np.uint64))

    def rc(off=good[0], ln=good[1], n=2, kind=E.MEM_HOST, null=None, n_bytes=64):
        ptrs = dict(bytes=data.ctypes.data, offsets=off.ctypes.data, lengths=ln.ctypes.data, digests=digests.ctypes.data)
        if null:
            ptrs[null] = None
        return lib.flacenc_hip_md5_spans(h._h, ptrs["bytes"], n_bytes, ptrs["offsets"], ptrs["lengths"], n,
                                         ptrs["digests"], kind)

    top = (1 << 64) - 1
    bad = [dict(null="bytes"), dict(null="digests"), dict(null="offsets"), dict(null="lengths"), dict(kind=7),
           dict(n=(1 << 24) + 1),
           dict(ln=np.array([8, 57], np.uint64)), dict(off=np.array([0, 65], np.uint64), ln=np.array([8, 0], np.uint64)),
           dict(n_bytes=63), dict(off=np.array([0, top - 3], np.uint64), ln=np.array([8, 8], np.uint64)),
           dict(off=np.array([0, 50], np.uint64), ln=np.array([8, top - 10], np.uint64))]
    for kw in bad:
        for kind in (E.MEM_HOST, E.MEM_DEVICE):
            assert rc(**dict(dict(kind=kind), **kw)) == E.ERR_BAD_ARGUMENT, kw
    assert (digests == 0x5A).all()
    assert rc(n=0) == E.OK and (digests == 0x5A).all()
    assert rc() == E.OK
    assert np.array_equal(digests, want_digests(data, *good))


# ---------------------------------------------------------------- decode_streams_md5
def run_plain(h, batch, max_frames=None):
    out = batch.fresh_out()
    totals, call, _ = h.decode_streams(batch.data, batch.table, batch.max_frames() if max_frames is None else max_frames,
                                       out)
    return out, totals, call


def run_md5(h, batch, max_frames=None, in_kind="pageable", out_kind="pageable"):
    src = seams.buffer_of(in_kind, len(batch.data))
    src[:] = batch.data
    out = seams.buffer_of(out_kind, batch.out_bytes)
    out[:] = FILL
    totals, call, _, digests = h.decode_streams_md5(src, batch.table,
                                                    batch.max_frames() if max_frames is None else max_frames, out)
    return np.array(out, copy=True), totals, call, digests


def run_md5_device(h, batch, max_frames=None, md5=True):
    """On device pointers, with guard bytes around the digests; md5 False: flacenc_hip_decode_streams, no digests."""
    torch, dev = torch_dev()
    n = len(batch.streams)
    d_in = torch.from_numpy(batch.data).to(dev)
    d_out = torch.full((batch.out_bytes,), FILL, dtype=torch.uint8, device=dev)
    d_tot = torch.full((n, 4), -1, dtype=torch.int64, device=dev)
    d_dig = torch.full((32 + 16 * n + 32,), 0xC3, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    frames = batch.max_frames() if max_frames is None else max_frames
    if md5:
        call, _ = h.decode_streams_md5_device(d_in.data_ptr(), d_in.numel(), batch.table, frames, d_out.data_ptr(),
                                              d_out.numel(), d_tot.data_ptr(), d_dig.data_ptr() + 32)
    else:
        call, _ = h.decode_streams_device(d_in.data_ptr(), d_in.numel(), batch.table, frames, d_out.data_ptr(),
                                          d_out.numel(), d_tot.data_ptr())
    raw = d_dig.cpu().numpy()
    assert (raw[:32] == 0xC3).all() and (raw[32 + 16 * n:] == 0xC3).all() and (md5 or (raw == 0xC3).all())
    return d_out.cpu().numpy(), d_tot.cpu().numpy().astype(np.uint64), call, raw[32:32 + 16 * n].reshape(n, 16).copy()


def slot_digests(batch, out, totals):
    """hashlib over the first totals[s][1] * channels * width bytes of every slot."""
    want = []
    for i, s in enumerate(batch.streams):
        n = int(totals[i][1]) * s.channels * s.width
        assert n <= batch.capacities[i]
        want.append(np.frombuffer(hashlib.md5(batch.slot(out, i)[:n].tobytes()).digest(), np.uint8))
    return np.array(want, np.uint8).reshape(-1, 16)


def check_md5(h, batch, **kw):
    ref_out, ref_totals, ref_call = run_plain(h, batch, **kw)
    want = slot_digests(batch, ref_out, ref_totals)
    for got in (run_md5(h, batch, **kw), run_md5_device(h, batch, **kw)):
        out, totals, call, digests = got
        assert np.array_equal(out, ref_out) and np.array_equal(totals, ref_totals) and call == ref_call
        assert np.array_equal(digests, want)
    return ref_out, ref_totals, want


def stop_batch():
    stops, base = cases.stops()
    m = cases.mixed()
    streams, caps = [], []
    for k, (name, (s, frames, why)) in enumerate(stops.items()):
        streams += [m[k], s]
        caps += [None, len(base.pcm)]
    streams += [m[9], base, m[6]]          # a slot that ends inside frame 3: NO_ROOM
    caps += [None, 3 * 192 * 4 + 100, None]
    return cases.Batch(streams, capacities=caps, seed=5)


def garbage_batch():
    m = cases.mixed()
    streams = []
    for i, g in enumerate(cases.garbage()):
        streams += [g, m[i % len(m)]]
    return cases.Batch(streams, seed=11)


def test_decode_streams_md5_on_a_mixed_batch(hooks_handle):
    h = hooks_handle
    m = cases.mixed()
    batch = cases.Batch(m, seed=3)
    out, totals, want = check_md5(h, batch)
    for i, s in enumerate(m):          # the whole stream decoded: the STREAMINFO digest of its ground truth
        assert int(totals[i][3]) == 0 and want[i].tobytes() == hashlib.md5(s.pcm.tobytes()).digest(), s.name
    empty = [i for i, s in enumerate(m) if len(s.data) == 0]
    assert empty and all(want[i].tobytes() == EMPTY for i in empty)
    # pinned buffers on either side give the same
    got = run_md5(h, batch, in_kind="pinned+3", out_kind="pinned")
    assert np.array_equal(got[0], out) and np.array_equal(got[3], want)


def test_decode_streams_md5_on_stops_and_garbage(hooks_handle):
    h = hooks_handle
    batch = stop_batch()
    out, totals, want = check_md5(h, batch)
    whys = {int(t[3]) for t in totals}
    assert {0, _capi.DECODE_CHAIN, _capi.DECODE_NO_ROOM, _capi.DECODE_UNSUPPORTED} <= whys
    assert any(int(t[1]) == 0 and int(t[3]) != 0 and want[i].tobytes() == EMPTY for i, t in enumerate(totals))
    out, totals, want = check_md5(h, garbage_batch())
    assert all(int(totals[2 * i][3]) != 0 for i in range(32))


def test_an_index_error_gives_the_empty_digest_for_every_stream(hooks_handle):
    h = hooks_handle
    m = cases.mixed()
    batch = cases.Batch([m[0], m[1], m[3]], gaps=[4, 4, 4])
    frames = sum(len(s.frame_sizes) for s in batch.streams)
    for run in (run_md5, run_md5_device):
        out, totals, call, digests = run(h, batch, max_frames=frames - 1)
        assert call == [_capi.INDEX_ERROR, 0] and not totals.any() and (out == FILL).all()
        assert [d.tobytes() for d in digests] == [EMPTY] * 3
    check_md5(h, batch, max_frames=frames)
    # a null digests pointer is refused and nothing is written
    out = batch.fresh_out()
    totals = np.full((3, 4), 0x77, np.uint64)
    call = np.zeros(2, np.uint64)
    rc = h._lib.flacenc_hip_decode_streams_md5(h._h, batch.data.ctypes.data, len(batch.data), batch.table.ctypes.data, 3,
                                               frames, out.ctypes.data, len(out), totals.ctypes.data, call.ctypes.data,
                                               _capi.MEM_HOST, None)
    assert rc == _capi.ERR_BAD_ARGUMENT and (out == FILL).all() and (totals == 0x77).all() and not call.any()


def test_the_plan(hooks_handle):
    h = hooks_handle
    m = cases.mixed()
    four = [m[0], m[1], m[3], m[4]]
    many = cases.Batch([four[i % 4] for i in range(400)], spacing=2)
    few = cases.Batch(four)
    plans = {}
    for name, batch in (("4", few), ("400", many)):
        ref = run_plain(h, batch, max_frames=many.max_frames())
        plans[name, "host", "plain"] = h.debug_last_decode_streams_plan()
        got = run_md5(h, batch, max_frames=many.max_frames())
        plans[name, "host", "md5"] = h.debug_last_decode_streams_plan()
        want = slot_digests(batch, ref[0], ref[1])
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[3], want)
        run_md5_device(h, batch, max_frames=many.max_frames(), md5=False)
        plans[name, "device", "plain"] = h.debug_last_decode_streams_plan()
        got = run_md5_device(h, batch, max_frames=many.max_frames())
        plans[name, "device", "md5"] = h.debug_last_decode_streams_plan()
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[3], want)
    for kind in ("host", "device"):
        for form in ("plain", "md5"):
            assert plans["4", kind, form] == plans["400", kind, form], (kind, form)
        plain, p = plans["4", kind, "plain"], plans["4", kind, "md5"]
        # launches, synchronisations, transfers, channel classes
        assert 0 < p[0] - plain[0] <= 2 and p[1] == plain[1] and 0 <= p[2] - plain[2] <= 1 and p[3] == plain[3] == 4, kind
    plain = plans["4", "host", "plain"]
    # decode_streams afterwards on the same handle: its old plan
    run_plain(h, few, max_frames=many.max_frames())
    assert h.debug_last_decode_streams_plan() == plain


def test_handle_reuse(hooks_handle):
    h = hooks_handle
    rng = np.random.default_rng(0x2E05E)
    data = rng.integers(0, 256, 50_000).astype(np.uint8)

    def spans(n, top):
        lengths = rng.integers(0, top, n).astype(np.uint64)
        offsets = rng.integers(0, len(data) - top, n).astype(np.uint64)
        assert np.array_equal(h.md5_spans(data, offsets, lengths), want_digests(data, offsets, lengths))

    big = cases.Batch(cases.mixed() + cases.mixed()[:10], seed=13)
    small = cases.Batch(cases.mixed()[:2])
    spans(300, 2000)
    first = check_md5(h, big)
    ref = run_plain(h, small)
    spans(3, 40)
    check_md5(h, small)
    again = run_plain(h, small)
    assert np.array_equal(ref[0], again[0]) and np.array_equal(ref[1], again[1])
    spans(700, 90)
    second = check_md5(h, big)
    assert np.array_equal(first[0], second[0]) and np.array_equal(first[2], second[2])
    spans(1, 30_000)


def test_decode_many_with_device_md5(hooks_handle, tmp_path):
    """tools/decode_many.py --device-md5 on two .flac files of tools/encode_flac.py: two `MD5 OK` lines and the WAVs of the
    default path; with one STREAMINFO digest byte flipped it exits non-zero with `MD5 mismatch`."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tools"))
    import decode_flac
    import decode_many
    import encode_flac
    h = hooks_handle
    rng = np.random.default_rng(77)
    pcms = [np.cumsum(rng.integers(-300, 301, (n, 2)), axis=0).astype(np.int32).clip(-30000, 30000)
            for n in (3 * 1152 + 77, 4096 + 500)]
    files = [encode_flac.encode_pcm(pcms[0], 16, 44100, h, block_size=1152)[0],
             encode_flac.encode_pcm_variable(pcms[1], 16, 44100, h, block_size=1024, levels=3)[0]]
    for i, (data, pcm) in enumerate(zip(files, pcms)):   # STREAMINFO is the first block: its digest at bytes 26..41
        assert bytes(data[:4]) == b"fLaC" and data[4] & 0x7F == 0
        assert bytes(data[26:42]) == hashlib.md5(pcm.astype("<i2").tobytes()).digest()
    paths = []
    for i, data in enumerate(files):
        paths.append(str(tmp_path / ("f%d.flac" % i)))
        open(paths[-1], "wb").write(data)
    tool = os.path.join(root, "tools", "decode_many.py")
    # the default path, in this process: decode_all without the flag, hashlib, write_wav
    os.makedirs(tmp_path / "plain")
    for i, (pcm, info) in enumerate(decode_many.decode_all(files, h)):
        assert decode_flac.md5_status(pcm, info) == "MD5 OK"
        decode_flac.write_wav(str(tmp_path / "plain" / ("f%d.wav" % i)), pcm, info)
    for (pcm, info, digest), want in zip(decode_many.decode_all(files, h, device_md5=True), pcms):
        assert digest == hashlib.md5(want.astype("<i2").tobytes()).digest() == info["md5"]
        assert decode_many.device_md5_status(digest, info) == "MD5 OK"
    dev = subprocess.run([sys.executable, tool, *paths, "--out-dir", str(tmp_path / "dev"), "--device-md5"], check=True,
                         capture_output=True, text=True)
    assert dev.stdout.count("MD5 OK") == 2
    for name in ("f0.wav", "f1.wav"):
        assert open(tmp_path / "dev" / name, "rb").read() == open(tmp_path / "plain" / name, "rb").read()
    bad = bytearray(files[1])
    bad[26 + 5] ^= 0x04
    open(paths[1], "wb").write(bytes(bad))
    p = subprocess.run([sys.executable, tool, *paths, "--out-dir", str(tmp_path / "bad"), "--device-md5"],
                       capture_output=True, text=True)
    assert p.returncode != 0 and "MD5 mismatch" in p.stderr + p.stdout
