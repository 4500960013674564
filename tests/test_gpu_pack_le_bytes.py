"""flacenc_hip_pack_le_bytes on the GPU, device and host pointers, against the numpy model (tests/pcm_pack_model.py):
every width and channel count over block-size lists that mix empty, tiny, odd and long frames, frame starts on all four byte alignments,
rows with a sentinel beyond each block size, `out` inside guard regions of another sentinel, the frame counts that cross one
workgroup's worth of the scan and the 65535 of a grid's second dimension, an output one byte short, both forms, and the
round trip through flacenc_hip_fill_le_bytes.  Everything compared is bytes and integers: every comparison is exact."""
import numpy as np
import pytest
import torch

import pcm_pack_model as model
from flacenc_rs_amd import _capi

pytestmark = pytest.mark.gpu
GUARD, OUT_FILL = 64, 0xC3


@pytest.fixture(scope="module")
def h():
    with _capi.Handle(0) as handle:
        yield handle


def device_pack(h, x, bs, bytes_per, shift=0, short=0, offsets=True):
    """The call on device tensors.  `out` starts `shift` bytes into a dword, between two guards; its capacity is the
    exact need minus `short`.  -> (bytes of out's extent, offsets or None, total); guards and, when the capacity is short,
    the whole extent must come back as they were filled."""
    n, channels, stride = x.shape
    want, off, total = model.pack_le_bytes(x, bs, bytes_per)
    need = len(want)
    rows = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    sizes = torch.from_numpy(np.ascontiguousarray(bs, np.uint32).view(np.int32)).cuda()
    buf = torch.full((GUARD + shift + need + GUARD,), OUT_FILL, dtype=torch.uint8, device="cuda")
    offs = torch.full((n + 1 + 2,), -1, dtype=torch.int64, device="cuda")   # two entries of guard
    tot = torch.full((2,), -1, dtype=torch.int64, device="cuda")
    assert buf.data_ptr() % 4 == 0
    torch.cuda.synchronize()   # the call runs on the handle's stream: the tensors must be there
    rc = h.pack_le_bytes_device(rows.data_ptr(), stride, sizes.data_ptr(), n, channels, bytes_per,
                                buf.data_ptr() + GUARD + shift, need - short, offs.data_ptr() if offsets else None,
                                tot.data_ptr(), check=False)
    assert rc == (_capi.ERR_BAD_ARGUMENT if short and need else _capi.OK)
    raw = buf.cpu().numpy()
    assert (raw[:GUARD + shift] == OUT_FILL).all() and (raw[GUARD + shift + need:] == OUT_FILL).all(), "guard bytes written"
    o = offs.cpu().numpy()
    t = tot.cpu().numpy()
    assert t[1] == -1 and (o[n + 1:] == -1).all()
    if not offsets:
        assert (o == -1).all()
    return raw[GUARD + shift:GUARD + shift + need], (o[:n + 1].view(np.uint64) if offsets else None), int(t[0])


@pytest.mark.parametrize("bytes_per", model.BYTES)
@pytest.mark.parametrize("channels", model.CHANNELS)
def test_mixed_block_sizes_equal_the_model(h, bytes_per, channels):
    bs = np.array(model.MIXED, np.uint32)
    if bytes_per in (1, 3) and channels in (1, 3):   # frame starts on every byte alignment without moving `out`
        assert model.frame_start_alignments(bs, channels, bytes_per, 4096) == {0, 1, 2, 3}
    seen = set()
    for stride, shift in ((4096, 0), (4101, 1), (4096, 2), (4101, 3)):   # stride == and > the largest block
        x = model.rows(bs, channels, stride, bytes_per, seed=200 + stride + shift)
        want, off, total = model.pack_le_bytes(x, bs, bytes_per)
        got, goff, gtotal = device_pack(h, x, bs, bytes_per, shift=shift)
        assert gtotal == total and np.array_equal(goff, off)
        assert np.array_equal(got, want), (stride, shift, int(np.flatnonzero(got != want)[0]))
        assert not model.holds_sentinel(got, bytes_per, channels)
        seen |= {(a + shift) % 4 for a in model.frame_start_alignments(bs, channels, bytes_per, stride)}
        # the host form, the offsets left out, and the device form without offsets
        hout, hoff, htotal, fits = h.pack_le_bytes(x, bs, bytes_per)
        assert fits and htotal == total and np.array_equal(hoff, off) and np.array_equal(hout, want)
        got2, none, gtotal2 = device_pack(h, x, bs, bytes_per, shift=shift, offsets=False)
        assert none is None and gtotal2 == total and np.array_equal(got2, want)
    assert seen == {0, 1, 2, 3}


@pytest.mark.parametrize("bytes_per", model.BYTES)
def test_extremes_and_values_that_do_not_fit_keep_their_low_bytes(h, bytes_per):
    ext = model.extremes(bytes_per)
    n = len(ext)
    x = np.zeros((2, 2, n + 3), np.int32)
    x[0, 0, :n], x[0, 1, :n] = ext, ext[::-1]
    x[1, 0, :n], x[1, 1, :n] = ext[::-1], ext
    x[:, :, n:] = model.SENTINEL
    want, off, total = model.pack_le_bytes(x, [n, n], bytes_per)
    # the model's own statement of "low bytes": value mod 2^(8 * width), little-endian
    first = [int(v) & ((1 << (8 * bytes_per)) - 1) for v in (ext[0], ext[-1])]
    assert want[:2 * bytes_per].tobytes() == b"".join(v.to_bytes(bytes_per, "little") for v in first)
    got, goff, gtotal = device_pack(h, x, [n, n], bytes_per)
    assert gtotal == total == 2 * n and np.array_equal(goff, off) and np.array_equal(got, want)


@pytest.mark.parametrize("n_frames", [1, 2, 300, 70000])
def test_frame_counts_across_the_scan_and_the_grid(h, n_frames):
    """Block sizes 1..3 at stride 4.  300 frames take more than one wave of the scan's workgroup; 70000 take 69 of its
    steps of 1024 frames and are more than the 65535 that flacenc_hip_fill_le_bytes' grid.y allows."""
    rng = np.random.default_rng(n_frames)
    bs = rng.integers(1, 4, n_frames).astype(np.uint32)
    for channels, bytes_per, shift in ((1, 3, 1), (2, 1, 3), (3, 2, 0)):
        x = model.rows(bs, channels, 4, bytes_per, seed=n_frames + channels)
        want, off, total = model.pack_le_bytes(x, bs, bytes_per)
        got, goff, gtotal = device_pack(h, x, bs, bytes_per, shift=shift)
        assert gtotal == total and np.array_equal(goff, off) and np.array_equal(got, want)
        assert not model.holds_sentinel(got, bytes_per, channels)


def test_block_sizes_above_the_stride_count_as_the_stride(h):
    x = model.rows([9, 9, 9], 2, 9, 3, seed=3)
    bs = np.array([9, 4000000000, 2], np.uint32)
    want, off, total = model.pack_le_bytes(x, bs, 3)
    got, goff, gtotal = device_pack(h, x, bs, 3, shift=1)
    assert gtotal == total == 20 and np.array_equal(goff, off) and np.array_equal(got, want)


@pytest.mark.parametrize("bytes_per,channels", [(1, 1), (2, 2), (3, 3), (4, 8)])
def test_one_byte_short_writes_nothing_and_still_reports_the_total(h, bytes_per, channels):
    bs = np.array([5, 0, 257, 64, 3], np.uint32)
    x = model.rows(bs, channels, 260, bytes_per, seed=9)
    want, off, total = model.pack_le_bytes(x, bs, bytes_per)
    got, goff, gtotal = device_pack(h, x, bs, bytes_per, shift=1, short=1)
    assert (got == OUT_FILL).all(), "the output does not fit: nothing may be written"
    assert gtotal == total and np.array_equal(goff, off)
    # the blocking forms say so: BAD_ARGUMENT, total and offsets still written, `out` untouched
    out = np.full(len(want) + 8, 0xEE, np.uint8)
    hout, hoff, htotal, fits = h.pack_le_bytes(x, bs, bytes_per, out_capacity=len(want) - 1, out=out)
    assert not fits and htotal == total and np.array_equal(hoff, off) and (out == 0xEE).all() and hout.size == 0
    rows = torch.from_numpy(x).cuda()
    sizes = torch.from_numpy(bs.view(np.int32)).cuda()
    dout = torch.full((len(want),), OUT_FILL, dtype=torch.uint8, device="cuda")
    tot = torch.zeros(1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    rc = h.pack_le_bytes_device(rows.data_ptr(), 260, sizes.data_ptr(), len(bs), channels, bytes_per, dout.data_ptr(),
                                len(want) - 1, None, tot.data_ptr(), check=False)
    assert rc == _capi.ERR_BAD_ARGUMENT and int(tot.cpu()[0]) == total and bool((dout == OUT_FILL).all())
    h.pack_le_bytes_device(rows.data_ptr(), 260, sizes.data_ptr(), len(bs), channels, bytes_per, dout.data_ptr(),
                           len(want), None, tot.data_ptr())
    assert np.array_equal(dout.cpu().numpy(), want)


def test_no_frames_and_rejected_arguments(h):
    out, off, total, fits = h.pack_le_bytes(np.zeros((0, 2, 16), np.int32), np.zeros(0, np.uint32), 2)
    assert fits and total == 0 and out.size == 0 and off.tolist() == [0]
    x, bs = np.zeros((1, 2, 16), np.int32), np.array([16], np.uint32)
    tot, o = np.zeros(1, np.uint64), np.zeros(256, np.uint8)
    for channels, bytes_per in ((0, 2), (9, 2), (2, 0), (2, 5)):
        rc = h._lib.flacenc_hip_pack_le_bytes(h._h, x.ctypes.data, 16, bs.ctypes.data, 1, channels, bytes_per,
                                              o.ctypes.data, 256, None, tot.ctypes.data, _capi.MEM_HOST)
        assert rc == _capi.ERR_BAD_ARGUMENT, (channels, bytes_per)
    assert not o.any()


@pytest.mark.parametrize("bytes_per,channels,n", [(1, 1, 63), (2, 2, 256), (3, 3, 257), (3, 2, 1152), (4, 8, 64)])
def test_round_trip_through_fill_le_bytes(h, bytes_per, channels, n):
    nf = 5
    data = np.random.default_rng(n).integers(0, 256, nf * n * channels * bytes_per).astype(np.uint8)
    rows = h.fill_le_bytes(data.tobytes(), channels, bytes_per, n)          # [nf, channels, n]
    assert np.array_equal(rows, model.fill_le_bytes(data, channels, bytes_per, n))
    out, off, total, fits = h.pack_le_bytes(rows, [n] * nf, bytes_per)
    assert fits and total == nf * n and np.array_equal(out, data)
    # and the other way round on values that fit the width
    x = h.fill_le_bytes(out.tobytes(), channels, bytes_per, n)
    assert np.array_equal(x, rows)
