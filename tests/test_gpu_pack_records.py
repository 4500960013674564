"""frame_pack_kernel and channel_pack_kernel on records that no encoder of this project made: the hand-built cases of
tests/pack_cases.py (explicit Rice partition orders and parameters on every residual path of the packer, empty first
partitions, mixed paths in one frame, parameter and wasted-bit extremes, the header sweep).  Each launch must give the
bytes tests/flac_write.py wrote from RFC 9639 -- which tests/test_pack_cases_cpu.py has already held to the oracle's
Frame::write and to two decoders -- and must decode back to the samples on the GPU.  Everything is exact."""
import numpy as np
import pytest

import flac_parse
import pack_cases as pc
from flacenc_rs_amd import _capi
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

GROUPS = range(pc.N_GROUPS)
# the launches that also go through the device entry points with residual rows of n + 1 words (rows off 16 bytes: the
# scalar loads): both kernels, both instances, all four residual paths -- test_the_device_launches_cover_every_path
DEVICE_SHAPES = {(True, 2, 4096, 16), (True, 2, 1152, 16), (True, 2, 1000, 16), (True, 2, 4608, 16), (True, 2, 100, 16),
                 (True, 2, 4095, 16), (True, 2, 6000, 24), (False, 3, 576, 16), (False, 8, 4096, 16), (False, 1, 97, 16)}
CANARY = 0x5A5A1234


@pytest.fixture(scope="module")
def h():
    with _capi.Handle(0) as handle:
        yield handle


def dev(a):
    import torch
    return torch.from_numpy(np.array(a, copy=True)).to("cuda")


def on_device(g):
    return (g.stereo, g.channels, g.n, g.bps) in DEVICE_SHAPES and g.rate == 44100


def pack_host(h, g, x, rec, res):
    """The host entry point -> the frames, a list of bytes."""
    pack = h.pack_stereo_frames if g.stereo else h.pack_frames
    return pack(x, rec, res, g.bps, g.rate, g.first, g.step)


def lengths_from_records(h, g, rec):
    """flacenc_hip_stereo_frame_lengths_async on the launch's records -> uint32 [F]."""
    import torch
    d_rec = dev(np.frombuffer(rec.tobytes(), np.uint8))
    d_len = torch.full((len(rec),), -1, dtype=torch.int32, device="cuda")
    h.stereo_frame_lengths_device(d_rec.data_ptr(), len(rec), g.n, g.bps, g.rate, g.first, g.step, d_len.data_ptr(),
                                  stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return d_len.cpu().numpy().view(np.uint32)


def pack_device(h, g, x, rec, res):
    """The device entry points on residual rows of n + 1 words (canaries between the rows), then the decoder on the
    packed buffer as it lies on the device.  -> (frames, decoded (samples, block sizes, numbers, status))."""
    import torch
    nf, ch, n = x.shape
    rows = np.full((nf * ch, n + 1), CANARY, np.int32)
    rows[:, :n] = res.reshape(nf * ch, n)
    d_x, d_rec, d_rows = dev(x), dev(np.frombuffer(rec.tobytes(), np.uint8)), dev(rows)
    stride = h.frame_bytes_bound(n, g.bps) if g.stereo else h.frame_bytes_bound_channels(ch, n, g.bps)
    d_out = torch.zeros((nf, stride), dtype=torch.uint8, device="cuda")
    d_len = torch.zeros(nf, dtype=torch.int32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    if g.stereo:
        h.pack_stereo_frames_device(d_x.data_ptr(), nf, n, n, d_rec.data_ptr(), d_rows.data_ptr(), n + 1, g.bps, g.rate,
                                    g.first, g.step, d_out.data_ptr(), stride, d_len.data_ptr(), stream=s)
    else:
        h.pack_frames_device(d_x.data_ptr(), nf, ch, n, n, d_rec.data_ptr(), d_rows.data_ptr(), n + 1, g.bps, g.rate,
                             g.first, g.step, d_out.data_ptr(), stride, d_len.data_ptr(), stream=s)
    d_off = torch.arange(nf, dtype=torch.int64, device="cuda") * stride
    d_dec = torch.full((nf, ch, n), CANARY, dtype=torch.int32, device="cuda")
    d_bs = torch.full((nf,), -1, dtype=torch.int32, device="cuda")
    d_num = torch.full((nf,), -1, dtype=torch.int64, device="cuda")
    d_st = torch.full((nf,), -1, dtype=torch.int32, device="cuda")
    h.decode_frames_device(d_out.data_ptr(), d_off.data_ptr(), d_len.data_ptr(), nf, ch, g.bps, n, d_dec.data_ptr(), n,
                           d_bs.data_ptr(), d_num.data_ptr(), d_st.data_ptr(), s)
    torch.cuda.synchronize()
    assert np.array_equal(d_rows.cpu().numpy(), rows)             # the packer only reads
    decoded = (d_dec.cpu().numpy(), d_bs.cpu().numpy().view(np.uint32), d_num.cpu().numpy().view(np.uint64),
               d_st.cpu().numpy().view(np.uint32))
    out, lens = d_out.cpu().numpy(), d_len.cpu().numpy().view(np.uint32)
    return [bytes(out[f, :lens[f]]) for f in range(nf)], decoded


def check_bytes(g, index, frames):
    """Every frame: the expected bytes; and, stated apart so that a failure says where, the oracle's header, the body of
    flac_write between header and CRC-16, and both CRCs by flac_parse."""
    want = pc.launch_expected(index)
    bad = []
    for f, case in enumerate(g.cases):
        got = frames[f]
        hdr = orc.write_frame_header(g.n, case.tag, g.bps, g.rate, False, g.first + f * g.step)
        ok = (len(got) == len(want[f]) and got[:len(hdr)] == hdr and got[len(hdr):-2] == pc.expected_body(case) and
              flac_parse.crc8(got[:len(hdr) - 1]) == got[len(hdr) - 1] and
              flac_parse.crc16(got[:-2]) == int.from_bytes(got[-2:], "big") and got == want[f])
        if not ok:
            first = next((i for i, (a, b) in enumerate(zip(got, want[f])) if a != b), min(len(got), len(want[f])))
            bad.append((case.name, len(got), len(want[f]), "first difference at byte %d" % first))
    assert not bad, bad


def check_decoded(g, decoded):
    out, bs, num, st = decoded
    assert not st.any(), [(g.cases[f].name, int(st[f])) for f in np.flatnonzero(st)]
    assert (bs == g.n).all()
    assert np.array_equal(num, g.first + np.arange(len(g.cases), dtype=np.uint64) * g.step)
    want = np.stack([c.x for c in g.cases])
    wrong = np.flatnonzero((out != want).reshape(len(g.cases), -1).any(axis=1))
    assert wrong.size == 0, [g.cases[f].name for f in wrong]


def test_the_device_launches_cover_every_path():
    groups = [g for g in pc.groups() if on_device(g)]
    assert {(g.stereo, g.channels, g.n, g.bps) for g in groups} == DEVICE_SHAPES
    assert {p for g in groups for c in g.cases for p in pc.paths(c) if p} == \
        {"aligned", "runs", "walk cached", "walk uncached"}
    for stereo in (True, False):                                  # both kernels, each in both instances
        assert {g.n % 4096 == 0 for g in groups if g.stereo == stereo} == {True, False}
    assert any("order == part_len walk" in c.edges for g in groups for c in g.cases)


@pytest.mark.parametrize("index", GROUPS)
def test_packed_records_equal_the_written_frames_and_decode_back(h, index):
    g = pc.groups()[index]
    for case in g.cases:
        pc.check_domain(case)                                     # nothing outside the domain reaches a launch
    x, rec, res = pc.launch_inputs(g)
    frames = pack_host(h, g, x, rec, res)
    check_bytes(g, index, frames)
    lens = np.array([len(b) for b in frames], np.uint32)
    if g.stereo:                                                  # Frame::count_bits from the records alone
        assert np.array_equal(lengths_from_records(h, g, rec), lens)
    offsets = np.concatenate([[0], np.cumsum(lens[:-1], dtype=np.uint64)]).astype(np.uint64)
    check_decoded(g, h.decode_frames(b"".join(frames), offsets, lens, g.channels, g.bps, g.n))
    if on_device(g):
        d_frames, decoded = pack_device(h, g, x, rec, res)
        check_bytes(g, index, d_frames)
        check_decoded(g, decoded)
