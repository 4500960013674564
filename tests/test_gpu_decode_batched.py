"""The GPU-only parts of the frame decoder (flac_decode.cpp: skim_kernel, crc16_kernel, subframe_kernel<VERIFY>) and
the single-stream index (stream_index.cpp) on mixed launches, held to the ground truth of tests/decode_cases.py:
every frame carries the samples it was written from, and tests/test_decode_cases_cpu.py has proved on the CPU that the
launches hold the alignments, frame lengths, wave compositions and damage they claim.  All comparisons are exact."""
import numpy as np
import pytest

import decode_cases as dc
import flac_write as fw
from flacenc_rs_amd import _capi, decode_cpu

pytestmark = pytest.mark.gpu

GROUPS = [(1, 8), (1, 16), (1, 24), (2, 8), (2, 12), (2, 16), (2, 20), (2, 24), (3, 16), (4, 16), (5, 16), (6, 16),
          (7, 16), (8, 16)]
CANARY = 0x5A5A1234
CANARY64 = 0x5A5A12345A5A1234


@pytest.fixture(scope="module")
def h():
    with _capi.Handle(0) as handle:
        yield handle


@pytest.fixture(scope="module")
def cpu():
    return decode_cpu.DecoderCpu(decode_cpu.build())


def dev(a):
    import torch
    return torch.from_numpy(np.array(a, copy=True)).to("cuda")


def device_decode(h, launch, channels, bps, mbs, stride=None, skew=0, expected=None):
    """The device forms on rows of `stride` words that start `skew` words into a buffer filled with CANARY.
    decode -> (samples [n, channels, mbs], block_sizes, numbers, status) after checking that every word outside
    [row, row + mbs) still holds the canary; verify (expected [n, channels, mbs]) -> status."""
    import torch
    buf, off, ln, _ = launch
    n, stride = len(off), stride or mbs
    words = skew + n * channels * stride + 64
    host = np.full(words, CANARY, np.int32)
    inside = np.zeros(words, bool)
    rows = skew + np.arange(n * channels) * stride
    for t in rows:
        inside[t:t + mbs] = True
    if expected is not None:
        view = host[skew:skew + n * channels * stride].reshape(n, channels, stride)
        view[:, :, :mbs] = expected
    d_rows = dev(host)
    d_buf, d_off, d_ln = dev(buf), dev(off.view(np.int64)), dev(ln.view(np.int32))
    st = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    if expected is not None:
        h.verify_frames_device(d_buf.data_ptr(), d_off.data_ptr(), d_ln.data_ptr(), n, channels, bps, mbs,
                               d_rows.data_ptr() + 4 * skew, stride, st.data_ptr(), stream)
        torch.cuda.synchronize()
        assert np.array_equal(d_rows.cpu().numpy(), host)                      # verify writes only status
        return st.cpu().numpy().view(np.uint32)
    bs = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    num = torch.full((n,), -1, dtype=torch.int64, device="cuda")
    h.decode_frames_device(d_buf.data_ptr(), d_off.data_ptr(), d_ln.data_ptr(), n, channels, bps, mbs,
                           d_rows.data_ptr() + 4 * skew, stride, bs.data_ptr(), num.data_ptr(), st.data_ptr(), stream)
    torch.cuda.synchronize()
    got = d_rows.cpu().numpy()
    assert (got[~inside] == CANARY).all(), np.flatnonzero(got[~inside] != CANARY)[:8]
    out = got[skew:skew + n * channels * stride].reshape(n, channels, stride)[:, :, :mbs]
    return out, bs.cpu().numpy().view(np.uint32), num.cpu().numpy().view(np.uint64), st.cpu().numpy().view(np.uint32)


def check_decoded(got, launch, channels, mbs, witness):
    """got = (samples, block sizes, numbers, status) against the ground truth of the launch and the host core."""
    out, bs, num, st = got
    entries = launch[3]
    valid = np.array([label is None for _, label in entries])
    assert not st[valid].any(), [(entries[f][0].name, int(st[f])) for f in np.flatnonzero(valid & (st != 0))[:8]]
    assert (st[~valid] != 0).all(), [entries[f] for f in np.flatnonzero(~valid & (st == 0))[:8]]
    want = dc.expected_rows(entries, channels, mbs)
    bad = np.flatnonzero((out != want).reshape(len(entries), -1).any(axis=1))
    assert bad.size == 0, [(entries[f][0].name, entries[f][1]) for f in bad[:8]]   # samples, zero tails, zero bad rows
    assert np.array_equal(bs, [c.x.shape[1] if label is None else 0 for c, label in entries])
    assert np.array_equal(st, witness[3]) and np.array_equal(bs, witness[1]) and np.array_equal(num, witness[2])
    for f, (c, label) in enumerate(entries):
        if label is None and c.number is not None:
            assert num[f] == c.number, c.name


def test_the_group_list_is_the_corpus():
    assert sorted(dc.groups()) == GROUPS


@pytest.mark.parametrize("channels,bps", GROUPS)
def test_decode_and_verify_a_mixed_launch_per_group(h, cpu, channels, bps):
    cases = dc.groups()[(channels, bps)]
    mbs = dc.max_block_size(cases)
    for layout in (dc.interleaved, dc.shuffled, dc.back_to_back):
        launch = layout(cases)
        buf, off, ln, entries = launch
        witness = cpu.decode_frames(buf, off, ln, channels, bps, mbs, threads=8)
        got = device_decode(h, launch, channels, bps, mbs)
        check_decoded(got, launch, channels, mbs, witness)
        if layout is dc.interleaved:
            check_decoded(h.decode_frames(buf, off, ln, channels, bps, mbs), launch, channels, mbs, witness)
        # verify on the same launch: the truth passes, damaged frames keep the status decode gave them
        st = device_decode(h, launch, channels, bps, mbs, expected=dc.expected_rows(entries, channels, mbs))
        assert np.array_equal(st, got[3])


def perturbed(h, launch, channels, bps, mbs, base_status, f, c, t):
    """One differing expected sample at frame f, channel c, position t: MISMATCH there, every other frame untouched."""
    entries = launch[3]
    exp = dc.expected_rows(entries, channels, mbs)
    assert entries[f][1] is None and t < entries[f][0].x.shape[1]
    exp[f, c, t] ^= 1
    st = device_decode(h, launch, channels, bps, mbs, expected=exp)
    want = base_status.copy()
    want[f] = _capi.DECODE_MISMATCH
    assert np.array_equal(st, want), (f, c, t, np.flatnonzero(st != want)[:8])


def test_verify_finds_one_differing_sample_wherever_it_lies(h):
    # mono 24-bit: order-32 frames of 72, 80 and 97 samples next to damaged copies
    cases = dc.groups()[(1, 24)]
    launch = dc.interleaved(cases)
    entries = launch[3]
    mbs = dc.max_block_size(cases)
    base = device_decode(h, launch, 1, 24, mbs, expected=dc.expected_rows(entries, 1, mbs))
    valid = [f for f, (_, label) in enumerate(entries) if label is None]
    assert not base[valid].any() and (np.delete(base, valid) != 0).all()
    lpc = [f for f in valid if entries[f][0].subs == (("lpc", 32),)]
    odd = [f for f in lpc if entries[f][0].x.shape[1] % 16]
    after_damage = [f for f in valid if f and entries[f - 1][1] is not None]
    before_damage = [f for f in valid if f + 1 < len(entries) and entries[f + 1][1] is not None]
    assert lpc and odd and after_damage and before_damage
    perturbed(h, launch, 1, 24, mbs, base, lpc[0], 0, 0)                                     # position 0
    perturbed(h, launch, 1, 24, mbs, base, lpc[1], 0, 17)                                    # inside the warm-up
    perturbed(h, launch, 1, 24, mbs, base, lpc[2], 0, 31)                                    # its last sample
    perturbed(h, launch, 1, 24, mbs, base, odd[0], 0, entries[odd[0]][0].x.shape[1] - 1)     # last of a ragged block
    perturbed(h, launch, 1, 24, mbs, base, after_damage[0], 0, 5)                            # wave neighbours damaged
    perturbed(h, launch, 1, 24, mbs, base, before_damage[-1], 0, 40)
    # the last channel of an 8-channel frame
    cases = dc.groups()[(8, 16)]
    launch = dc.interleaved(cases)
    mbs = dc.max_block_size(cases)
    base = device_decode(h, launch, 8, 16, mbs, expected=dc.expected_rows(launch[3], 8, mbs))
    perturbed(h, launch, 8, 16, mbs, base, 0, 7, mbs - 1)
    perturbed(h, launch, 8, 16, mbs, base, 0, 7, 0)
    # the side channel of each stereo assignment (coded channel 1, 0, 1), and the channel beside it
    cases = dc.side_cases()
    for bps in (8, 16, 24):
        group = [c for c in cases if c.bps == bps]
        launch = dc.back_to_back(group)
        mbs = dc.max_block_size(group)
        base = device_decode(h, launch, 2, bps, mbs, expected=dc.expected_rows(launch[3], 2, mbs))
        assert not base.any()
        for f, c in enumerate(group):
            side = {8: 1, 9: 0, 10: 1, 1: 1}[c.number]
            perturbed(h, launch, 2, bps, mbs, base, f, side, c.x.shape[1] - 1)
            perturbed(h, launch, 2, bps, mbs, base, f, 1 - side, 3)


def small_mixed_launch(channels):
    """Frames of at most 1001 samples, one of exactly 1001 among them."""
    rng = np.random.default_rng(1001 + channels)
    x = np.stack([dc.signal(rng, 1001, 16) for _ in range(channels)])
    data = fw.frame(x, channels - 1, 16, [dict(kind="fixed", order=2)] * channels, number=1)
    full = dc.Case("n 1001", data, channels, 16, x, 1, (("fixed", 2),) * channels, "")
    if channels == 1:
        cases = [c for c in dc.groups()[(1, 16)] if c.x.shape[1] <= 1001]
    else:
        cases = list(dc.channel_cases(channels))
    cases = cases[:40] + [full] + cases[40:]
    return dc.interleaved(cases)


@pytest.mark.parametrize("channels", [1, 2, 3])
def test_strides_and_row_alignment(h, channels):
    """max_block_size 1001: stride 1001 and 1003 mix 16-byte aligned rows (the vector path of run_subframe) with
    unaligned ones (the scalar path) in one launch, stride 1004 is all vector, one word of skew makes it all scalar."""
    mbs = 1001
    launch = small_mixed_launch(channels)
    entries = launch[3]
    truth = dc.expected_rows(entries, channels, mbs)
    ref = device_decode(h, launch, channels, 16, mbs, stride=1008)
    assert np.array_equal(ref[0], truth)
    exp = truth.copy()
    f = next(f for f, (c, label) in enumerate(entries) if label is None and c.x.shape[1] == 1001)
    exp[f, channels - 1, 1000] += 1                       # the last staged sample of a group of 9
    g = next(f for f, (c, label) in enumerate(entries) if label is None and c.x.shape[1] % 16 == 1)
    exp[g, 0, entries[g][0].x.shape[1] - 1] -= 1          # a group of one
    want = ref[3].copy()
    want[[f, g]] = _capi.DECODE_MISMATCH
    for stride, skew in ((1001, 0), (1003, 0), (1004, 0), (1004, 1), (1001, 1), (1003, 3)):
        got = device_decode(h, launch, channels, 16, mbs, stride=stride, skew=skew)
        for a, b in zip(got, ref):
            assert np.array_equal(a, b), (stride, skew)
        assert np.array_equal(device_decode(h, launch, channels, 16, mbs, stride=stride, skew=skew, expected=truth),
                              ref[3])
        assert np.array_equal(device_decode(h, launch, channels, 16, mbs, stride=stride, skew=skew, expected=exp),
                              want), (stride, skew)


@pytest.mark.parametrize("channels", [2, 3, 5, 6, 7])
def test_channel_counts_fill_several_workgroups(h, cpu, channels):
    cases = dc.channel_cases(channels)
    per = 256 // channels
    assert len(cases) % per and (len(cases) > 3 * per or channels == 2)
    for launch in (dc.back_to_back(cases), dc.interleaved(cases)):
        buf, off, ln, entries = launch
        witness = cpu.decode_frames(buf, off, ln, channels, 16, 192, threads=8)
        got = h.decode_frames(buf, off, ln, channels, 16, 192)
        check_decoded(got, launch, channels, 192, witness)
        truth = dc.expected_rows(entries, channels, 192)
        assert np.array_equal(device_decode(h, launch, channels, 16, 192, expected=truth), got[3])
        f = max(f for f, (_, label) in enumerate(entries) if label is None)   # in the partial last workgroup
        perturbed(h, launch, channels, 16, 192, got[3], f, channels - 1, entries[f][0].x.shape[1] - 1)


def test_host_form_checks_every_span_against_the_buffer(h):
    cases = dc.groups()[(1, 24)][:12]
    buf, off, ln, entries = dc.back_to_back(cases)
    mbs = dc.max_block_size(cases)
    off, ln = off.copy(), ln.copy()
    ln[-1] += 1                                            # offsets[f] + lengths[f] = n_bytes + 1
    off[5] = len(buf) + 1                                  # the offset itself lies outside
    out, bs, _, st = h.decode_frames(buf, off, ln, 1, 24, mbs)
    want = dc.expected_rows(entries, 1, mbs)
    want[[5, 11]] = 0
    assert st[5] == _capi.DECODE_LENGTH and st[11] == _capi.DECODE_LENGTH and not np.delete(st, [5, 11]).any()
    assert np.array_equal(out, want) and bs[5] == 0 and bs[11] == 0


# ---------------------------------------------------------------- index
def index_device(h, data, channels, bps, max_frames, null=False):
    """flacenc_hip_index_frames_async with offsets / lengths of max_frames + 8 entries filled with a canary
    -> (offsets, lengths, ok) after checking that nothing was written past the count it reports."""
    import torch
    buf = dev(np.frombuffer(bytes(data), np.uint8)) if len(data) else None
    room = max_frames + 8
    off = dev(np.full(room, CANARY64, np.int64))
    ln = dev(np.full(room, CANARY, np.int32))
    nf = dev(np.full(1, -1, np.int64))
    ptr = 0 if (buf is None or null) else buf.data_ptr()
    h.index_frames_device(ptr, len(data), channels, bps, max_frames, off.data_ptr(), ln.data_ptr(), nf.data_ptr(),
                          torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    raw = int(nf.cpu().numpy().view(np.uint64)[0])
    n = raw & (_capi.INDEX_ERROR - 1)
    off, ln = off.cpu().numpy(), ln.cpu().numpy()
    assert n <= max_frames and (off[n:] == CANARY64).all() and (ln[n:] == CANARY).all()
    return off[:n].view(np.uint64), ln[:n].view(np.uint32), not (raw & _capi.INDEX_ERROR)


def check_prefix(got, offsets, lengths, n, ok):
    off, ln, flag_clear = got
    assert flag_clear == ok and len(off) == n
    assert np.array_equal(off, offsets[:n]) and np.array_equal(ln, lengths[:n])


@pytest.mark.parametrize("stream", ["tiny fixed", "tiny variable", "seams", "one frame"])
def test_index_equals_the_offsets_the_stream_was_built_with(h, cpu, stream):
    build = {"tiny fixed": dc.tiny_stream, "tiny variable": lambda: dc.tiny_stream(True), "seams": dc.seam_stream,
             "one frame": dc.one_frame_stream}[stream]
    name, data, offsets, lengths, channels, bps = build()
    n = len(offsets)
    check_prefix(index_device(h, data, channels, bps, n), offsets, lengths, n, True)
    check_prefix(index_device(h, data, channels, bps, n + 100), offsets, lengths, n, True)
    check_prefix(index_device(h, data, channels, bps, n - 1), offsets, lengths, n - 1, False)   # one below the count
    check_prefix(index_device(h, data, channels, bps, 0), offsets, lengths, 0, False)           # no room: no write
    for cut in (1, 3):                                    # the chain breaks in the last frame: the verified prefix
        c_off, c_ln, c_ok = cpu.index_frames(data[:-cut], channels, bps, n)
        assert not c_ok and len(c_off) == n - 1
        check_prefix(index_device(h, data[:-cut], channels, bps, n), c_off, c_ln, n - 1, False)
    check_prefix(index_device(h, b"\x55" + data, channels, bps, n), offsets, lengths, 0, False)  # no frame at byte 0
    if n > 2:                                             # a bit flipped in the middle frame: the frames before it
        f = n // 2
        bad = bytearray(data)
        bad[int(offsets[f]) + int(lengths[f]) - 3] ^= 0x04
        c_off, c_ln, c_ok = cpu.index_frames(bytes(bad), channels, bps, n)
        assert not c_ok and len(c_off) == f
        check_prefix(index_device(h, bytes(bad), channels, bps, n), offsets, lengths, f, False)


def test_index_of_an_empty_buffer(h):
    for max_frames in (0, 4):
        check_prefix(index_device(h, b"", 1, 8, max_frames), np.zeros(0, np.uint64), np.zeros(0, np.uint32), 0, True)
    name, data, offsets, lengths, channels, bps = dc.one_frame_stream()
    check_prefix(index_device(h, data, channels, bps, 1), offsets, lengths, 1, True)


def test_index_at_the_candidate_capacity(h, cpu):
    """max_frames = 16 gives room for 16 + 16 / 4 + 4096 = 4116 candidate headers.  A field of planted headers that
    fills it exactly indexes; one more candidate sets the flag and leaves a verified prefix of the chain (the candidates
    at the highest positions are dropped, so the last true frames go first); a larger max_frames clears it."""
    cap = dc.candidate_capacity(16)
    name, data, offsets, lengths, channels, bps = dc.planted_field_stream(cap - 3)
    check_prefix(index_device(h, data, channels, bps, 16), offsets, lengths, 3, True)
    for planted, prefix in ((cap - 2, 2), (cap - 1, 1), (5100, 1)):
        name, data, offsets, lengths, channels, bps = dc.planted_field_stream(planted)
        c_off, c_ln, c_ok = cpu.index_frames(data, channels, bps, 16)                 # the host core has no such limit
        assert c_ok and np.array_equal(c_off, offsets) and np.array_equal(c_ln, lengths)
        check_prefix(index_device(h, data, channels, bps, 16), offsets, lengths, prefix, False)
    # 5103 candidates: max_frames = 806 is the first whose capacity covers them
    assert dc.candidate_capacity(806) == 5103
    check_prefix(index_device(h, data, channels, bps, 806), offsets, lengths, 3, True)
    got = index_device(h, data, channels, bps, 805)
    check_prefix(got, offsets, lengths, len(got[0]), False)
    assert len(got[0]) == 2
