"""32-bit FLAC frames through the host build of the decoder's core (fdc_decode_frames_depth / fdc_index_frames_depth of
flacenc_rs_amd/csrc/flac_decode_cpu.cpp): every case of depth32_cases decodes to the samples it was written from, the
24-bit entry points answer as they always have, and the stand-alone driver runs the cases and broken copies of them
under ASan + UBSan as its own process.  No GPU."""
import shutil

import numpy as np
import pytest

import depth32_cases as d32
import flac_write as fw
from flacenc_rs_amd import decode_cpu

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


@pytest.fixture(scope="module")
def dec():
    return decode_cpu.DecoderCpu(decode_cpu.build())


@pytest.fixture(scope="module")
def cases():
    return d32.frame_cases()


def decode_one(dec, data, nch, bps, limit, maxbs=1024):
    out, bs, num, st = dec.decode_frames(data, [0], [len(data)], nch, bps, maxbs, max_bits_per_sample=limit)
    return out[0], int(bs[0]), int(num[0]), int(st[0])


def test_the_case_list_covers_what_it_should(cases):
    names = " | ".join(c["name"] for c in cases)
    assert {c["channels"] for c in cases} == {1, 2, 8}
    for needle in ("code 8 ", "code 9 ", "code 10 ", "wasted 31", "wasted 32", "parameter 30", "width 31", "36-bit",
                   "n=16", "n=17", "code 0", "34-bit") + tuple(f"lpc {o} shift {s}" for o in d32.LPC_ORDERS for s in (0, 14)):
        assert needle in names, needle
    assert any(int(np.abs(c["x"][0] - c["x"][1]).max()) == (1 << 32) - 1 for c in cases if c["channels"] == 2)


def test_every_case_decodes_to_its_input(dec, cases):
    for c in cases:
        out, bs, num, st = decode_one(dec, c["data"], c["channels"], c["bps"], 32)
        n = c["x"].shape[1]
        assert (st, bs, num) == (0, n, c["number"]), c["name"]
        assert np.array_equal(out[:, :n], c["x"]), c["name"]
        assert not out[:, n:].any()


def test_verify_and_index(dec, cases):
    for (nch, bps), group in d32.by_shape(cases).items():
        data = b"".join(c["data"] for c in group)
        lengths = np.array([len(c["data"]) for c in group], np.uint32)
        offsets = (np.cumsum(lengths) - lengths).astype(np.uint64)
        exp = np.zeros((len(group), nch, 128), np.int32)
        for f, c in enumerate(group):
            exp[f, :, : c["x"].shape[1]] = c["x"]
        st = dec.decode_frames(data, offsets, lengths, nch, bps, 128, expected=exp, max_bits_per_sample=32)[3]
        assert not st.any()
        exp[0, nch - 1, 3] ^= 1
        st = dec.decode_frames(data, offsets, lengths, nch, bps, 128, expected=exp, max_bits_per_sample=32)[3]
        assert st[0] == decode_cpu.DECODE_MISMATCH and not st[1:].any()
        off, ln, ok = dec.index_frames(data, nch, bps, len(group) + 4, max_bits_per_sample=32)
        assert ok and np.array_equal(off, offsets) and np.array_equal(ln, lengths)
        # under the default limit the same bytes hold no frame
        off, _, ok = dec.index_frames(data, nch, bps if bps <= 24 else 24, len(group) + 4, max_bits_per_sample=24)
        assert not ok and len(off) == 0


def test_mixed_streams_index_and_decode(dec):
    for s in d32.mixed_streams():
        data = b"".join(s["frames"])
        off, ln, ok = dec.index_frames(data, s["channels"], s["bps"], 16, max_bits_per_sample=32)
        assert ok and len(off) == len(s["frames"])
        out, bs, num, st = dec.decode_frames(data, off, ln, s["channels"], s["bps"], s["n"], max_bits_per_sample=32)
        assert not st.any() and (bs == s["n"]).all() and num.tolist() == list(range(len(off)))
        assert np.array_equal(out, np.stack(s["x"]))


def test_invalid_streams_with_valid_crcs_follow_the_value_rule(dec):
    """Values that leave 32 bits, and sums that leave 64: the low 32 bits of the two's-complement 64-bit computation,
    worked out in Python integers by depth32_cases."""
    for c in d32.invalid_cases():
        out, bs, _, st = decode_one(dec, c["data"], c["channels"], 32, 32)
        n = c["want"].shape[1]
        assert (st, bs) == (0, n), c["name"]
        assert np.array_equal(out[:, :n], c["want"]), c["name"]


def test_the_24_bit_entry_points_answer_as_before(dec, cases):
    c = cases[0]
    # the call: more than 24 bits is refused, with and without the depth argument at 24
    for limit, refusal in ((None, AssertionError), (24, ValueError)):
        with pytest.raises(refusal):
            decode_one(dec, c["data"], 1, 32, limit)
        with pytest.raises(refusal):
            decode_one(dec, c["data"], 1, 25, limit)
    for bad in (0, 16, 25, 33):  # the limit itself: 24 or 32
        with pytest.raises(ValueError):
            decode_one(dec, c["data"], 1, 16, bad)
    # the frame: sample-size code 7 is UNSUPPORTED (and a mismatch with the stream's 24 bits)
    for limit in (None, 24):
        assert decode_one(dec, c["data"], 1, 24, limit)[3] == decode_cpu.DECODE_UNSUPPORTED | decode_cpu.DECODE_STREAM_MISMATCH
    hdr = fw.header(1024, 0, 24, 0, ss_code=7)
    assert decode_one(dec, hdr + b"\0" * 8, 1, 24, None)[3] & decode_cpu.DECODE_UNSUPPORTED
    # under the limit of 32 a code-7 frame in a 24-bit stream is a mismatch and nothing else
    assert decode_one(dec, c["data"], 1, 24, 32)[3] == decode_cpu.DECODE_STREAM_MISMATCH
    # a shallow frame decodes to the same samples under either limit
    rng = np.random.default_rng(5)
    x = d32.sinusoid(rng, 64, bps=16)[None]
    good = fw.frame(np.stack([x[0], x[0] // 2]), 10, 16, [dict(kind="fixed", order=2)] * 2)
    a, b = decode_one(dec, good, 2, 16, None), decode_one(dec, good, 2, 16, 32)
    assert a[1:] == b[1:] == (64, 0, 0) and np.array_equal(a[0], b[0])
    assert dec.index_frames(good, 2, 16, 4)[2] and dec.index_frames(good, 2, 16, 4, max_bits_per_sample=32)[2]


def test_sanitized_driver_on_the_cases_and_their_broken_copies(dec, cases, tmp_path):
    """The FDC_MAIN program under ASan + UBSan, its own process, each frame from a buffer of exactly its own bytes: no
    report, the results of the plain build, the cases clean and the broken copies with a status."""
    exe = decode_cpu.build_sanitized_driver(str(tmp_path))
    broken = d32.broken_copies(cases)
    for (nch, bps), group in d32.by_shape(cases).items():
        blobs = [c["data"] for c in group] + [b for _, b, ch, depth in broken if (ch, depth) == (nch, bps)]
        data = b"".join(blobs)
        lengths = np.array([len(b) for b in blobs], np.uint32)
        offsets = (np.cumsum(lengths) - lengths).astype(np.uint64)
        out, bs, _, st = dec.decode_frames(data, offsets, lengths, nch, bps, 128, max_bits_per_sample=32)
        st2, bs2, out2, _, _, err = decode_cpu.run_sanitized(exe, data, offsets, lengths, nch, bps, 128, str(tmp_path),
                                                             max_bits_per_sample=32)
        assert np.array_equal(st2, st) and np.array_equal(bs2, bs) and np.array_equal(out2, out), err
        assert not st2[: len(group)].any()
        assert (st2[len(group):] != 0).all()  # a flipped bit fails a CRC (or the parse), a cut frame its length
        for f, c in enumerate(group):
            assert np.array_equal(out2[f, :, : c["x"].shape[1]], c["x"])
    # the invalid streams that reach reconstruction: the wrap at 64 bits is defined behaviour, no report
    invalid = d32.invalid_cases()
    for nch in (1, 2):
        group = [c for c in invalid if c["channels"] == nch]
        data = b"".join(c["data"] for c in group)
        lengths = np.array([len(c["data"]) for c in group], np.uint32)
        offsets = (np.cumsum(lengths) - lengths).astype(np.uint64)
        st2, _, out2, _, _, err = decode_cpu.run_sanitized(exe, data, offsets, lengths, nch, 32, 128, str(tmp_path),
                                                           max_bits_per_sample=32)
        assert not st2.any(), err
        for f, c in enumerate(group):
            assert np.array_equal(out2[f, :, : c["want"].shape[1]], c["want"]), c["name"]
