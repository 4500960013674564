"""tests/decode_cases.py proves its claims without a GPU: every valid frame decodes to its samples through the host
build of the decoder's core and through tests/flac_parse.py, every single-bit-damaged frame gets a status, and the
layouts hold the alignments, length residues and wave compositions that tests/test_gpu_decode_batched.py relies on.
The index streams give the offsets they were built with on the host core, the over-capacity stream included."""
import shutil

import numpy as np
import pytest

import decode_cases as dc
import flac_parse
from flacenc_rs_amd import decode_cpu

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


@pytest.fixture(scope="module")
def dec():
    return decode_cpu.DecoderCpu(decode_cpu.build())


def check_launch(dec, launch, channels, bps, mbs):
    """Valid frames: status 0, their samples, zeros beyond; damaged frames: a status and a zero row."""
    buf, off, ln, entries = launch
    out, bs, num, st = dec.decode_frames(buf, off, ln, channels, bps, mbs, threads=4)
    want = dc.expected_rows(entries, channels, mbs)
    valid = np.array([label is None for _, label in entries])
    assert not st[valid].any(), [entries[f][0].name for f in np.flatnonzero(valid & (st != 0))[:8]]
    undetected = [(entries[f][0].name, entries[f][1]) for f in np.flatnonzero(~valid & (st == 0))]
    assert not undetected, undetected                         # the share that may go undetected is 0
    assert np.array_equal(out, want)
    assert np.array_equal(bs, [c.x.shape[1] if label is None else 0 for c, label in entries])
    for f, (c, label) in enumerate(entries):
        if label is None and c.number is not None:
            assert num[f] == c.number, c.name
    return st


def test_every_group_decodes_to_its_samples_and_every_flip_is_caught(dec):
    groups = dc.groups()
    assert {(1, 8), (1, 16), (1, 24), (2, 8), (2, 16), (2, 24)} <= set(groups)
    flips = 0
    for (channels, bps), cases in groups.items():
        mbs = dc.max_block_size(cases)
        check_launch(dec, dc.back_to_back(cases), channels, bps, mbs)
        check_launch(dec, dc.shuffled(cases), channels, bps, mbs)
        launch = dc.interleaved(cases)
        st = check_launch(dec, launch, channels, bps, mbs)
        labels = [label for _, label in launch[3] if label is not None]
        flips += len(labels)
        for want in ("sync", "blocking", "block size", "sample rate", "channels", "sample size", "number", "crc8",
                     "body first", "body last", "crc16 hi", "crc16 lo"):
            assert want in labels
        if (channels, bps) == (1, 16):
            for want in ("first round lane 0", "middle round lane 31", "last round lane 63"):
                assert want in labels
        assert (st != 0).sum() == len(labels)
    assert flips > 400


def test_flac_parse_reads_the_same_samples_kinds_and_orders():
    """The second reader: independent of the product and of the writer's residual code path."""
    for (channels, bps), cases in dc.groups().items():
        for i, c in enumerate(cases):
            if c.name.startswith("crc len") and i % 8 and len(c.data) not in (10, 11, 258, 514, 770):
                continue      # the sweep's frames differ only in length; the host core above reads every one
            if c.subs is None and c.x.shape[1] > 4608:
                continue      # test_decode_core_cpu parses the imported corpora itself where flac_parse can
            ref = flac_parse.parse_frame(c.data, stream_bps=bps, wasted_ok=True)
            assert ref["length"] == len(c.data) and np.array_equal(ref["channels"], c.x), c.name
            if c.subs is not None:
                assert tuple(zip(ref["kinds"], ref["orders"])) == c.subs, c.name
            if c.number is not None:
                assert ref["number"] == c.number


def test_corner_coefficients_are_the_largest_whose_residual_fits():
    cases = dc.corner_cases()
    shifts, full = set(), 0
    for c in cases:
        ref = flac_parse.parse_frame(c.data, stream_bps=24)
        assert ref["orders"] == [32] * c.channels and np.array_equal(ref["channels"], c.x)
        lo, hi = -(1 << 23), (1 << 23) - 1
        assert c.x.max() == hi and c.x.min() == lo                     # full-scale samples
        coded = [c.x[0]] if c.channels == 1 else [c.x[0], c.x[0] - c.x[1]]
        assert c.channels == 1 or (coded[1].max() == (1 << 24) - 1 and coded[1].min() == -(1 << 24) + 1)   # 25 bits
        pat, shift = c.name.split()[1], int(c.name.split()[3])
        shifts.add(shift)
        for x in coded:
            m = dc.largest_magnitude(x, pat, shift)
            assert dc.residual_fits(x, dc.pattern_coefs(pat, m), shift)[0]
            assert m == 16383 or not dc.residual_fits(x, dc.pattern_coefs(pat, m + 1), shift)[0]
            full += m == 16383
            # the sum itself leaves 32 bits: what SubDecoder's 64-bit accumulation is for
            pred = max(abs(sum(int(k) * int(x[t - 1 - j]) for j, k in enumerate(dc.pattern_coefs(pat, m))))
                       for t in range(32, len(x)))
            assert pred >= 1 << 31 or shift == 0
    assert shifts == set(range(16)) and full >= 8
    coefs = {v for c in cases for pat in [c.name.split()[1]] for v in dc.pattern_coefs(pat, 16383)}
    assert coefs == {16383, -16384}


def test_side_cases_cover_every_assignment_at_the_ends_of_the_range():
    seen = set()
    for c in dc.side_cases():
        lo, hi = -(1 << (c.bps - 1)), (1 << (c.bps - 1)) - 1
        ref = flac_parse.parse_frame(c.data, stream_bps=c.bps)
        seen.add((c.bps, ref["channel_tag"]))
        l, r = c.x
        assert ((l == hi) & (r == lo)).any() and ((l == lo) & (r == hi)).any()
        assert {int(v) & 1 for v in l + r} == {0, 1}
    assert seen == {(b, t) for b in (8, 16, 24) for t in (1, 8, 9, 10)}


def test_crc_sweep_lengths_alignments_and_the_big_frame():
    sweep = dc.crc_sweep_cases()
    lm2 = [len(c.data) - 2 for c in sweep]
    assert lm2 == list(dc.SWEEP) and lm2[0] == 8 and lm2[-1] >= 800
    assert {v % 256 for v in lm2} == set(range(256)) and {255, 256, 257, 511, 512, 513, 767, 768, 769} <= set(lm2)
    assert len(dc.big_frame_case().data) > 65536
    for key, cases in dc.groups().items():
        if len(cases) < 8:
            continue          # a format the imported corpora hold a frame or four of
        for layout in (dc.back_to_back, dc.shuffled, dc.interleaved):
            _, off, ln, _ = layout(cases)
            assert {int(o) % 4 for o in off} == {0, 1, 2, 3}, (key, layout.__name__)   # every phase of the dword refill
            assert np.array_equal(off[1:], np.cumsum(ln[:-1], dtype=np.uint64))       # back to back


def test_wave_composition_of_the_company():
    cases = dc.groups()[(1, 16)]
    company = cases[:256]
    assert [c.name for c in company] == [c.name for c in dc.company_cases()]        # it leads the launch
    waves = dc.wave_table(company, 1)
    assert len(waves) == 4 and all(len(w) == 64 for w in waves)
    claims = dc.bucket_claims(waves)
    assert claims == {4: [0], 8: [1], 16: [2], 32: [3]}                             # each run_subframe<MAXP> in company
    kinds = {k for k, _, _ in waves[3]}
    sizes = {n for _, _, n in waves[3]}
    assert kinds == {"constant", "verbatim", "fixed", "lpc"} and {1, 16, 4097, 16384, 32768} <= sizes
    assert ("lpc", 16, 16) in waves[3]                                              # order == block size
    # the multichannel launches: frames straddle waves, and every bucket occurs in company there too
    for channels in (3, 5, 6, 7):
        cc = dc.channel_cases(channels)
        per = 256 // channels
        assert len(cc) > 3 * per and len(cc) % per and 64 % channels
        assert all(64 <= c.x.shape[1] <= 192 for c in cc)
        assert dc.bucket_claims(dc.wave_table(cc, channels))[32]
    st = dc.channel_cases(2)
    assert len(st) >= 300 and len(st) % 128 and {c.note for c in st} == {"tag 1", "tag 8", "tag 9", "tag 10"}


def test_channel_launches_decode_on_the_host_core(dec):
    for channels in (2, 3, 5, 6, 7):
        cases = dc.channel_cases(channels)
        check_launch(dec, dc.back_to_back(cases), channels, 16, 192)
        for c in cases[::23]:
            ref = flac_parse.parse_frame(c.data, stream_bps=16)
            assert np.array_equal(ref["channels"], c.x) and tuple(zip(ref["kinds"], ref["orders"])) == c.subs


def test_index_streams_give_the_offsets_they_were_built_with(dec):
    for name, data, offsets, lengths, channels, bps in (dc.tiny_stream(), dc.tiny_stream(True), dc.seam_stream(),
                                                        dc.one_frame_stream(), dc.empty_stream()):
        n = len(offsets)
        off, ln, ok = dec.index_frames(data, channels, bps, n)
        assert ok and np.array_equal(off, offsets) and np.array_equal(ln, lengths), name
        if n:
            off, ln, ok = dec.index_frames(data, channels, bps, n - 1)
            assert not ok and np.array_equal(off, offsets[:n - 1]), name
            for cut in (1, 3):
                off, ln, ok = dec.index_frames(data[:-cut], channels, bps, n)
                assert not ok and np.array_equal(off, offsets[:n - 1]) and np.array_equal(ln, lengths[:n - 1]), name
            off, _, ok = dec.index_frames(b"\x55" + data, channels, bps, n)
            assert not ok and len(off) == 0
    lens = dc.tiny_stream()[3]
    assert lens.min() >= 8 and lens.max() <= 40 and len(lens) >= 3000
    assert {int(o) % 16 for o in dc.seam_stream()[2]} >= {15, 0}
    assert {int(o) % 4096 for o in dc.seam_stream()[2]} >= {4095, 0, 1}
    assert flac_parse.parse_frame(dc.seam_stream()[1][15:32], stream_bps=8)["variable"] == 1
    assert flac_parse.parse_frame(dc.tiny_stream()[1][:10], stream_bps=8)["variable"] == 0


def test_planted_fields_hold_the_candidates_they_say_and_index_on_the_host_core(dec):
    cap = dc.candidate_capacity(16)
    assert cap == 4116
    for planted in (cap - 3, cap - 2, 5100):
        name, data, offsets, lengths, channels, bps = dc.planted_field_stream(planted)
        assert dc.count_candidates(data, channels, bps) == planted + 3, name
        off, ln, ok = dec.index_frames(data, channels, bps, 16)
        assert ok and np.array_equal(off, offsets) and np.array_equal(ln, lengths), name
    assert dc.candidate_capacity(806) == 5103 and dc.candidate_capacity(805) < 5103
