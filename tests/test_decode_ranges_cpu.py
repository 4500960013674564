"""flacenc_hip_decode_ranges without a GPU: the model the GPU tests compare against (tests/ranges_model.py) gives, for every
range of the corpus (tests/ranges_cases.py), the slice of the samples its stream was written from; the corpus holds the
shapes it claims; csrc/stream_ranges_core.h equals brute force under the sanitizers (a stand-alone program); the range
descriptor's layout, the call and its constant are the same in the C header, the numpy binding and the Rust binding; and
the SEEKTABLE helper of tools/flac_metadata.py round-trips and points at the frames of a corpus stream."""
import os
import re
import subprocess
import sys

import numpy as np

import ranges_cases as rcases
import ranges_model as rmodel
import streams_cases as cases
from flacenc_rs_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "flacenc_rs_amd", "csrc")
INCLUDE = os.path.join(ROOT, "include")
sys.path.insert(0, os.path.join(ROOT, "tools"))


def slices_of_ground_truth(rb, want):
    """Every expected slot is the slice [first, min(first + n, S)) of the PCM the stream was written from."""
    for (s, first, n), (data, tot) in zip(rb.ranges, want):
        st = rb.streams[s]
        if st.pcm is None:
            continue
        fb = st.channels * st.width
        S = len(st.pcm) // fb
        end = min(first + n, S)
        assert tot[0] == max(0, end - first), (st.name, first, n, tot)
        assert np.array_equal(data, st.pcm[first * fb:first * fb + tot[0] * fb]), (st.name, first, n)
        assert tot[1] == (0 if tot[0] == n else _capi.DECODE_RANGE_END), (st.name, first, n, tot)


def test_every_expected_slot_is_the_slice_of_the_samples_written():
    rb, names = rcases.corpus()
    want = rmodel.expected_batch(rb)
    slices_of_ground_truth(rb, want)
    slices_of_ground_truth(rcases.many_on_one(), rmodel.expected_batch(rcases.many_on_one()))
    # seek points: the frame starts the model reports are the ones the streams were written with
    for (s, first, n), (_, tot) in zip(rb.ranges, want):
        st = rb.streams[s]
        off, pos = cases.offsets_of(st), rcases.starts_of(st)
        if first >= pos[-1]:
            assert tot[2:] == [len(st.data), int(pos[-1])]
        else:
            j = int(np.searchsorted(pos, first, side="right")) - 1
            assert tot[2:] == [int(off[j]), int(pos[j])], (st.name, first, tot)


def test_the_corpus_holds_the_shapes_it_claims():
    rb, names = rcases.corpus()
    want = rmodel.expected_batch(rb)
    kinds = {k for _, k in names}
    assert {"inside one frame", "exactly one frame", "three frames, partial ends", "first sample", "nothing asked",
            "last sample", "past the end", "begins at the end", "begins beyond the end", "ends at the end",
            "empty: from 0"} <= kinds
    streams = {s for s, _ in names}
    assert {"mono 16 tail", "stereo 16 tags", "variable stereo", "variable mono", "mono lpc32", "stereo mid/side",
            "stereo left/side", "stereo right/side", "empty", "mono 8 wide"} <= streams
    assert {s.channels for s in rb.streams} == {1, 2, 3, 8} and {s.bps for s in rb.streams} == {8, 12, 16, 20, 24}
    assert any(s.width > (s.bps + 7) // 8 for s in rb.streams)
    by = {(s, k): i for i, (s, k) in enumerate(names)}
    tail = rb.streams[0]
    assert tail.frame_sizes[-1][1] == 17 and rb.ranges[by[("mono 16 tail", "last sample")]][1:] == (5 * 256 + 16, 1)
    i = by[("stereo 16 tags", "inside one frame")]
    assert rb.ranges[i][1:] == (192 + 3, 192 - 8) and want[i][1][:2] == [184, 0]
    i = by[("stereo 16 tags", "past the end")]
    assert want[i][1][:2] == [10, _capi.DECODE_RANGE_END] and rb.ranges[i][2] == 25
    i = by[("stereo 16 tags", "begins at the end")]
    assert want[i][1] == [0, _capi.DECODE_RANGE_END, len(rb.streams[1].data), 8 * 192 + 40]
    i = by[("stereo 16 tags", "ends at the end")]
    assert want[i][1][:2] == [13, 0]
    i = by[("stereo 16 tags", "nothing asked at the end")]
    assert want[i][1][:2] == [0, 0]
    assert want[by[("empty", "empty: from 0")]][1] == [0, _capi.DECODE_RANGE_END, 0, 0]
    assert want[by[("empty", "empty: nothing asked")]][1] == [0, 0, 0, 0]
    # slots at odd byte offsets and at offsets of 2 mod 4, with FILL in front of every one
    assert any(o % 2 for o in rb.slot_offsets) and any(o % 4 == 2 for o in rb.slot_offsets)
    spans = sorted(zip(rb.slot_offsets, rb.slot_bytes))
    assert all(a + n < b for (a, n), (b, _) in zip(spans, spans[1:]))
    # every stereo tag with an odd skip
    for name in ("stereo 16 tags", "stereo mid/side", "stereo left/side", "stereo right/side"):
        s, first, n = rb.ranges[by[(name, "inside one frame")]]
        assert (first - int(rcases.starts_of(rb.streams[s])[1])) % 2 == 1
    many = rcases.many_on_one()
    on_one = [r for r in many.ranges if r[0] == 1]
    assert len(on_one) == 33 and on_one[30] == on_one[31] == on_one[32]
    assert all(a[1] > b[1] for a, b in zip(on_one[:30], on_one[1:30]))          # descending
    assert any(a[1] < b[1] + b[2] for a, b in zip(on_one[:30], on_one[1:30]))   # overlapping
    assert any(len(many.streams[r[0]].data) == 0 for r in many.ranges)


def test_spans_that_start_at_a_seek_point_give_the_bytes_of_the_whole_stream():
    for s in (cases.mixed()[1], cases.mixed()[8], cases.mixed()[0]):
        pos = rcases.starts_of(s)
        whole = rmodel.truth(s)
        for k in (1, len(s.frame_sizes) - 1):
            part = rmodel.truth(rcases.span_from(s, k))
            first, n = int(pos[k]) + 7, 50
            a, ta = whole.expected(first, n)
            b, tb = part.expected(first - int(pos[k]), n)
            assert np.array_equal(a, b) and ta[:2] == tb[:2], (s.name, k)
            # the seek point one call returns, fed to a second
            again = rmodel.truth(cases.Stream("again", s.data[ta[2]:], s.channels, s.bps, s.mbs, None, s.width))
            c, tc = again.expected(first - ta[3], n)
            assert np.array_equal(a, c) and tc[:2] == ta[:2], (s.name, k)


def test_damaged_streams_stop_where_the_corpus_says():
    rb, info = rcases.damaged()
    want = rmodel.expected_batch(rb)
    _, base = cases.stops()
    for name, i, D, why in info:
        mine = [(r, w) for r, w in zip(rb.ranges, want) if r[0] == i]
        (before, wb), (across, wa), (behind, wh) = mine
        assert wb[1][:2] == [before[2], 0], name                                  # complete
        assert wa[1][:2] == [min(10, D), why], name                               # a prefix and the stream's reason
        assert wh[1][:2] == [0, why] and wh[1][3] == D, name                      # nothing, the seek point where it stopped
        truth = rb.streams[i].pcm if rb.streams[i].pcm is not None else base.pcm
        if name != "leading garbage":
            fb = rb.streams[i].channels * rb.streams[i].width
            assert np.array_equal(wb[0], truth[before[1] * fb:(before[1] + before[2]) * fb]), name
            assert np.array_equal(wa[0], truth[across[1] * fb:D * fb]), name
    rg = rcases.with_garbage()
    slices_of_ground_truth(rg, rmodel.expected_batch(rg))


def test_stream_ranges_core_equals_brute_force_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "stream_ranges_core_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-static-libasan",
                           "-static-libubsan", "-I", INCLUDE, "-I", CSRC,
                           os.path.join(ROOT, "tests", "host", "stream_ranges_core_test.cpp"), "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "stream_ranges_core OK" in p.stdout, p.stdout[-2000:] + p.stderr[-2000:]
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr


def test_the_range_descriptor_is_32_bytes_with_the_same_fields_everywhere(tmp_path):
    names = list(_capi.RANGE_DESC_DTYPE.names)
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "flacenc_hip.h"\nint main(void) {\n'
                   '  printf("%zu", sizeof(flacenc_hip_range_desc));\n'
                   + "".join('  printf(" %%zu", offsetof(flacenc_hip_range_desc, %s));\n' % n for n in names)
                   + '  printf(" %u", FLACENC_HIP_DECODE_RANGE_END);\n  return 0;\n}\n')
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I", INCLUDE, str(src), "-o", exe])
    got = [int(v) for v in subprocess.check_output([exe], text=True).split()]
    assert got == [32, 0, 8, 16, 24, 28, 1024]
    dt = _capi.RANGE_DESC_DTYPE
    assert dt.itemsize == 32 and [dt.fields[n][1] for n in names] == got[1:6]
    assert [dt.fields[n][0].itemsize for n in names] == [8, 8, 8, 4, 4]
    assert _capi.DECODE_RANGE_END == 1024
    rust = open(os.path.join(ROOT, "rust", "flacenc_hip.rs")).read()
    m = re.search(r"#\[repr\(C\)\]\s*#\[derive\([^)]*\)\]\s*pub struct RangeDesc \{(.*?)\n\}", rust, flags=re.S)
    assert m, "no #[repr(C)] RangeDesc"
    fields = re.findall(r"pub (\w+):\s*(\w+),", m.group(1))
    assert fields == [(n, "u64" if dt.fields[n][0].itemsize == 8 else "u32") for n in names]
    assert re.search(r"pub const DECODE_RANGE_END: u32 = 1024;", rust)
    header = open(os.path.join(INCLUDE, "flacenc_hip.h")).read()
    body = re.search(r"struct flacenc_hip_range_desc \{(.*?)\};", header, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(\w+)\s+(\w+);", body) == [("uint64_t" if t == "u64" else "uint32_t", n) for n, t in fields]
    assert "typedef struct flacenc_hip_range_desc flacenc_hip_range_desc;" in header


def test_header_bindings_and_library_agree_on_the_export():
    name = "flacenc_hip_decode_ranges"
    header = open(os.path.join(INCLUDE, "flacenc_hip.h")).read()
    assert re.search(r"\bint %s\s*\(" % name, header)
    assert re.search(r"#define FLACENC_HIP_ABI_VERSION\s+6\b", header) and _capi.ABI_VERSION == 6
    assert name in _capi.EXPORTED_SYMBOLS and "%s_async" % name not in _capi.EXPORTED_SYMBOLS
    assert "flacenc_hip_debug_last_decode_ranges_plan" in _capi.DEBUG_SYMBOLS
    assert "flacenc_hip_debug_last_decode_ranges_plan" in open(os.path.join(CSRC, "flacenc_hip_debug.h")).read()
    assert "flacenc_hip_*;" in open(os.path.join(CSRC, "exports.map")).read()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _capi.LIB_PATH], text=True)
    assert re.search(r"\bT %s$" % name, out, flags=re.M)
    assert "debug_last_decode_ranges_plan" not in out
    assert re.search(r"pub fn %s\(" % name, open(os.path.join(ROOT, "rust", "flacenc_hip.rs")).read())
    assert "decode_ranges(" in open(os.path.join(ROOT, "flacenc_rs_amd", "host", "flacenc.hpp")).read()
    assert _capi.load().flacenc_hip_abi_version() == 6


def test_the_seektable_helper_round_trips_and_points_at_frames():
    import flac_metadata as fm
    points = [(0, 0, 4096), (44100 * 3 + 17, 1 << 33, 1152), (fm.PLACEHOLDER, 0, 0), ((1 << 36) - 1, (1 << 40) + 5, 16)]
    block = fm.seektable_block(points, last=True)
    assert block[0] == 0x80 | 3 and int.from_bytes(block[1:4], "big") == 18 * len(points) == len(block) - 4
    assert fm.parse_seektable(block[4:]) == points
    assert fm.seektable_block(points, last=False)[0] == 3
    assert fm.last_point_at_or_before(points, 44100 * 3 + 16) == (0, 0, 4096)
    assert fm.last_point_at_or_before(points, 44100 * 3 + 17) == points[1]
    assert fm.last_point_at_or_before(points, 1 << 35) == points[1]          # the placeholder is skipped
    assert fm.last_point_at_or_before(None, 99) == (0, 0, 0)
    # against a corpus stream: every point is a frame of the stream, at the offset and position it was written at
    for s, every in ((cases.mixed()[8], 300), (cases.mixed()[0], 256), (cases.mixed()[12], 5000), (cases.mixed()[0], 1)):
        off, pos = cases.offsets_of(s), rcases.starts_of(s)
        pts = fm.seek_points([b for b, _ in s.frame_sizes], [n for _, n in s.frame_sizes], every)
        frames = {(int(p), int(o), n) for p, o, (_, n) in zip(pos, off, s.frame_sizes)}
        assert pts[0][:2] == (0, 0) and set(pts) <= frames and pts == sorted(set(pts)), s.name
        for k in range(0, int(pos[-1]), every):   # sample k * every lies in the frame of the last point at or before it
            p = fm.last_point_at_or_before(pts, k)
            assert p[0] <= k < p[0] + p[2], (s.name, every, k)
        # a file: STREAMINFO, the SEEKTABLE, the frames; read back by the shared reader
        info = bytes([0]) + (34).to_bytes(3, "big") + bytes(10) + ((44100 << 44) | (1 << 41) | (15 << 36)).to_bytes(8, "big") + bytes(16)
        data = b"fLaC" + info + fm.seektable_block(pts) + s.data.tobytes()
        got_info, got_pts, first = fm.read_blocks(data)
        assert got_pts == pts and data[first:] == s.data.tobytes() and got_info["channels"] == 2
        for p in pts:
            assert data[first + p[1]] == 0xFF and data[first + p[1] + 1] & 0xFE == 0xF8   # a frame's sync code
    import decode_flac
    assert decode_flac.read_metadata(data) == (got_info, first)
