"""flacenc_hip_decode_streams without a GPU: the model the GPU tests compare against (tests/streams_model.py) gives the
samples every stream of the corpus was written from; the corpus' boundary claims hold on the host build of the decoder
core; csrc/stream_batch_core.h equals brute force under the sanitizers (a stand-alone program); the garbage streams go
through the existing stand-alone sanitized driver of the core; and the descriptor's layout is the same in the C header,
the numpy dtype and the Rust binding."""
import os
import re
import subprocess

import numpy as np
import pytest

import decode_cases
import streams_cases as cases
import streams_model as model
from flacenc_rs_amd import _capi, decode_cpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "flacenc_rs_amd", "csrc")
INCLUDE = os.path.join(ROOT, "include")


def whole(s, capacity=None):
    return model.expected(s.data, s.channels, s.bps, s.mbs, s.width, len(s.pcm) if capacity is None else capacity)


def test_the_model_gives_the_samples_the_streams_were_written_from():
    seen_channels, seen_bits = set(), set()
    for s in cases.mixed():
        pcm, totals = whole(s)
        assert np.array_equal(pcm, s.pcm), s.name
        samples = len(s.pcm) // (s.channels * s.width)
        assert totals == [len(s.frame_sizes), samples, len(s.data), 0], s.name
        assert [n for _, n in s.frame_sizes] == [n for _, n in s.frame_sizes if 16 <= n <= 1152]
        seen_channels.add(s.channels)
        seen_bits.add(s.bps)
    assert seen_channels == {1, 2, 3, 8} and seen_bits == {8, 12, 16, 20, 24}
    assert any(len(s.data) == 0 for s in cases.mixed()) and any(len(s.frame_sizes) == 1 for s in cases.mixed())
    assert any(s.frame_sizes and s.frame_sizes[-1][1] < 64 for s in cases.mixed())


def test_the_stops_stop_where_the_corpus_says():
    stops, base = cases.stops()
    off = cases.offsets_of(base)
    for name, (s, frames, why) in stops.items():
        pcm, totals = model.expected(s.data, s.channels, s.bps, s.mbs, s.width, 1 << 30)
        assert totals[0] == frames and totals[3] == why, (name, totals)
        if name == "leading garbage":
            assert totals[2] == 0
        elif name != "block above max":
            assert totals[2] == off[frames] and np.array_equal(pcm, base.pcm[:len(pcm)]), name
    # a slot that ends inside frame k; the second call on what is left gives the rest
    k = 3
    room = sum(n for _, n in base.frame_sizes[:k]) * 4 + 100
    first, t1 = whole(base, capacity=room)
    assert t1 == [k, k * 192, int(off[k]), _capi.DECODE_NO_ROOM]
    rest, t2 = model.expected(base.data[t1[2]:], 2, 16, base.mbs, 2, len(base.pcm))
    assert t2[3] == 0 and np.array_equal(np.concatenate([first, rest]), base.pcm)


def test_a_stream_cut_in_two_inside_a_frame():
    """Whole it decodes fully; the first part gives the frames before the cut and CHAIN at the cut frame's start; the
    second part gives no frame and CHAIN at 0 -- so laid next to each other as two streams they must not chain."""
    s = cases.mixed()[1]
    off = cases.offsets_of(s)
    k = 4
    cut = int(off[k]) + (int(off[k + 1]) - int(off[k])) // 2
    assert whole(s)[1][3] == 0
    pcm, totals = model.expected(s.data[:cut], s.channels, s.bps, s.mbs, s.width, len(s.pcm))
    assert totals == [k, k * 192, int(off[k]), _capi.DECODE_CHAIN] and np.array_equal(pcm, s.pcm[:len(pcm)])
    pcm, totals = model.expected(s.data[cut:], s.channels, s.bps, s.mbs, s.width, len(s.pcm))
    assert totals == [0, 0, 0, _capi.DECODE_CHAIN] and len(pcm) == 0


def test_two_streams_end_to_end_are_one_chain_for_the_single_stream_index():
    """What a boundary-blind batch would do: the existing index, given both as one buffer, walks a + b frames."""
    a, b = cases.mixed()[0], cases.mixed()[20]
    assert (a.channels, a.bps) == (b.channels, b.bps)
    both = np.concatenate([a.data, b.data])
    off, ln, ok = model.decoder().index_frames(both, a.channels, a.bps, len(both) // 9 + 1)
    assert ok and len(off) == len(a.frame_sizes) + len(b.frame_sizes)


def test_a_gap_with_a_copied_frame_holds_a_candidate():
    s = cases.mixed()[0]
    frame = s.data[:s.frame_sizes[0][0]]
    gap = np.concatenate([np.full(7, cases.GAP, np.uint8), frame, np.full(5, cases.GAP, np.uint8)])
    assert decode_cases.is_candidate(bytes(gap), 7, s.channels, s.bps)
    assert decode_cases.count_candidates(bytes(gap), s.channels, s.bps) >= 1


def test_stream_batch_core_equals_brute_force_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "stream_batch_core_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-static-libasan",
                           "-static-libubsan", "-I", INCLUDE, "-I", CSRC,
                           os.path.join(ROOT, "tests", "host", "stream_batch_core_test.cpp"), "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "stream_batch_core OK" in p.stdout, p.stdout[-2000:] + p.stderr[-2000:]
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr


def test_garbage_streams_pass_the_sanitized_driver_of_the_core(tmp_path):
    """Stream by stream, each as one span of its own -- the bounds the batch gives the core -- before any GPU run."""
    exe = decode_cpu.build_sanitized_driver()
    stops, _ = cases.stops()
    for s in cases.garbage() + [v[0] for v in stops.values()]:
        st, _, _, ioff, _, _ = decode_cpu.run_sanitized(exe, s.data.tobytes(), [0], [len(s.data)], s.channels, s.bps,
                                                        s.mbs, str(tmp_path))
        pcm, totals = model.expected(s.data, s.channels, s.bps, s.mbs, s.width, 4096)
        assert len(ioff) >= totals[0], s.name


def test_the_descriptor_is_48_bytes_with_the_same_fields_everywhere(tmp_path):
    names = list(_capi.STREAM_DESC_DTYPE.names)
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "flacenc_hip.h"\nint main(void) {\n'
                   '  printf("%zu", sizeof(flacenc_hip_stream_desc));\n'
                   + "".join('  printf(" %%zu", offsetof(flacenc_hip_stream_desc, %s));\n' % n for n in names)
                   + "  return 0;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I", INCLUDE, str(src), "-o", exe])
    got = [int(v) for v in subprocess.check_output([exe], text=True).split()]
    assert got == [48, 0, 8, 16, 24, 32, 36, 40, 44]
    dt = _capi.STREAM_DESC_DTYPE
    assert dt.itemsize == 48 and [dt.fields[n][1] for n in names] == got[1:]
    assert [dt.fields[n][0].itemsize for n in names] == [8, 8, 8, 8, 4, 4, 4, 4]
    rust = open(os.path.join(ROOT, "rust", "flacenc_hip.rs")).read()
    m = re.search(r"#\[repr\(C\)\]\s*#\[derive\([^)]*\)\]\s*pub struct StreamDesc \{(.*?)\n\}", rust, flags=re.S)
    assert m, "no #[repr(C)] StreamDesc"
    fields = re.findall(r"pub (\w+):\s*(\w+),", m.group(1))
    assert fields == [(n, "u64" if dt.fields[n][0].itemsize == 8 else "u32") for n in names]
    header = open(os.path.join(INCLUDE, "flacenc_hip.h")).read()
    body = re.search(r"struct flacenc_hip_stream_desc \{(.*?)\};", header, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(\w+)\s+(\w+);", body) == [("uint64_t" if t == "u64" else "uint32_t", n) for n, t in fields]


def test_header_bindings_and_library_agree_on_the_export():
    name = "flacenc_hip_decode_streams"
    header = open(os.path.join(INCLUDE, "flacenc_hip.h")).read()
    assert re.search(r"\bint %s\s*\(" % name, header)
    assert name in _capi.EXPORTED_SYMBOLS and "%s_async" % name not in _capi.EXPORTED_SYMBOLS
    assert "flacenc_hip_debug_last_decode_streams_plan" in _capi.DEBUG_SYMBOLS
    assert "flacenc_hip_*;" in open(os.path.join(CSRC, "exports.map")).read()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _capi.LIB_PATH], text=True)
    assert re.search(r"\bT %s$" % name, out, flags=re.M)
    assert "debug_last_decode_streams_plan" not in out
    assert re.search(r"pub fn %s\(" % name, open(os.path.join(ROOT, "rust", "flacenc_hip.rs")).read())
    assert "decode_streams(" in open(os.path.join(ROOT, "flacenc_rs_amd", "host", "flacenc.hpp")).read()
    assert _capi.load().flacenc_hip_abi_version() == 6
