"""flacenc_hip_decode_ranges_planar without a GPU: the call and its two constants are the same in the C header, the numpy
binding, the Rust binding and the library; csrc/stream_planar_core.h (slot, element address, head / body / tail split,
zero interval, value rule, table check) equals brute force under the sanitizers, as a stand-alone program; and the
expectation builder of the GPU tests (tests/planar_model.py) reproduces the samples the corpus streams were written from
and the ends of the 8-, 16- and 24-bit ranges exactly."""
import ctypes
import os
import re
import subprocess

import numpy as np

import planar_model as pmodel
import ranges_cases as rcases
import ranges_model as rmodel
import streams_cases as cases
from flacenc_rs_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "flacenc_rs_amd", "csrc")
INCLUDE = os.path.join(ROOT, "include")
NAME = "flacenc_hip_decode_ranges_planar"


def test_header_bindings_and_library_agree_on_the_export():
    header = open(os.path.join(INCLUDE, "flacenc_hip.h")).read()
    m = re.search(r"\bint %s\s*\((.*?)\);" % NAME, header, flags=re.S)
    assert m, "not declared"
    args = [a.strip() for a in re.sub(r"\s+", " ", m.group(1)).split(",")]
    assert args == ["flacenc_hip_handle* h", "const uint8_t* bytes", "uint64_t n_bytes", "const void* streams",
                    "size_t n_streams", "const void* ranges", "size_t n_ranges", "size_t max_frames", "void* out",
                    "uint64_t out_bytes", "uint32_t sample_format", "uint64_t* totals", "uint64_t call_totals[2]",
                    "int memory_kind"]
    assert re.search(r"#define FLACENC_HIP_SAMPLE_I32\s+0u\b", header) and _capi.SAMPLE_I32 == 0
    assert re.search(r"#define FLACENC_HIP_SAMPLE_F32\s+1u\b", header) and _capi.SAMPLE_F32 == 1
    assert re.search(r"#define FLACENC_HIP_ABI_VERSION\s+6\b", header) and _capi.ABI_VERSION == 6
    assert NAME in _capi.EXPORTED_SYMBOLS and NAME + "_async" not in _capi.EXPORTED_SYMBOLS
    assert "no stream-taking form" in re.sub(r"\s*\n \*\s*", " ", header[:m.start()][-6000:])
    assert "flacenc_hip_decode_ranges_planar below" in header   # decode_ranges' own comment points here
    assert "flacenc_hip_*;" in open(os.path.join(CSRC, "exports.map")).read()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _capi.LIB_PATH], text=True)
    assert re.search(r"\bT %s$" % NAME, out, flags=re.M)
    rust = open(os.path.join(ROOT, "rust", "flacenc_hip.rs")).read()
    r = re.search(r"pub fn %s\((.*?)\) -> c_int;" % NAME, rust, flags=re.S)
    assert r and "sample_format: u32" in r.group(1) and "out: *mut c_void" in r.group(1)
    assert re.search(r"pub const SAMPLE_I32: u32 = 0;", rust) and re.search(r"pub const SAMPLE_F32: u32 = 1;", rust)
    lib = _capi.load()
    assert lib.flacenc_hip_abi_version() == 6
    fn = getattr(lib, NAME)
    assert len(fn.argtypes) == 14 and fn.argtypes[10] is ctypes.c_uint32 and fn.restype is ctypes.c_int
    assert hasattr(_capi.Handle, "decode_ranges_planar") and hasattr(_capi.Handle, "decode_ranges_planar_device")


def test_a_null_handle_is_a_bad_argument():
    lib = _capi.load()
    buf = np.zeros(64, np.uint8)
    table = np.zeros(1, _capi.STREAM_DESC_DTYPE)
    rtable = np.zeros(1, _capi.RANGE_DESC_DTYPE)
    totals, call = np.full(4, 7, np.uint64), np.full(2, 7, np.uint64)
    rc = getattr(lib, NAME)(None, buf.ctypes.data, 64, table.ctypes.data, 1, rtable.ctypes.data, 1, 16, buf.ctypes.data, 64,
                            _capi.SAMPLE_F32, totals.ctypes.data, call.ctypes.data, _capi.MEM_HOST)
    assert rc == _capi.ERR_BAD_ARGUMENT and (totals == 7).all() and (call == 7).all() and not buf.any()


def test_stream_planar_core_equals_brute_force_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "stream_planar_core_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-static-libasan",
                           "-static-libubsan", "-I", INCLUDE, "-I", CSRC,
                           os.path.join(ROOT, "tests", "host", "stream_planar_core_test.cpp"), "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "stream_planar_core OK" in p.stdout, p.stdout[-2000:] + p.stderr[-2000:]
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr


def written_values(st):
    """int64 [channels, samples]: what the stream was written from, read back from its packed ground truth."""
    return pmodel.values_of(st.pcm, st.channels, st.width).astype(np.int64)


def test_the_builder_reproduces_the_samples_the_corpus_was_written_from():
    for rb in (rcases.corpus()[0], rcases.many_on_one()):
        want = rmodel.expected_batch(rb)
        for fmt in (_capi.SAMPLE_I32, _capi.SAMPLE_F32):
            slots = pmodel.expected_slots(rb, want, fmt)
            for (s, first, n), (slot, tot) in zip(rb.ranges, slots):
                st = rb.streams[s]
                w = tot[0]
                assert slot.shape == (st.channels, n) and slot.dtype == np.uint32 and not slot[:, w:].any()
                x = written_values(st)[:, first:first + w]
                assert x.shape[1] == w and (np.abs(x) <= 1 << (st.bps - 1)).all()
                if fmt == _capi.SAMPLE_I32:
                    assert np.array_equal(slot[:, :w].view(np.int32), x)
                else:
                    f = slot[:, :w].view(np.float32)
                    # exact: the element times 2^(bits - 1) is the sample, in float64 as in float32
                    assert np.array_equal(f.astype(np.float64) * 2.0 ** (st.bps - 1), x.astype(np.float64))
                    assert ((f >= -1) & (f < 1)).all()
                    assert not (slot[:, :w][x == 0]).any()   # +0.0f, never -0.0f
    # the sign extension, on samples whose container is wider than their depth and on ones whose is not
    assert np.array_equal(pmodel.values_of(np.array([0xFF, 0x7F, 0x80, 0x00], np.uint8), 2, 1)[:, 0], [-1, 127])
    assert np.array_equal(pmodel.values_of(np.array([0, 0, 0x80, 0xFF, 0xFF, 0x7F], np.uint8), 1, 3)[0], [-(1 << 23), (1 << 23) - 1])
    # de-interleaving: channel c of sample i is value i * channels + c
    v = pmodel.values_of(cases.pack(np.arange(12).reshape(3, 4) - 5, 2), 3, 2)
    assert np.array_equal(v, np.arange(12).reshape(3, 4) - 5)


def test_the_ends_of_the_8_16_and_24_bit_ranges():
    for bps in (8, 16, 24):
        lo, hi = -(1 << (bps - 1)), (1 << (bps - 1)) - 1
        width = bps // 8
        packed = cases.pack(np.array([[lo, hi, 0, -1, 1]]), width)
        for fmt in (_capi.SAMPLE_I32, _capi.SAMPLE_F32):
            slot = pmodel.slot_of(packed, 1, width, bps, 8, fmt)
            assert slot.shape == (1, 8) and not slot[0, 5:].any()
            if fmt == _capi.SAMPLE_I32:
                assert slot[0, :5].view(np.int32).tolist() == [lo, hi, 0, -1, 1]
                continue
            f = slot[0].view(np.float32)
            assert f[0] == np.float32(-1.0) and slot[0, 0] == 0xBF800000
            assert f[1] == np.float32(1.0) - np.float32(2.0 ** -(bps - 1)) and float(f[1]) == 1 - 2.0 ** -(bps - 1)
            assert slot[0, 2] == 0 and float(f[3]) == -2.0 ** -(bps - 1) and float(f[4]) == 2.0 ** -(bps - 1)


def test_the_odd_streams_decode_whole_and_some_values_exceed_their_depth():
    streams = pmodel.odd_streams()
    names = [s.name for s in streams]
    assert any(n.startswith("corner24") for n in names) and any(n.startswith("corner25") for n in names)
    assert any(n.startswith("side tag 8 bps 24") for n in names) and "wrapping sum" in names
    beyond = 0
    for s in streams:
        n = s.frame_sizes[0][1]
        data, tot = rmodel.truth(s).expected(0, n)
        assert tot[:2] == [n, 0], s.name          # one frame that decodes
        v = pmodel.values_of(data, s.channels, 4).astype(np.int64)
        beyond += bool((np.abs(v) > 1 << (s.bps - 1)).any())
        # F32 of such values: rounded once on the way to float, then scaled exactly
        f = pmodel.elements_of(v.astype(np.int32), s.bps, _capi.SAMPLE_F32).view(np.float32)
        assert np.array_equal(f.astype(np.float64), v.astype(np.int32).astype(np.float32).astype(np.float64) * 2.0 ** -(s.bps - 1))
    assert beyond >= 3
    wrap = streams[names.index("wrapping sum")]
    v = pmodel.values_of(rmodel.truth(wrap).expected(0, 40)[0], 1, 4)[0].astype(np.int64)
    true = 30000 + np.arange(40, dtype=np.int64) * ((1 << 28) + 12345)
    assert np.array_equal(v, ((true + (1 << 31)) % (1 << 32)) - (1 << 31)) and (v != true).any()
