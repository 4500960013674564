"""flacenc_hip_encode_streams_planar without a GPU: the call is the same in the C header, the numpy binding, the Rust
binding and the library; the numpy model of the quantiser (tests/planar_encode_model.py), which the GPU tests expect
from, equals an independent statement in exact rational arithmetic on every tie, edge and special value and inverts the
decoder's float rule; the model's layout builder puts rows where the header says; and
csrc/stream_planar_encode_core.h equals brute force under the sanitizers, as a stand-alone program."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import planar_encode_model as pem
from flacenc_rs_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "flacenc_rs_amd", "csrc")
INCLUDE = os.path.join(ROOT, "include")
NAME = "flacenc_hip_encode_streams_planar"
DEPTHS = (8, 16, 20, 24)


def test_header_bindings_and_library_agree_on_the_export():
    header = open(os.path.join(INCLUDE, "flacenc_hip.h")).read()
    m = re.search(r"\bint %s\s*\((.*?)\);" % NAME, header, flags=re.S)
    assert m, "not declared"
    args = [a.strip() for a in re.sub(r"\s+", " ", m.group(1)).split(",")]
    assert args == ["flacenc_hip_handle* h", "const flacenc_hip_frame_config* cfg", "const void* samples",
                    "uint64_t samples_bytes", "uint32_t sample_format", "uint64_t row_pitch", "const void* streams",
                    "size_t n_streams", "uint32_t block_size", "uint8_t* out", "uint64_t out_bytes",
                    "uint32_t* frame_lengths", "size_t max_frames", "uint64_t* totals", "uint64_t call_totals[2]",
                    "uint8_t* digests", "uint64_t* clipped", "int memory_kind"]
    assert re.search(r"#define FLACENC_HIP_ABI_VERSION\s+6\b", header) and _capi.ABI_VERSION == 6
    assert NAME in _capi.EXPORTED_SYMBOLS and NAME + "_async" not in _capi.EXPORTED_SYMBOLS
    out = subprocess.check_output(["nm", "-D", "--defined-only", _capi.LIB_PATH], text=True)
    assert re.search(r"\bT %s$" % NAME, out, flags=re.M)
    assert "flacenc_hip_debug" not in out                       # the product library's exports stay the C ABI
    hooks = subprocess.check_output(["nm", "-D", "--defined-only", _capi.HOOKS_LIB_PATH], text=True)
    assert re.search(r"\bT flacenc_hip_debug_set_planar_fill_form$", hooks, flags=re.M)
    rust = open(os.path.join(ROOT, "rust", "flacenc_hip.rs")).read()
    r = re.search(r"pub fn %s\((.*?)\) -> c_int;" % NAME, rust, flags=re.S)
    assert r
    rargs = [a.strip() for a in re.sub(r"\s+", " ", r.group(1)).strip().rstrip(",").split(",")]
    assert [a.split(":")[0] for a in rargs] == [a.split()[-1].replace("call_totals[2]", "call_totals") for a in args]
    assert "sample_format: u32" in rargs and "row_pitch: u64" in rargs and "clipped: *mut u64" in rargs
    fn = getattr(_capi.load(), NAME)
    assert len(fn.argtypes) == 18 and fn.argtypes[4] is ctypes.c_uint32 and fn.argtypes[5] is ctypes.c_uint64
    assert fn.restype is ctypes.c_int
    assert hasattr(_capi.Handle, "encode_streams_planar") and hasattr(_capi.Handle, "encode_streams_planar_device")
    from flacenc_rs_amd import crops
    assert "encode_crops" in crops.__all__ and "decode_crops" in crops.__all__


def test_a_null_handle_is_a_bad_argument_and_writes_nothing():
    lib = _capi.load()
    samples = np.zeros(64, np.float32)
    out = np.zeros(256, np.uint8)
    table = np.zeros(1, _capi.PCM_STREAM_DESC_DTYPE)
    table[0] = (0, 64, 0, 256, 1, 16, 2, 44100)
    lens, totals, call = np.full(4, 7, np.uint32), np.full(4, 7, np.uint64), np.full(2, 7, np.uint64)
    dig, clip = np.full(16, 7, np.uint8), np.full(1, 7, np.uint64)
    cfg = _capi.make_frame_config(_capi.make_config(lpc_order=8))
    rc = getattr(lib, NAME)(None, ctypes.byref(cfg), samples.ctypes.data, 256, _capi.SAMPLE_F32, 0, table.ctypes.data, 1, 64,
                            out.ctypes.data, 256, lens.ctypes.data, 4, totals.ctypes.data, call.ctypes.data,
                            dig.ctypes.data, clip.ctypes.data, _capi.MEM_HOST)
    assert rc == _capi.ERR_BAD_ARGUMENT
    assert (lens == 7).all() and (totals == 7).all() and (call == 7).all() and (dig == 7).all() and (clip == 7).all()
    assert not out.any()


def test_stream_planar_encode_core_equals_brute_force_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "stream_planar_encode_core_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-ffp-contract=off",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           "-static-libasan", "-static-libubsan", "-I", INCLUDE, "-I", CSRC,
                           os.path.join(ROOT, "tests", "host", "stream_planar_encode_core_test.cpp"), "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "stream_planar_encode_core OK" in p.stdout, p.stdout[-2000:] + p.stderr[-2000:]
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr


@pytest.mark.parametrize("bits", DEPTHS)
def test_the_model_of_q_equals_the_exact_statement_on_ties_edges_and_specials(bits):
    x = pem.float_cases(bits)
    got, clipped = pem.q(x, bits)
    lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
    for xi, g, c in zip(x, got, clipped):
        want = pem.q_exact(float(xi), bits)
        assert (int(g), bool(c)) == want, (float(xi), hex(int(np.float32(xi).view(np.uint32))))
    assert got.min() == lo and got.max() == hi
    # what the cases must contain to mean anything
    u = x.view(np.uint32)
    nan = np.isnan(x)
    assert nan.sum() >= 5 and (got[nan] == 0).all() and clipped[nan].all()
    assert (nan & (u >> 31 == 1)).any() and (nan & (u >> 31 == 0)).any()
    assert (nan & ((u & 0x00400000) == 0)).any() and (nan & ((u & 0x00400000) != 0)).any()   # signalling, quiet
    assert np.isinf(x).sum() == 2 and clipped[np.isinf(x)].all()
    assert (u == 0x80000000).any() and (u == 0).any() and (u == 1).any() and (u == 0x807FFFFF).any()
    zeroish = (np.abs(x) < 2.0 ** -100)
    assert (got[zeroish] == 0).all() and not clipped[zeroish].any()
    # named values: ties go to even, +1.0 is one step beyond the top and clamps, -1.0 is the bottom and does not
    s = np.float32(2.0 ** -(bits - 1))
    named = np.array([0.5 * s, 1.5 * s, 2.5 * s, -0.5 * s, -1.5 * s, 1.0, -1.0, 1.0 - s, (hi + 0.5) * s, (lo - 0.5) * s],
                     np.float32)
    g, c = pem.q(named, bits)
    # (hi + 0.5 is a tie towards the even hi + 1: clamps; lo - 0.5 is a tie towards the even lo: does not.  At 24 bits
    # hi + 0.5 is no float32: the cast rounds it to hi + 1 to the same end)
    assert g.tolist() == [0, 2, 2, 0, -2, hi, lo, hi, hi, lo]
    assert c.tolist() == [False] * 5 + [True, False, False, True, False]


@pytest.mark.parametrize("bits", DEPTHS)
def test_q_inverts_the_decoders_float_rule(bits):
    lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
    if bits <= 16:
        v = np.arange(lo, hi + 1, dtype=np.int32)
    else:
        v = np.unique(np.concatenate([np.arange(lo, hi + 1, 977, dtype=np.int64), [lo, lo + 1, -1, 0, 1, hi - 1, hi]])).astype(np.int32)
    got, clipped = pem.q(pem.unscale(v, bits), bits)
    assert np.array_equal(got, v) and not clipped.any()
    f = pem.unscale(v, bits)
    assert f.dtype == np.float32 and f.min() == -1.0 and f.max() < 1.0


def test_the_layout_builder_puts_rows_where_the_header_says():
    rng = np.random.default_rng(5)
    rows = [rng.integers(-100, 100, (c, n)).astype(np.int32) for c, n in ((1, 5), (2, 0), (3, 7), (2, 1), (8, 3), (1, 4))]
    descs = [(0, 0, 16, 2, 44100)] * len(rows)
    for pitch in (0, 10):
        lay = pem.layout(rows, descs, pitch, fill=0x7FFFFFFF)
        raw = lay.samples.view(np.uint32)
        assert pem.check_rows(lay.table, _capi.SAMPLE_I32, pitch, lay.samples.nbytes)
        assert not pem.check_rows(lay.table, _capi.SAMPLE_I32, pitch, lay.samples.nbytes - 4)   # the last element is the buffer's last
        assert not pem.check_rows(lay.table, 2, pitch, lay.samples.nbytes)
        seen = np.zeros(raw.size, bool)
        for i, (r, d) in enumerate(zip(rows, lay.table)):
            off, n = int(d["offset"]), int(d["total_samples"])
            assert off % 4 == 0 and off % 16 == (0, 4, 8, 12)[i % 4] and n == r.shape[1]
            for c in range(r.shape[0]):
                lo = off // 4 + c * (pitch or n)
                assert np.array_equal(lay.samples[lo:lo + n], r[c])
                seen[lo:lo + n] = True
        assert np.array_equal(seen, lay.elements) and (raw[~seen] == 0x7FFFFFFF).all() and (~seen).sum() >= 4 * len(rows)
    assert not pem.check_rows(pem.layout(rows, descs, 10).table, _capi.SAMPLE_I32, 6, 1 << 20)   # a pitch below a length
    bad = pem.layout(rows, descs, 0).table.copy()
    bad["offset"][0] += 2
    assert not pem.check_rows(bad, _capi.SAMPLE_I32, 0, 1 << 20)
    # packed PCM: the low `width` bytes, little-endian, channels interleaved
    assert pem.pack(np.array([[1, -2], [0x123456, -1]]), 3).tolist() == [1, 0, 0, 0x56, 0x34, 0x12, 0xFE, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF]
