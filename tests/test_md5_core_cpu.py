"""csrc/md5_core.h without a GPU: the arithmetic the device kernel of flacenc_hip_md5_spans shares with the host, run by a
stand-alone program (tests/host/md5_core_test.cpp) under the sanitizers and compared with hashlib -- the RFC 1321 test
suite, every length across the padding seams, every start alignment, each span in a heap buffer of exactly its size --
and once unsanitized on a span whose bit length needs more than 32 bits.  Then the two exports in the header, the
bindings and the product library, and the argument checks that need no device."""
import ctypes as C
import hashlib
import os
import re
import subprocess

import numpy as np
import pytest

from flacenc_rs_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "flacenc_rs_amd", "csrc")
INCLUDE = os.path.join(ROOT, "include")
SOURCE = os.path.join(ROOT, "tests", "host", "md5_core_test.cpp")
NAMES = ("flacenc_hip_md5_spans", "flacenc_hip_decode_streams_md5")

RFC_1321 = [
    (b"", "d41d8cd98f00b204e9800998ecf8427e"),
    (b"a", "0cc175b9c0f1b6a831c399e269772661"),
    (b"abc", "900150983cd24fb0d6963f7d28e17f72"),
    (b"message digest", "f96b697d7cb7938d525a2f31aaf161d0"),
    (b"abcdefghijklmnopqrstuvwxyz", "c3fcd3d76192e4007dfb496cca67e13b"),
    (b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789", "d174ab98d277d9f5a5611c2c9f419d9f"),
    (b"1234567890" * 8, "57edf4a22be3c955ac49da2e2107b67a"),
]


@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("md5_core") / "md5_core_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-static-libasan",
                           "-static-libubsan", "-I", INCLUDE, "-I", CSRC, SOURCE, "-o", exe])
    return exe


def digests_of(exe, data, spans, tmp_path):
    """spans: (offset, length, align) -> the program's hex digests, one per span; any sanitizer report fails."""
    (tmp_path / "data.bin").write_bytes(bytes(data))
    (tmp_path / "spans.txt").write_text("".join("%d %d %d\n" % s for s in spans))
    p = subprocess.run([exe, "spans", str(tmp_path / "data.bin"), str(tmp_path / "spans.txt")], capture_output=True,
                       text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-1000:] + p.stderr[-3000:]
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-3000:]
    got = p.stdout.split()
    assert len(got) == len(spans)
    return got


def test_the_rfc_1321_test_suite(sanitized, tmp_path):
    data = b"".join(m for m, _ in RFC_1321)
    spans, at = [], 0
    for m, _ in RFC_1321:
        spans.append((at, len(m), 0))
        at += len(m)
    got = digests_of(sanitized, data, spans, tmp_path)
    assert got == [want for _, want in RFC_1321]
    assert got == [hashlib.md5(m).hexdigest() for m, _ in RFC_1321]


def test_every_length_across_the_padding_seams_at_every_alignment(sanitized, tmp_path):
    """Lengths 0..200 (the seams 55 / 56 / 63 / 64 / 119 / 120 among them) of a fixed random buffer, each from starts at 8
    byte alignments, each in a heap buffer that ends with the span: an over-read is an AddressSanitizer report, and so
    is a read of the poisoned bytes in front of a misaligned start."""
    data = np.random.default_rng(0x3D5).integers(0, 256, 4096).astype(np.uint8).tobytes()
    spans = [(17 * align + n, n, align) for n in range(201) for align in range(8)]
    assert {55, 56, 63, 64, 119, 120} <= {n for _, n, _ in spans}
    got = digests_of(sanitized, data, spans, tmp_path)
    want = [hashlib.md5(data[o:o + n]).hexdigest() for o, n, _ in spans]
    assert got == want


def test_a_bit_length_above_32_bits(tmp_path):
    """One span of 2^29 + 3 bytes: 2^32 + 24 bits.  The unsanitized -O2 build of the same program, on bytes it generates
    itself; hashlib takes the same bytes in pieces."""
    exe = str(tmp_path / "md5_core_test_o2")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-I", INCLUDE, "-I", CSRC, SOURCE, "-o", exe])
    n = (1 << 29) + 3
    assert 8 * n > 0xFFFFFFFF
    h = hashlib.md5()
    golden = np.uint64(0x9E3779B97F4A7C15)
    step = 1 << 24
    for lo in range(0, n, step):
        i = np.arange(lo, min(n, lo + step), dtype=np.uint64)
        h.update(((i * golden) >> np.uint64(56)).astype(np.uint8).tobytes())
    got = subprocess.run([exe, "generated", str(n)], capture_output=True, text=True, timeout=300, check=True).stdout.split()
    assert got == [h.hexdigest()]


def test_the_span_check_never_forms_offset_plus_length(sanitized):
    def inside(n_bytes, *pairs):
        out = subprocess.run([sanitized, "inside", str(n_bytes)] + [str(v) for p in pairs for v in p], capture_output=True,
                             text=True, check=True)
        assert "runtime error" not in out.stderr
        return out.stdout.strip() == "inside"

    top = (1 << 64) - 1
    assert inside(100) and inside(100, (0, 100), (100, 0), (40, 60), (40, 60), (0, 0))
    assert not inside(100, (0, 101)) and not inside(100, (101, 0)) and not inside(100, (40, 61))
    assert not inside(100, (0, 10), (99, 2)) and not inside(0, (0, 1)) and inside(0, (0, 0))
    # offset + length wraps to a small number
    assert not inside(100, (50, top - 10)) and not inside(100, (top, 2)) and not inside(100, (top - 3, 4))
    assert not inside(top, (top, 1)) and inside(top, (top - 1, 1))


def test_header_bindings_and_library_agree_on_the_exports():
    header = open(os.path.join(INCLUDE, "flacenc_hip.h")).read()
    rust = open(os.path.join(ROOT, "rust", "flacenc_hip.rs")).read()
    hpp = open(os.path.join(ROOT, "flacenc_rs_amd", "host", "flacenc.hpp")).read()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _capi.LIB_PATH], text=True)
    lib = _capi.load()
    for name in NAMES:
        assert re.search(r"^int %s\(" % name, header, re.M), name
        assert "%s_async" % name not in header and "%s_async" % name not in _capi.EXPORTED_SYMBOLS
        assert name in _capi.EXPORTED_SYMBOLS and getattr(lib, name).argtypes, name
        assert re.search(r"\bT %s$" % name, out, flags=re.M), name
        assert re.search(r"pub fn %s\(" % name, rust), name
        assert name + "(" in hpp, name
    assert len(lib.flacenc_hip_decode_streams_md5.argtypes) == len(lib.flacenc_hip_decode_streams.argtypes) + 1
    for wrapper in ("md5_spans", "md5_spans_device", "decode_streams_md5", "decode_streams_md5_device"):
        assert hasattr(_capi.Handle, wrapper), wrapper
    assert "flacenc_hip_*;" in open(os.path.join(CSRC, "exports.map")).read()
    # additive: the ABI revision stays
    assert _capi.ABI_VERSION == 6 and lib.flacenc_hip_abi_version() == 6
    assert re.search(r"#define FLACENC_HIP_ABI_VERSION 6\b", header) and re.search(r"pub const ABI_VERSION: c_int = 6;", rust)


def test_arguments_are_refused_before_any_device_is_needed():
    """Without a handle there is nothing to run on: every call is BAD_ARGUMENT and writes nothing -- whatever else is wrong
    with it (null pointers, an unknown memory kind, a span past n_bytes, offset + length wrapping around 2^64).  The same
    table on a live handle is tests/test_gpu_md5_streams.py::test_arguments."""
    lib = _capi.load()
    data = np.arange(64, dtype=np.uint8)
    digests = np.full((2, 16), 0x5A, np.uint8)
    good = (np.array([0, 8], np.uint64), np.array([8, 56], np.uint64))
    past = (np.array([0, 8], np.uint64), np.array([8, 57], np.uint64))
    wraps = (np.array([0, (1 << 64) - 4], np.uint64), np.array([8, 8], np.uint64))
    for off, ln in (good, past, wraps):
        for kind in (_capi.MEM_HOST, _capi.MEM_DEVICE, 7):
            for d_ptr, o_ptr, l_ptr, b_ptr in ((digests.ctypes.data, off.ctypes.data, ln.ctypes.data, data.ctypes.data),
                                               (None, off.ctypes.data, ln.ctypes.data, data.ctypes.data),
                                               (digests.ctypes.data, None, ln.ctypes.data, data.ctypes.data),
                                               (digests.ctypes.data, off.ctypes.data, None, data.ctypes.data),
                                               (digests.ctypes.data, off.ctypes.data, ln.ctypes.data, None)):
                rc = lib.flacenc_hip_md5_spans(None, b_ptr, data.size, o_ptr, l_ptr, 2, d_ptr, kind)
                assert rc == _capi.ERR_BAD_ARGUMENT
    table = np.zeros(1, _capi.STREAM_DESC_DTYPE)
    table[0] = (0, 64, 0, 64, 1, 16, 4096, 2)
    out = np.full(64, 0xEE, np.uint8)
    totals = np.full(4, 0x77, np.uint64)
    call = np.full(2, 0x33, np.uint64)
    rc = lib.flacenc_hip_decode_streams_md5(None, data.ctypes.data, data.size, table.ctypes.data, 1, 8, out.ctypes.data,
                                            out.size, totals.ctypes.data, call.ctypes.data, _capi.MEM_HOST,
                                            digests.ctypes.data)
    assert rc == _capi.ERR_BAD_ARGUMENT
    assert (digests == 0x5A).all() and (out == 0xEE).all() and (totals == 0x77).all() and (call == 0x33).all()
