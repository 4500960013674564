"""flacenc_hip_set_max_bits_per_sample is declared by every layer that mirrors include/flacenc_hip.h, and adding it left
the ABI version at 6.  No GPU, no library."""
import fnmatch
import os
import re

from flacenc_rs_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "flacenc_hip_set_max_bits_per_sample"


def text(*path):
    return open(os.path.join(ROOT, *path)).read()


def test_the_header_declares_it():
    assert re.search(r"\bint\s+" + NAME + r"\(flacenc_hip_handle\*\s*h,\s*uint32_t\s+bits\);", text("include", "flacenc_hip.h"))


def test_the_version_script_exports_it():
    body = text("flacenc_rs_amd", "csrc", "exports.map")
    exported = re.search(r"global:(.*?)local:", body, re.S).group(1)
    patterns = [p.strip() for p in exported.split(";") if p.strip()]
    assert any(fnmatch.fnmatchcase(NAME, p) for p in patterns), patterns


def test_the_library_source_defines_it():
    assert re.search(r"\bint\s+" + NAME + r"\(flacenc_hip_handle\*\s*h,\s*uint32_t\s+bits\)\s*\{",
                     text("flacenc_rs_amd", "csrc", "api_handle.cpp"))
    assert "max_bps" in text("flacenc_rs_amd", "csrc", "api_internal.h")


def test_the_python_binding_declares_it():
    assert NAME in _capi.EXPORTED_SYMBOLS
    assert callable(getattr(_capi.Handle, "set_max_bits_per_sample"))
    assert re.search(r"L\." + NAME + r"\.argtypes = \[vp, C\.c_uint32\]", text("flacenc_rs_amd", "_capi.py"))


def test_the_rust_binding_declares_it():
    rs = text("rust", "flacenc_hip.rs")
    assert re.search(r"pub fn " + NAME + r"\(h: \*mut Handle, bits: u32\) -> c_int;", rs)
    assert "pub fn set_max_bits_per_sample(&self, bits: u32)" in rs


def test_the_cpp_mirror_declares_it():
    hpp = text("flacenc_rs_amd", "host", "flacenc.hpp")
    assert "void set_max_bits_per_sample(uint32_t bits)" in hpp and NAME + "(h_, bits)" in hpp


def test_the_abi_version_is_still_6():
    assert re.search(r"#define\s+FLACENC_HIP_ABI_VERSION\s+6\b", text("include", "flacenc_hip.h"))
    assert _capi.ABI_VERSION == 6
    assert re.search(r"ABI_VERSION:\s*c_int\s*=\s*6;", text("rust", "flacenc_hip.rs"))
