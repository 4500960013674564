"""flacenc_hip_set_max_encode_bits_per_sample and flacenc_hip_encode_pack_frames_wide are declared by every layer
that mirrors include/flacenc_hip.h, and adding them left the ABI version at 6.  No GPU, no library."""
import fnmatch
import os
import re

from flacenc_rs_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETTER = "flacenc_hip_set_max_encode_bits_per_sample"
WIDE = "flacenc_hip_encode_pack_frames_wide"


def text(*path):
    return open(os.path.join(ROOT, *path)).read()


def test_the_header_declares_them():
    header = text("include", "flacenc_hip.h")
    assert re.search(r"\bint\s+" + SETTER + r"\(flacenc_hip_handle\*\s*h,\s*uint32_t\s+bits\);", header)
    assert re.search(r"\bint\s+" + WIDE + r"\(flacenc_hip_handle\*\s*h,\s*const flacenc_hip_frame_config\*\s*cfg,", header)
    # what the path does not read is stated where the call is declared
    doc = header[header.index("The wide encode path"):header.index("int " + WIDE)]
    for word in ("use_lpc", "FLACENC_HIP_FLAG_RICE_ESCAPE", "fixed_order_sel", "fixed_partitions"):
        assert word in doc, word


def test_the_version_script_exports_them():
    exported = re.search(r"global:(.*?)local:", text("flacenc_rs_amd", "csrc", "exports.map"), re.S).group(1)
    patterns = [p.strip() for p in exported.split(";") if p.strip()]
    for name in (SETTER, WIDE):
        assert any(fnmatch.fnmatchcase(name, p) for p in patterns), patterns


def test_the_library_source_defines_them():
    assert re.search(r"\bint\s+" + SETTER + r"\(flacenc_hip_handle\*\s*h,\s*uint32_t\s+bits\)\s*\{",
                     text("flacenc_rs_amd", "csrc", "api_handle.cpp"))
    assert "max_encode_bps" in text("flacenc_rs_amd", "csrc", "api_internal.h")
    assert re.search(r'extern "C" int ' + WIDE + r"\(", text("flacenc_rs_amd", "csrc", "wide_encode.cpp"))
    # the step the stream-level calls enqueue on their own streams is internal: no _async form is exported yet
    assert WIDE + "_async" not in text("include", "flacenc_hip.h") and WIDE + "_async" not in _capi.EXPORTED_SYMBOLS


def test_the_python_binding_declares_them():
    for name in (SETTER, WIDE):
        assert name in _capi.EXPORTED_SYMBOLS
    assert callable(getattr(_capi.Handle, "set_max_encode_bits_per_sample"))
    assert callable(getattr(_capi.Handle, "encode_pack_frames_wide_device"))
    assert re.search(r"L\." + SETTER + r"\.argtypes = \[vp, C\.c_uint32\]", text("flacenc_rs_amd", "_capi.py"))


def test_the_rust_binding_declares_them():
    rs = text("rust", "flacenc_hip.rs")
    assert re.search(r"pub fn " + SETTER + r"\(h: \*mut Handle, bits: u32\) -> c_int;", rs)
    assert "pub fn set_max_encode_bits_per_sample(&self, bits: u32)" in rs
    assert re.search(r"pub fn " + WIDE + r"\(", rs)


def test_the_cpp_mirror_declares_it():
    hpp = text("flacenc_rs_amd", "host", "flacenc.hpp")
    assert "void set_max_encode_bits_per_sample(uint32_t bits)" in hpp and SETTER + "(h_, bits)" in hpp


def test_the_integration_guide_names_it():
    assert SETTER in text("INTEGRATION.md") and WIDE in text("INTEGRATION.md")


def test_the_abi_version_is_still_6():
    assert re.search(r"#define\s+FLACENC_HIP_ABI_VERSION\s+6\b", text("include", "flacenc_hip.h"))
    assert _capi.ABI_VERSION == 6
    assert re.search(r"ABI_VERSION:\s*c_int\s*=\s*6;", text("rust", "flacenc_hip.rs"))
