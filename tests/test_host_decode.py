"""Builds and runs tests/host/decode_test.cpp: flacenc::decode_frames of the C++ host mirror
(flacenc_rs_amd/host/flacenc.hpp) over the C ABI's flacenc_hip_decode_frames."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_decode_test(out_dir):
    out = os.path.join(out_dir, "decode_test")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "flacenc_rs_amd", "host"),
                           os.path.join(ROOT, "tests", "host", "decode_test.cpp"),
                           "-L", os.path.join(ROOT, "flacenc_rs_amd"), "-lflacenc_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "flacenc_rs_amd"), "-Wl,-rpath,/opt/rocm/lib",
                           "-L/opt/rocm/lib", "-lamdhip64", "-pthread", "-o", out])
    return out


def test_host_decode_compiles(tmp_path):
    assert os.path.exists(build_decode_test(str(tmp_path)))


@pytest.mark.gpu
def test_host_decode_on_gpu(tmp_path):
    res = subprocess.run([build_decode_test(str(tmp_path))], capture_output=True, text=True, timeout=600)
    print(res.stdout[-2000:], res.stderr[-2000:])
    assert res.returncode == 0 and "decode_test OK" in res.stdout
