"""Builds and runs tests/host/variable_test.cpp: HipContext::encode_variable of the C++ host mirror
(flacenc_rs_amd/host/flacenc.hpp) over the C ABI's flacenc_hip_encode_variable, decoded back by flacenc::decode_frames."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_variable_test(out_dir):
    out = os.path.join(out_dir, "variable_test")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "flacenc_rs_amd", "host"),
                           os.path.join(ROOT, "tests", "host", "variable_test.cpp"),
                           "-L", os.path.join(ROOT, "flacenc_rs_amd"), "-lflacenc_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "flacenc_rs_amd"), "-Wl,-rpath,/opt/rocm/lib",
                           "-L/opt/rocm/lib", "-lamdhip64", "-pthread", "-o", out])
    return out


def test_host_variable_compiles(tmp_path):
    assert os.path.exists(build_variable_test(str(tmp_path)))


@pytest.mark.gpu
def test_host_variable_on_gpu(tmp_path):
    res = subprocess.run([build_variable_test(str(tmp_path))], capture_output=True, text=True, timeout=600)
    print(res.stdout[-2000:], res.stderr[-2000:])
    assert res.returncode == 0 and "variable_test OK" in res.stdout
