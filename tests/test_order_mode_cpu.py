"""The order mode of the certified shapes without a GPU: tests/host/order_mode_core_test.cpp scripts verdict sequences
against flacenc_rs_amd/csrc/order_mode_core.h -- the step launch_adaptive (api_candidates.cpp) wraps its HIP calls around
-- and checks, from the header's constants: easy material never leaves the certified form, a verdict above kHardShare
opens a span of 8, spans double to 64 and stay, one probe per span, launches behind an unanswered probe stay two-pass, an
easy probe returns to certified, feedback only once enough subframes have accumulated, sequence numbers wrap without 0,
and a launch of 2^25 subframes is not watched.  Built by g++, plain and under ASan + UBSan."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_scripted_verdict_sequences(tmp_path, sanitize):
    exe = str(tmp_path / "order_mode_core_test")
    cmd = ["g++", "-O1" if sanitize else "-O2", "-std=c++17", "-Wall", "-Werror", "-I",
           os.path.join(ROOT, "flacenc_rs_amd", "csrc")]
    if sanitize:
        cmd += ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    subprocess.run(cmd + [os.path.join(ROOT, "tests", "host", "order_mode_core_test.cpp"), "-o", exe], check=True,
                   capture_output=True, text=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "all checks passed" in p.stdout

