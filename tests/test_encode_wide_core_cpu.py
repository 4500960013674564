"""wide_encode_core.h, the serial statement of the wide encode path, as a stand-alone program under AddressSanitizer and
UBSan (tests/host/wide_encode_core_test.cpp): its frames equal wide_model's byte for byte on every case, without and with
wasted bits, at other frame numbers and sample rates, and none is longer than its bytes bound.  No GPU."""
import os
import subprocess

import pytest

import wide_cases as wc
import wide_model as wm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "flacenc_rs_amd", "csrc")
INCLUDE = os.path.join(ROOT, "include")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("wide_encode_core") / "wide_encode_core_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-static-libasan",
                           "-static-libubsan", "-I", INCLUDE, "-I", CSRC,
                           os.path.join(ROOT, "tests", "host", "wide_encode_core_test.cpp"), "-o", path])
    return path


def run(exe, tmp_path, case_list, wasted, **kw):
    src, dst = tmp_path / "cases.bin", tmp_path / "frames.bin"
    src.write_bytes(wc.case_file(case_list, wasted, **kw))
    p = subprocess.run([exe, str(src), str(dst)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-2000:]
    assert "wide OK %d" % len(case_list) in p.stdout
    return wc.read_frames(dst.read_bytes(), len(case_list))


@pytest.mark.parametrize("wasted", (False, True))
def test_the_core_writes_the_models_frames(exe, tmp_path, wasted):
    got = run(exe, tmp_path, wc.cases(), wasted)
    for c, (frame, bound), (want, _) in zip(wc.cases(), got, wc.modelled(wasted)):
        assert frame == want, c["name"]
        assert len(frame) <= bound, c["name"]


def test_frame_numbers_and_sample_rates_reach_the_header(exe, tmp_path):
    picked = [c for c in wc.cases() if c["x"].shape[1] in (17, 192)][:6]
    for number, rate in ((127, 48000), (128, 50000), ((1 << 31) - 1, 12345), (70000, 1234560)):
        got = run(exe, tmp_path, picked, True, rate=rate, number=number)
        for c, (frame, bound) in zip(picked, got):
            want, _ = wm.encode_frame(c["x"], c["bps"], dict(c["cfg"], wasted_bits=True), number=number, rate=rate)
            assert frame == want and len(frame) <= bound, (c["name"], number, rate)
