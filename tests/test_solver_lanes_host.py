"""CPU: the fused kernel's lane-parallel quantise-and-certify step (levinson_phase_lanes) equals levinson_quantize_full.
The arithmetic the kernel's lanes run is flacenc_rs_amd/csrc/solver_lanes_core.h; tests/host/solver_lanes_test.cpp
assembles it the way the lanes do and compares qc[], order, shift, certified, tier2 and redo, as integers, with
levinson_quantize_full cut from qlpc_kernel_impl.h itself -- on the systems of test_solver_full_order_host.py through the
real recursion, and on constructed coefficient vectors (rounding ties, clamps at lo / hi, order truncation, shift 0 / 15,
non-finite entries, all zeros, max |a| a power of two) through a copy of that text whose one call of the recursion hands
out the constructed vectors instead.  Once optimised, once under AddressSanitizer + UBSan (a stand-alone host program)."""
import os
import re
import subprocess

import pytest

from test_solver_full_order_host import ROOT, solver_slice

CORE_CALL = "levinson_core_full<MAXP>(R, a, fwd, &skipped, &nonpd);"


def build_and_run(tmp_path, name, flags):
    text = solver_slice()
    (tmp_path / "solver_slice.inc").write_text(text)
    head, call, tail = text.rpartition(CORE_CALL)  # (the last one: levinson_quantize_full's)
    assert call and "levinson_quantize_full" in head[head.rindex("template <int MAXP, bool CERT>"):]
    (tmp_path / "solver_slice_injected.inc").write_text(head + "inject_core<MAXP>(R, a, fwd, &skipped, &nonpd);" + tail)
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", *flags, "-I", str(tmp_path),
                           "-I", os.path.join(ROOT, "flacenc_rs_amd", "csrc"),
                           os.path.join(ROOT, "tests", "host", "solver_lanes_test.cpp"), "-o", exe])
    res = subprocess.run([exe], capture_output=True, text=True, timeout=900)
    print(res.stdout[-4000:], res.stderr[-4000:])
    assert res.returncode == 0
    m = re.search(r"(\d+) cases \((\d+) through the recursion\), (\d+) asked for the second solve, (\d+) certified, "
                  r"(\d+) second tier, (\d+) at lo, (\d+) at hi, (\d+) shortened, (\d+) failures", res.stdout)
    cases, systems, redo, certified, tier2, at_lo, at_hi, shortened, failures = (int(v) for v in m.groups())
    assert failures == 0
    # 16 212 systems x 3 precisions x certificate on / off, and every constructed event occurred
    assert systems == 16212 * 6 and cases > systems + 50000
    assert 0 < redo < cases // 2 and certified > 1000 and tier2 > 1000 and at_lo > 100 and at_hi > 100 and shortened > 100


@pytest.mark.parametrize("name,flags", [("solver_lanes_test", ["-O2"]),
                                        ("solver_lanes_test_san", ["-O1", "-g", "-fsanitize=address,undefined",
                                                                   "-fno-sanitize-recover=undefined"])])
def test_lane_parallel_quantiser_equals_levinson_quantize_full(tmp_path, name, flags):
    build_and_run(tmp_path, name, flags)
