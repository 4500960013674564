"""CPU: the fused kernel's straight-line full-order solver (levinson_quantize_full) equals the generic one
(levinson_quantize at P == MAXP) bit for bit wherever it does not ask for the second solve, and asks for it exactly in
the generic code's corners -- on the text of flacenc_rs_amd/csrc/qlpc_kernel_impl.h itself, cut out and compiled for the
host (tests/host/solver_full_order_test.cpp), with the kernels' floating-point flags."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def solver_slice():
    src = open(os.path.join(ROOT, "flacenc_rs_amd", "csrc", "qlpc_kernel_impl.h")).read()
    log2 = re.search(r"// exact ceil\(log2\(m\)\).*?\n}\n", src, re.S).group(0)
    begin = src.index("constexpr double kCertSafety")
    end = src.index("// phase 1 inner block")
    end = src.rindex("// ------", begin, end)
    body = src[begin:end]
    for name in ("levinson_core", "quant_certified", "levinson_quantize", "levinson_core_full", "levinson_quantize_full"):
        assert re.search(r"\b%s\(" % name, body), name
    return log2 + "\n" + body


def test_full_order_solver_equals_generic_solver_on_the_host(tmp_path):
    (tmp_path / "solver_slice.inc").write_text(solver_slice())
    exe = str(tmp_path / "solver_full_order_test")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-I", str(tmp_path),
                           os.path.join(ROOT, "tests", "host", "solver_full_order_test.cpp"), "-o", exe])
    res = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(res.stdout[-4000:], res.stderr[-2000:])
    assert res.returncode == 0
    cases, redo, failures = (int(v) for v in re.search(r"(\d+) cases, (\d+) asked for the second solve, (\d+) failures",
                                                       res.stdout).groups())
    assert failures == 0 and cases > 100000 and 0 < redo < cases // 2  # (most of the arbitrary and near-singular systems ask for it; the material does not)
