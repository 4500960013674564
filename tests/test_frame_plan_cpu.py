"""The plan of a frame-level call (csrc/frame_plan.cpp) without a GPU.  tests/host/frame_plan_test.cpp links the real
planner and the real dispatch unit, compiled for the host alone, against the stub launchers the dispatch trace uses
(tests/host/stub_launchers.h) and walks calls x blocks x orders x row alignment x config switches x flags x handle state
through plan_frame_call.  At every point the plan must equal the conditions of the layer it replaced (the program's
legacy_* functions), agree with plan_qlpc_route on what its records launch, and grant scratch so that every launch comes
back with hipSuccess and no record that is denied the split scratch would route differently with one.  ("The
plan of a frame-level call".)"""
import os
import re
import subprocess
import time

import pytest

from test_dispatch_routes_cpu import CSRC, INCLUDE, ROOT, makefile_hipcc


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("frame_plan") / "frame_plan_test")
    subprocess.check_call([makefile_hipcc(), "--offload-host-only", "-O2", "-std=c++17", "-Wall", "-Werror",
                           "-Wno-unused-function", "-I", INCLUDE, "-I", CSRC, "-x", "hip",
                           os.path.join(ROOT, "tests", "host", "frame_plan_test.cpp"),
                           os.path.join(CSRC, "frame_plan.cpp"), os.path.join(CSRC, "qlpc_dispatch.cpp"), "-pthread",
                           "-o", exe])
    t0 = time.monotonic()
    p = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    return p, time.monotonic() - t0


def test_the_plan_equals_the_parent_and_its_records_route_and_launch(run):
    p, _ = run
    assert p.returncode == 0, p.stderr[-3000:] + p.stdout
    counts = {k: int(v) for k, v in re.findall(r"(\w+) (\d+)", p.stdout)}
    assert counts["failures"] == 0
    # the grid reaches every path, and the general path most of the time (every search flag and escape lands there)
    assert all(counts[k] > 1000 for k in ("fused", "bigblock", "subwave", "general")), counts
    assert counts["points"] == sum(counts[k] for k in ("fused", "bigblock", "subwave", "general")) > 20_000_000
    assert counts["launches"] > counts["points"] // 4


def test_the_grid_runs_in_well_under_a_minute(run):
    assert run[1] < 60.0, run[1]  # (26 s of CPU time over up to eight threads when this was written)

