"""The launch routing of csrc/qlpc_dispatch.cpp without a GPU: which launchers a launch record reaches, in which order
and with which arguments.  tests/host/dispatch_trace.cpp links the real dispatch unit, compiled for the host alone,
against stub launchers that only write down what they were given, walks a grid of records (call shapes x block sizes x
orders x the full cross product of the flag axes) through launch_qlpc and launch_subwave_frames, and prints digests of
the traces.  They must equal tests/golden/dispatch_routes.txt: a launch that takes another route, an equivalent one
included, fails here.  ("The route of a launch", says how to re-record the golden when routing is meant to
change, and how to find the launch that differs.)"""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "flacenc_rs_amd", "csrc")
INCLUDE = os.path.join(ROOT, "include")
GOLDEN = os.path.join(ROOT, "tests", "golden", "dispatch_routes.txt")


def makefile_hipcc():
    """HIPCC as csrc/Makefile has it (`HIPCC ?= ...`: the environment's wins)."""
    default = re.search(r"^HIPCC \?= *(\S+)", open(os.path.join(CSRC, "Makefile")).read(), re.M).group(1)
    return os.environ.get("HIPCC", default)


def parse(text):
    groups, sequences, launchers = {}, {}, {}
    for line in text.splitlines():
        w = line.split()
        if w[0] == "g":
            groups[(int(w[1]), int(w[2]), int(w[3]))] = (int(w[4]), w[5], int(w[6]))
        elif w[0] == "s":
            sequences[(w[2], tuple(w[3:]))] = int(w[1])
        elif w[0] == "l":
            launchers[w[1]] = int(w[2])
    return groups, sequences, launchers


@pytest.fixture(scope="module")
def routes(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("dispatch_trace") / "dispatch_trace")
    subprocess.check_call([makefile_hipcc(), "--offload-host-only", "-O2", "-std=c++17", "-Wall", "-Werror",
                           "-Wno-unused-function", "-I", INCLUDE, "-I", CSRC, "-x", "hip",
                           os.path.join(ROOT, "tests", "host", "dispatch_trace.cpp"),
                           os.path.join(CSRC, "qlpc_dispatch.cpp"), os.path.join(CSRC, "frame_plan.cpp"), "-pthread", "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    return p.stdout


def test_every_group_of_the_grid_takes_the_recorded_routes(routes):
    got, want = parse(routes)[0], parse(open(GOLDEN).read())[0]
    assert sorted(got) == sorted(want)
    shapes = dict(kv.split("=") for kv in open(GOLDEN).read().splitlines()[1].split()[2:])
    differ = ["%s:%d:%d" % (shapes[str(s)], n, p) for (s, n, p) in sorted(want) if got[(s, n, p)] != want[(s, n, p)]]
    assert not differ, "%d groups differ; compare `dispatch_trace --dump %s` of the two builds" % (len(differ), differ[0])
    assert routes == open(GOLDEN).read()


def test_every_stub_launcher_is_reached(routes):
    """each launcher the dispatch unit can call -- every per-instance one -- occurs in at least one trace"""
    launchers = parse(routes)[2]
    header = open(os.path.join(CSRC, "qlpc_kernel.h")).read()

    def instances(macro):
        body = re.search(r"#define %s\(X\)((?:.*\\\n)*.*)\n" % macro, header).group(1)
        return ["_".join(re.findall(r"\d+", m)) for m in re.findall(r"X\(([^)]*)\)", body)]

    want = ["launch_qlpc_" + i for i in instances("FLACENC_HIP_FOR_EACH_INSTANCE")]
    want += ["launch_levinson_" + i for i in instances("FLACENC_HIP_FOR_EACH_INSTANCE")]
    want += ["launch_qlpc_wave_" + i for i in instances("FLACENC_HIP_FOR_EACH_WAVE_INSTANCE")]
    want += ["launch_qlpc_wave72_" + i for i in instances("FLACENC_HIP_FOR_EACH_WAVE72_INSTANCE")]
    want += ["launch_qlpc_subwave_" + i for i in instances("FLACENC_HIP_FOR_EACH_SUBWAVE_INSTANCE")]
    want += ["launch_bigblock_acorr", "launch_bigblock_residual", "launch_bigblock_fixed_select",
             "launch_bigblock_fixed_residual", "launch_acorr_reference", "launch_sumabs_reference", "launch_direct_mse"]
    assert len(want) == 8 + 8 + 24 + 21 + 28 + 7
    assert sorted(launchers) == sorted(want)
    assert [name for name in want if launchers[name] == 0] == []


def test_no_error_return_the_golden_does_not_have(routes):
    """every launch of the grid that comes back with hipErrorInvalidValue / hipErrorNotSupported does so in the golden
    too: after the same launchers, as often"""
    got, want = parse(routes)[1], parse(open(GOLDEN).read())[1]
    errors = {k: v for k, v in got.items() if k[0] != "hipSuccess"}
    assert errors and {k[0] for k in errors} == {"hipErrorInvalidValue", "hipErrorNotSupported"}
    for key, count in errors.items():
        assert want.get(key) == count, key
    assert {k: v for k, v in want.items() if k[0] != "hipSuccess"} == errors
