"""CPU: the lane-major copy of the window table that the fused 4096 kernel reads at four workgroups per CU
(flacenc_rs_amd/csrc/window_lanes_core.h) holds the time-major weights, entry for entry.  tests/host/window_lanes_test.cpp
runs the header's builder -- the one get_window_entry runs -- on the library's own weights (flacenc_hip_lpc_window_weights)
for Tukey(0.4), Tukey(1.0), a tiny alpha, a partial and a punch-out piece, and checks every (j, lane, i) against
w[64 lane - 12 + 4 j + i], the zeros outside the block, the table's size and the reads the kernel makes of it.  Once
optimised, once under AddressSanitizer + UBSan (a stand-alone host program)."""
import os
import re
import subprocess

import pytest

from flacenc_rs_amd import _capi

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
N = 4096
WINDOWS = [
    (_capi.WINDOW_TUKEY, 0.4, 0, 0),
    (_capi.WINDOW_TUKEY, 1.0, 0, 0),
    (_capi.WINDOW_TUKEY, 0.005, 0, 0),  # (a taper of 10 samples: ends inside lane 0's first quads)
    (_capi.WINDOW_PARTIAL_TUKEY, 0.2, 29492, 65536),
    (_capi.WINDOW_PUNCHOUT_TUKEY, 0.2, 21845, 43690),
]


@pytest.mark.parametrize("name,flags", [("window_lanes_test", ["-O2"]),
                                        ("window_lanes_test_san", ["-O1", "-g", "-fsanitize=address,undefined",
                                                                   "-fno-sanitize-recover=undefined"])])
def test_lane_major_table_equals_time_major_weights(tmp_path, name, flags):
    files = []
    for k, e in enumerate(WINDOWS):
        w = _capi.lpc_window_weights(*e, N)
        assert w.dtype == "float32" and w.shape == (N,) and (w != 1.0).any()
        path = tmp_path / f"w{k}.f32"
        w.tofile(path)
        files.append(str(path))
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wall", *flags,
                           "-I", os.path.join(ROOT, "flacenc_rs_amd", "csrc"),
                           os.path.join(ROOT, "tests", "host", "window_lanes_test.cpp"), "-o", exe])
    res = subprocess.run([exe, *files], capture_output=True, text=True, timeout=120)
    print(res.stdout[-4000:], res.stderr[-4000:])
    assert res.returncode == 0
    m = re.search(r"(\d+) windows, (\d+) entries, (\d+) zeros outside the block, (\d+) kernel reads, (\d+) failures",
                  res.stdout)
    windows, entries, zeros, reads, failures = (int(v) for v in m.groups())
    assert failures == 0 and windows == len(WINDOWS)
    # 21 slots x 64 lanes x 4 per window; lane 0's three slots in front of the block and lane 63's two behind it
    assert entries == windows * 5376 and zeros == windows * 20 and reads == entries
