"""Capture and replay of every capturable case of tests/stream_cases.py, in a process of its own (started once by
tests/test_gpu_stream_contract.py): a capture that the runtime invalidates must not cascade into the rest of the suite.

    python tests/stream_capture_child.py REPORT.json

Per case: warm the handle at that shape, capture the single async call on static buffers into a graph on a non-NULL stream
(capture_error_mode="global": an allocation, a synchronise or a launch on another stream during the capture is an error),
replay three times -- X, D, X again, each copied into the static input on the same stream before its replay -- and compare
every replay with that input's reference.  The third replay catches what a replay leaves behind (counter slots, the
order mode's feedback word).  One stream is captured: every graph is linear.

The report is rewritten after every case; the run stops at the first error (an exception from the library, the runtime or
the capture), so a case that is missing from the report did not run."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)


def main(path):
    import torch

    import stream_cases as sc
    from flacenc_rs_amd import _capi

    report = {"cases": {}, "stopped_at": None}

    def save():
        with open(path + ".tmp", "w") as f:
            json.dump(report, f)
        os.replace(path + ".tmp", path)

    save()
    ref, dut = _capi.Handle(0), _capi.Handle(0)
    for case in sc.all_cases():
        if not case.capturable:
            continue
        entry = {"error": None, "replays": [], "differs": []}
        report["cases"][case.name] = entry
        try:
            b = sc.Bound(case, ref)
            b.load("D")
            b.arm()
            b.launch(dut, torch.cuda.current_stream().cuda_stream)   # warm at this shape
            torch.cuda.synchronize()
            s, g = torch.cuda.Stream(), torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=s, capture_error_mode="global"):
                b.launch(dut, torch.cuda.current_stream().cuda_stream)
            for which in "XDX":
                with torch.cuda.stream(s):
                    b.arm()
                    b.load(which)
                    g.replay()
                s.synchronize()
                got = b.collect()
                entry["replays"].append(sc.same(got, b.expected[which]))
                entry["differs"].append(sc.first_difference(got, b.expected[which]))
            del g
        except Exception as e:  # noqa: BLE001 -- the report carries it; nothing more runs on this runtime
            entry["error"] = "%s: %s" % (type(e).__name__, e)
            report["stopped_at"] = case.name
            save()
            return 1
        save()
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
