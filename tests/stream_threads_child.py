"""Two handles, two streams, two host threads, in a process in which no handle exists and no kernel of the library has
been launched yet (started once by tests/test_gpu_stream_contract.py).

    python tests/stream_threads_child.py REPORT.json

The first use of every kernel in the process -- the `static DynamicLdsOptIn` bookkeeping of lds_opt_in.h, which all
handles share -- and of every handle -- its scratch, its window cache, its marked-subframe counters -- happens while the
other thread is inside the library: the inputs of stream_cases.SEQUENCES are built without a handle (Case.inputs), two
fresh handles launch their six cases each from a thread of their own (ctypes releases the GIL inside the calls), with no
synchronise between the calls, and only after the join does a third handle run the blocking forms that state what the
outputs must be.  Then both sequences run again interleaved from one thread.  The report is one entry per (phase, case):
the first output that differs, or null."""
import json
import os
import sys
import threading

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)


def main(path):
    import torch

    import stream_cases as sc
    from flacenc_rs_amd import _capi

    report = {"error": None, "threads": {}, "interleaved": {}}
    try:
        torch.zeros(1, device="cuda")
        work = [[sc.Bound(sc.by_name(name), None) for name in seq] for seq in sc.SEQUENCES]
        for seq in work:
            for b in seq:
                b.load("X")
                b.arm()
        handles = [_capi.Handle(0), _capi.Handle(0)]
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        torch.cuda.synchronize()
        errors, gate = [], threading.Barrier(2)

        def run(i):
            try:
                gate.wait(timeout=30)
                for b in work[i]:
                    b.launch(handles[i], streams[i].cuda_stream)
                streams[i].synchronize()
            except Exception as e:  # noqa: BLE001
                errors.append("thread %d: %r" % (i, e))

        threads = [threading.Thread(target=run, args=(i,)) for i in range(2)]
        for t in threads:
            t.start()
        for t in threads:
            t.join(timeout=120)
        if errors or any(t.is_alive() for t in threads):
            raise RuntimeError("; ".join(errors) or "a thread did not end")
        got = {"threads": [[b.collect() for b in seq] for seq in work]}
        for seq in work:
            for b in seq:
                b.arm()
        torch.cuda.current_stream().synchronize()
        for b0, b1 in zip(*work):
            b0.launch(handles[0], streams[0].cuda_stream)
            b1.launch(handles[1], streams[1].cuda_stream)
        for s in streams:
            s.synchronize()
        got["interleaved"] = [[b.collect() for b in seq] for seq in work]
        # only now the references: the blocking forms on a handle of their own
        with _capi.Handle(0) as ref:
            for i, seq in enumerate(work):
                for j, b in enumerate(seq):
                    b.resolve(ref)
                    for phase in ("threads", "interleaved"):
                        g = got[phase][i][j]
                        report[phase][b.case.name] = None if sc.same(g, b.expected["X"]) else \
                            str(sc.first_difference(g, b.expected["X"]))
    except Exception as e:  # noqa: BLE001 -- the report carries it
        report["error"] = "%s: %s" % (type(e).__name__, e)
    with open(path, "w") as f:
        json.dump(report, f)
    return 1 if report["error"] else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
