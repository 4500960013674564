"""Measurements for FLACENC_HIP_FLAG_RICE_ESCAPE (results in profiles/rice_escape_rates.txt).

    python tools/time_rice_escape.py pack   [--frames 24576] [--steps 20] [--repeats 5]
    python tools/time_rice_escape.py ab     --parent-lib PATH [--rounds 3] [--bench]
    python tools/time_rice_escape.py cost   [--frames 24576]
    python tools/time_rice_escape.py gain

pack   one process: flacenc_hip_pack_stereo_frames_async on the bench workload (frames of 4096 samples, order 8, the
       records of the unflagged encode), after bench.py's clock spin-up; `repeats` windows of `steps` launches between
       device events -> one JSON line with every window's ms per launch.
ab     the same in child processes that alternate between two builds of the library (FLACENC_HIP_LIB: the parent
       commit's and this tree's), `rounds` each -> per build the windows' median and the spread (max - min) / median
       over all of its windows; --bench does the same with `python bench.py --gpus 1` (its ms_per_step).
cost   the flagged frame-level call (encode + pack in one call) against the SAME call unflagged, on the bench workload
       and on blocks of 1152 samples, and the pass's own time per row (the flagged candidate batch less the unflagged
       one over the same rows).
gain   bytes with and without the flag on the four signal families of tests/escape_cases.py, the bench signal and the
       golden music fixtures.
Every time is taken between device events around launches on one stream; nothing here runs without a GPU."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def spin(fn, seconds=0.05):
    """bench.py's clock spin-up: the same work, untimed, for `seconds`."""
    import torch
    t = time.perf_counter()
    while time.perf_counter() - t < seconds:
        fn()
        torch.cuda.synchronize()


def windows(fn, steps, repeats):
    """`repeats` windows of `steps` launches between two device events -> ms per launch of each window."""
    import torch
    st = torch.cuda.current_stream()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(st)
        for _ in range(steps):
            fn()
        b.record(st)
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / steps)
    return out


def workload(F, n, bps=16):
    import torch
    from flacenc_rs_amd import _capi
    host = _capi.sigen_frames(F, 2, n, bps, 200.0, 0.4, 0.4, seed=0xF1AC0001)
    h = _capi.Handle(0)
    x = torch.from_numpy(host).cuda()
    res = torch.empty((F, _capi.FRAME_RESULT_DTYPE.itemsize), dtype=torch.uint8, device="cuda")
    stride = h.frame_bytes_bound(n, bps)
    out = torch.empty((F, stride), dtype=torch.uint8, device="cuda")
    lens = torch.zeros(F, dtype=torch.int32, device="cuda")
    return _capi, h, x, res, out, lens, stride


def cmd_pack(args):
    import torch
    F, n, bps = args.frames, 4096, 16
    _capi, h, x, res, out, lens, stride = workload(F, n)
    resid = torch.empty((F * 2, n), dtype=torch.int32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    cfg = _capi.make_frame_config(_capi.make_config(lpc_order=8))
    h.encode_stereo_frames_device(cfg, x.data_ptr(), F, n, n, bps, res.data_ptr(), resid.data_ptr(), n, stream=s)

    def pack():
        h.pack_stereo_frames_device(x.data_ptr(), F, n, n, res.data_ptr(), resid.data_ptr(), n, bps, 44100, 0, 1,
                                    out.data_ptr(), stride, lens.data_ptr(), stream=s)

    spin(pack)
    ms = windows(pack, args.steps, args.repeats)
    print(json.dumps({"what": "pack_stereo_frames", "lib": os.environ.get("FLACENC_HIP_LIB", "tree"), "frames": F,
                      "ms_per_launch": [round(v, 4) for v in ms], "bytes": int(lens.sum().item())}))


def child(argv, lib):
    env = dict(os.environ)
    if lib:
        env["FLACENC_HIP_LIB"] = lib
    else:
        env.pop("FLACENC_HIP_LIB", None)
    r = subprocess.run([sys.executable] + argv, env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    if r.returncode != 0:
        raise SystemExit("child failed (%d): %s" % (r.returncode, r.stderr[-2000:]))
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


def summary(values):
    med = statistics.median(values)
    return {"median_ms": round(med, 4), "min_ms": round(min(values), 4), "max_ms": round(max(values), 4),
            "spread": round((max(values) - min(values)) / med, 4), "windows": len(values)}


def cmd_ab(args):
    me = os.path.abspath(__file__)
    got = {"parent": [], "tree": []}
    bench = {"parent": [], "tree": []}
    for _ in range(args.rounds):
        for name, lib in (("parent", os.path.abspath(args.parent_lib)), ("tree", None)):
            got[name] += child([me, "pack", "--frames", str(args.frames), "--steps", str(args.steps), "--repeats",
                                str(args.repeats)], lib)["ms_per_launch"]
            print(name, "pack", got[name][-args.repeats:], file=sys.stderr, flush=True)
            if args.bench:
                bench[name].append(child([os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "3"],
                                         lib)["ms_per_step"])
                print(name, "bench", bench[name][-1], file=sys.stderr, flush=True)
    out = {"what": "pack_stereo_frames, parent against tree, alternating processes", "frames": args.frames,
           "parent": summary(got["parent"]), "tree": summary(got["tree"])}
    out["tree_over_parent"] = round(out["tree"]["median_ms"] / out["parent"]["median_ms"], 4)
    if args.bench:
        out["bench_ms_per_step"] = {k: summary(v) for k, v in bench.items()}
        out["bench_tree_over_parent"] = round(out["bench_ms_per_step"]["tree"]["median_ms"] /
                                              out["bench_ms_per_step"]["parent"]["median_ms"], 4)
    print(json.dumps(out))


def cmd_cost(args):
    import torch
    rows = []
    for n, F in ((4096, args.frames), (1152, args.frames)):
        _capi, h, x, res, out, lens, stride = workload(F, n)
        s = torch.cuda.current_stream().cuda_stream
        params = torch.empty((F * 4, _capi.PARAMS_DTYPE.itemsize), dtype=torch.uint8, device="cuda")
        cand = torch.empty((F * 4, n), dtype=torch.int32, device="cuda")
        entry = {"block_size": n, "frames": F}
        for name, flags in (("unflagged", 0), ("flagged", _capi.FLAG_RICE_ESCAPE)):
            q = _capi.make_config(lpc_order=8, flags=flags)
            cfg = _capi.make_frame_config(q)

            def call():
                h.encode_pack_stereo_frames_device(cfg, x.data_ptr(), F, n, n, 16, 44100, 0, 1, res.data_ptr(),
                                                   out.data_ptr(), stride, lens.data_ptr(), stream=s)

            def batch():
                h.stereo_qlpc_batch_device(q, x.data_ptr(), F, n, n, 16, params.data_ptr(), cand.data_ptr(), n, stream=s)

            spin(call)
            entry[name + "_encode_pack_ms"] = round(statistics.median(windows(call, 5, 5)), 4)
            entry[name + "_bytes"] = int(lens.sum().item())
            spin(batch)
            entry[name + "_candidate_batch_ms"] = round(statistics.median(windows(batch, 5, 5)), 4)
        entry["flagged_over_unflagged"] = round(entry["flagged_encode_pack_ms"] / entry["unflagged_encode_pack_ms"], 2)
        entry["flagged_Msamples_per_s"] = round(F * 2 * n / entry["flagged_encode_pack_ms"] / 1e3, 1)
        entry["unflagged_Msamples_per_s"] = round(F * 2 * n / entry["unflagged_encode_pack_ms"] / 1e3, 1)
        entry["pass_us_per_row"] = round((entry["flagged_candidate_batch_ms"] - entry["unflagged_candidate_batch_ms"]) *
                                         1e3 / (F * 4), 4)
        rows.append(entry)
        del h, x, res, out, lens, params, cand
        torch.cuda.empty_cache()
    print(json.dumps({"what": "cost of FLACENC_HIP_FLAG_RICE_ESCAPE", "rows": rows}))


def cmd_gain(args):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import escape_cases as ec
    import util
    from flacenc_rs_amd import _capi
    h = _capi.Handle(0)

    def size(x, bps, flags):
        cfg = _capi.make_frame_config(_capi.make_config(lpc_order=8, flags=flags), use_fixed=True)
        res, resid = h.encode_stereo_frames(x, bps, cfg)
        return sum(len(b) for b in h.pack_stereo_frames(x, res, resid, bps, 44100))

    material = {}
    for name in ec.ESCAPING[1:]:
        fam = ec.FAMILIES[name]
        material[name] = (np.stack([np.stack([fam(4096, 2 * f)[0], fam(4096, 2 * f + 1)[0]]) for f in range(32)]),
                          fam(4096)[1])
    ramp = ec.ramp(4096)[0]
    material["ramp"] = (np.stack([np.stack([ramp, ramp[::-1]])] * 32).astype(np.int32), 24)
    material["bench signal"] = (_capi.sigen_frames(256, 2, 4096, 16, 200.0, 0.4, 0.4, seed=0xF1AC0001), 16)
    golden = sorted({f.split(".")[1] for f in os.listdir(util.GOLDEN) if f.startswith("testsignal.") and ".ch0." in f})
    for name in golden:
        l, r = util.test_signal(name, 0), util.test_signal(name, 1)
        nf = len(l) // 4096
        material["golden " + name] = (np.stack([l[:nf * 4096].reshape(nf, 4096), r[:nf * 4096].reshape(nf, 4096)],
                                               axis=1).astype(np.int32), 16)
    rows = []
    for name, (x, bps) in material.items():
        a, b = size(x, bps, 0), size(x, bps, _capi.FLAG_RICE_ESCAPE)
        rows.append({"material": name, "frames": len(x), "bytes_unflagged": a, "bytes_flagged": b,
                     "change": round(b / a - 1.0, 6)})
    print(json.dumps({"what": "bytes with and without FLACENC_HIP_FLAG_RICE_ESCAPE (4096-sample stereo frames, order 8, "
                              "fixed candidate on)", "rows": rows}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("command", choices=["pack", "ab", "cost", "gain"])
    ap.add_argument("--frames", type=int, default=24576)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent-lib")
    ap.add_argument("--bench", action="store_true")
    args = ap.parse_args()
    if args.command == "ab" and not args.parent_lib:
        ap.error("ab needs --parent-lib")
    {"pack": cmd_pack, "ab": cmd_ab, "cost": cmd_cost, "gain": cmd_gain}[args.command](args)


if __name__ == "__main__":
    main()
