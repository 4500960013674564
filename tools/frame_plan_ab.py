#!/usr/bin/env python3
"""A/B driver for the host layer that plans frame-level calls (csrc/frame_plan.cpp, api_frames.cpp, api_candidates.cpp):
runs every entry point that goes through it, so that two builds can be compared kernel by kernel and call by call.

  frame_plan_ab.py calls [--root DIR] [--log FILE]
      On one handle, 8 frames per call, at every (shape, fixed config, flag) of the grid below, one after the other:
      encode_stereo_frames, encode_frames with 1 and 3 channels, encode_pack_stereo_frames (default and FUSED_PACK) and
      the three candidate batches, each followed by a synchronise.  Writes one line per call (what, return code, a
      checksum of every output, the handle's scratch bytes) to FILE.  Run it under `rocprofv3 --kernel-trace --output-format csv -d DIR -- python ...`
      and nothing else with it.
  frame_plan_ab.py sequence KERNEL_TRACE_CSV
      Prints rocprofv3's kernel trace as the ordered list of (kernel name, grid, workgroup size): a table of the
      distinct ones and the sequence of indices into it.
  frame_plan_ab.py launches [--root DIR] [--calls 2000] [--repeat 5]
      The launch-bound case: back-to-back encode_stereo_frames_device calls of 8 frames at 4096 / order 8, ending in one
      synchronise; prints a JSON line with the microseconds per call of every repetition.

--root names the tree whose flacenc_rs_amd package (and library) is loaded: this one by default, a build of another
commit in a second directory for the other side of the comparison.  DESIGN.md, "The plan of a frame-level call"."""
import argparse
import csv
import json
import os
import sys
import time
import zlib

SHAPES = [(63, 8), (192, 8), (1152, 8), (4096, 8), (4096, 16), (4608, 10), (8192, 8)]
FRAMES, BPS = 8, 16


def load(root):
    sys.path.insert(0, os.path.abspath(root))
    import numpy as np
    import torch
    from flacenc_rs_amd import _capi
    assert os.path.abspath(_capi.__file__).startswith(os.path.abspath(root)), _capi.__file__
    return np, torch, _capi


def grid(_capi):
    fixed = [("nofixed", dict(use_fixed=False)), ("approxent32", dict(use_fixed=True, fixed_partitions=32)),
             ("approxent3", dict(use_fixed=True, fixed_partitions=3))]
    flags = [("plain", 0)] + [(n, getattr(_capi, "FLAG_" + n)) for n in (
        "WASTED_BITS", "ORDER_SEARCH", "RICE_ESCAPE", "REFERENCE_SUM_ORDER", "CANONICAL_SUM_ORDER", "GENERIC_KERNEL")]
    for n, order in SHAPES:
        for fname, fkw in fixed:
            for gname, g in flags:
                yield "%d/%d %s %s" % (n, order, fname, gname), n, order, fkw, g


def calls(args):
    np, torch, _capi = load(args.root)
    dev = torch.device("cuda:0")
    log = open(args.log, "w") if args.log else sys.stdout
    with _capi.Handle(0, hooks=True) as h:  # (the hooks build: the product's objects + flacenc_hip_debug_scratch_bytes)
        for name, n, order, fkw, g in grid(_capi):
            stride = (n + 3) & ~3
            host = {}
            for ch in (2, 3):  # (the 1-channel call takes the first rows of the 3-channel signal)
                x = _capi.sigen_frames(FRAMES, ch, n, BPS, 200.0, 0.4, 0.4, seed=0xF1AC0000 + n)
                x[2] &= ~3  # two frames with wasted bits in every channel
                x[5] &= ~15
                padded = np.zeros((FRAMES, ch, stride), np.int32)
                padded[:, :, :n] = x
                host[ch] = torch.from_numpy(padded).to(dev)
            cfg = _capi.make_frame_config(_capi.make_config(lpc_order=order, flags=g), **fkw)
            fused = _capi.make_frame_config(_capi.make_config(lpc_order=order, flags=g | _capi.FLAG_FUSED_PACK), **fkw)
            bound = h.frame_bytes_bound(n, BPS)
            out = {"res": torch.zeros(FRAMES * 8 * 752, dtype=torch.uint8, device=dev),
                   "rows": torch.zeros(FRAMES * 4 * stride, dtype=torch.int32, device=dev),
                   "keys": torch.zeros(FRAMES * 4, dtype=torch.int64, device=dev),
                   "bytes": torch.zeros(FRAMES * bound, dtype=torch.uint8, device=dev),
                   "lens": torch.zeros(FRAMES, dtype=torch.int32, device=dev)}
            p = {k: v.data_ptr() for k, v in out.items()}
            s2, s3 = host[2].data_ptr(), host[3].data_ptr()
            entries = [
                ("encode_stereo_frames", lambda: h.encode_stereo_frames_device(cfg, s2, FRAMES, n, stride, BPS, p["res"], p["rows"], stride)),
                ("encode_frames_1", lambda: h.encode_frames_device(cfg, s3, FRAMES, 1, n, stride, BPS, p["res"], p["rows"], stride)),
                ("encode_frames_3", lambda: h.encode_frames_device(cfg, s3, FRAMES, 3, n, stride, BPS, p["res"], p["rows"], stride)),
                ("encode_pack_stereo", lambda: h.encode_pack_stereo_frames_device(cfg, s2, FRAMES, n, stride, BPS, 44100, 0, 1, p["res"], p["bytes"], bound, p["lens"])),
                ("encode_pack_stereo_fused", lambda: h.encode_pack_stereo_frames_device(fused, s2, FRAMES, n, stride, BPS, 44100, 0, 1, p["res"], p["bytes"], bound, p["lens"])),
                ("qlpc_batch", lambda: h.qlpc_batch_device(cfg.qlpc, s3, FRAMES * 3, n, stride, 0, p["res"], p["rows"], stride)),
                ("stereo_qlpc_batch", lambda: h.stereo_qlpc_batch_device(cfg.qlpc, s2, FRAMES, n, stride, BPS, p["res"], p["rows"], stride)),
                ("fixed_lpc_batch", lambda: h.fixed_lpc_batch_device(cfg, s2, FRAMES, n, stride, None, BPS, _capi.LAYOUT_STEREO_FRAMES, p["res"], p["rows"], stride, p["keys"])),
            ]
            for entry, run in entries:
                for t in out.values():
                    t.zero_()
                torch.cuda.synchronize()
                try:
                    run()
                    rc = 0
                except _capi.FlacencHipError as e:
                    rc = e.code
                h.synchronize()
                torch.cuda.synchronize()
                crc = 0
                for k in sorted(out):
                    crc = zlib.crc32(out[k].cpu().numpy().tobytes(), crc)
                log.write("%s %s rc %d crc %08x scratch %d\n" % (name, entry, rc, crc, h.debug_scratch_bytes()[0]))
    log.close()


def compact(launches, out=sys.stdout):
    """The ordered launches, lossless and small: the table of distinct (kernel, grid, workgroup), then the sequence as
    indices into it, 24 to a line."""
    table = {}
    ids = [table.setdefault(x, len(table)) for x in launches]
    out.write("# %d launches, %d distinct (kernel, grid, workgroup)\n" % (len(ids), len(table)))
    for x, i in table.items():
        out.write("k%d %s\n" % (i, x))
    for at in range(0, len(ids), 24):
        out.write("s %s\n" % " ".join(str(i) for i in ids[at:at + 24]))


def sequence(args):
    rows = list(csv.DictReader(open(args.csv)))
    rows.sort(key=lambda r: int(r["Dispatch_Id"]))
    # (the driver's own torch kernels -- clearing the outputs between calls -- are not the library's)
    compact(["%s grid %s,%s,%s workgroup %s,%s,%s" % (
        r["Kernel_Name"], r["Grid_Size_X"], r["Grid_Size_Y"], r["Grid_Size_Z"], r["Workgroup_Size_X"],
        r["Workgroup_Size_Y"], r["Workgroup_Size_Z"]) for r in rows if "at::native" not in r["Kernel_Name"]])


def launches(args):
    np, torch, _capi = load(args.root)
    dev = torch.device("cuda:0")
    n, order = 4096, 8
    x = torch.from_numpy(_capi.sigen_frames(FRAMES, 2, n, BPS, 200.0, 0.4, 0.4, seed=0xF1AC0001)).to(dev)
    res = torch.zeros(FRAMES * 752, dtype=torch.uint8, device=dev)
    rows = torch.zeros(FRAMES * 2 * n, dtype=torch.int32, device=dev)
    cfg = _capi.make_frame_config(_capi.make_config(lpc_order=order))
    series = []
    with _capi.Handle(0) as h:
        def burst(k):
            for _ in range(k):
                h.encode_stereo_frames_device(cfg, x.data_ptr(), FRAMES, n, n, BPS, res.data_ptr(), rows.data_ptr(), n)
            h.synchronize()
        burst(200)  # warm-up: window cache, scratch, the order mode's buffers
        for _ in range(args.repeat):
            t0 = time.perf_counter()
            burst(args.calls)
            series.append((time.perf_counter() - t0) * 1e6 / args.calls)
    print(json.dumps({"root": os.path.abspath(args.root), "calls": args.calls, "us_per_call": series}))


def main():
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="mode", required=True)
    a = sub.add_parser("calls")
    a.add_argument("--root", default=here)
    a.add_argument("--log")
    a.set_defaults(fn=calls)
    a = sub.add_parser("sequence")
    a.add_argument("csv")
    a.set_defaults(fn=sequence)
    a = sub.add_parser("launches")
    a.add_argument("--root", default=here)
    a.add_argument("--calls", type=int, default=2000)
    a.add_argument("--repeat", type=int, default=5)
    a.set_defaults(fn=launches)
    args = ap.parse_args()
    args.fn(args)


if __name__ == "__main__":
    main()
