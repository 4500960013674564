"""Cost and gain of FLACENC_HIP_FLAG_WASTED_BITS -> profiles/wasted_bits_rates.json (same box, same process, A/B).

  bench workload   98 304 stereo frames x 4096 16-bit samples, LPC order 8 (bench.py's shape and material): ms of
                   flacenc_hip_encode_pack_stereo_frames_async without and with the flag (the flag adds the scan and one
                   host synchronisation; no frame has wasted bits, so the same kernels follow)
  wasted material  the same content << 8 at 24 bits: ms without the flag, with it (every frame goes through the fix-up:
                   shift, the candidate batches, the deciding kernel, the packer), and with FLACENC_HIP_FLAG_GENERIC_KERNEL
                   alone (the candidate batches' speed on the unshifted input); bytes without and with the flag
  golden fixtures  the real-audio fixtures (tests/golden testsignal.*, 16-bit) at 16 bits, << 4 at 20, << 8 at 24: bytes
                   without and with the flag

    python tools/time_wasted_bits.py [--frames 98304] [--reps 7] [--out profiles/wasted_bits_rates.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from flacenc_rs_amd import _capi  # noqa: E402
import util  # noqa: E402


def timed(fn, reps):
    """Median ms of fn() on the current stream (events around each repetition, after one warm-up) and median wall ms."""
    fn()
    torch.cuda.synchronize()
    ms, wall = [], []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        ms.append(a.elapsed_time(b))
    return round(float(np.median(ms)), 4), round(float(np.median(wall)), 4)


class Packer:
    def __init__(self, h, x, bps):
        self.h, self.x, self.bps = h, x, bps
        self.n, _, self.b = x.shape
        self.slot = h.frame_bytes_bound(self.b, bps)
        self.out = torch.empty(self.n * self.slot, dtype=torch.uint8, device="cuda")
        self.ln = torch.zeros(self.n, dtype=torch.int32, device="cuda")
        self.res = torch.empty(self.n * 752, dtype=torch.uint8, device="cuda")

    def __call__(self, cfg):
        self.h.encode_pack_stereo_frames_device(cfg, self.x.data_ptr(), self.n, self.b, self.b, self.bps, 44100, 0, 1,
                                                self.res.data_ptr(), self.out.data_ptr(), self.slot, self.ln.data_ptr(),
                                                torch.cuda.current_stream().cuda_stream)

    def total_bytes(self, cfg):
        self(cfg)
        torch.cuda.synchronize()
        return int(self.ln.sum().item())


def cfg_of(flags, order=8):
    return _capi.make_frame_config(_capi.make_config(lpc_order=order, flags=flags))  # (bench.py's: use_fixed off)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=98304)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wasted_bits_rates.json"))
    args = ap.parse_args()
    W, G = _capi.FLAG_WASTED_BITS, _capi.FLAG_GENERIC_KERNEL
    F, n = args.frames, 4096
    samples = F * n * 2
    gsps = lambda ms: round(samples / ms / 1e6, 2)  # noqa: E731
    rec = {"frames": F, "block_size": n, "lpc_order": 8, "reps": args.reps, "device": torch.cuda.get_device_name(0)}
    with _capi.Handle(0) as h:
        host = _capi.sigen_frames(F, 2, n, 16, 200.0, 0.4, 0.4, seed=0xF1AC0001)
        x = torch.from_numpy(host).cuda()
        p = Packer(h, x, 16)
        off, off_wall = timed(lambda: p(cfg_of(0)), args.reps)
        on, on_wall = timed(lambda: p(cfg_of(W)), args.reps)
        assert p.total_bytes(cfg_of(0)) == p.total_bytes(cfg_of(W))
        rec["bench_workload"] = {"flag_off_ms": off, "flag_on_ms": on, "flag_off_wall_ms": off_wall,
                                 "flag_on_wall_ms": on_wall, "flag_off_gsps": gsps(off), "flag_on_gsps": gsps(on),
                                 "slowdown": round(on / off - 1.0, 4), "slowdown_wall": round(on_wall / off_wall - 1.0, 4)}
        print(json.dumps(rec["bench_workload"]), flush=True)
        del p
        x24 = torch.from_numpy(host.astype(np.int32) << 8).cuda()
        del x
        p = Packer(h, x24, 24)
        off, _ = timed(lambda: p(cfg_of(0)), args.reps)
        gen, _ = timed(lambda: p(cfg_of(G)), args.reps)
        on, on_wall = timed(lambda: p(cfg_of(W)), args.reps)
        b_off, b_on = p.total_bytes(cfg_of(0)), p.total_bytes(cfg_of(W))
        rec["wasted_material"] = {"content": "bench workload << 8 at 24 bits", "flag_off_ms": off, "flag_on_ms": on,
                                  "flag_on_wall_ms": on_wall, "generic_kernel_ms": gen, "flag_off_gsps": gsps(off),
                                  "flag_on_gsps": gsps(on), "generic_kernel_gsps": gsps(gen), "bytes_flag_off": b_off,
                                  "bytes_flag_on": b_on, "size_ratio_off_over_on": round(b_off / b_on, 4)}
        print(json.dumps(rec["wasted_material"]), flush=True)
        del p, x24
        torch.cuda.empty_cache()
        gold = []
        for name in ("ras103", "ras22", "sus109", "sus6"):
            l, r = util.test_signal(name, 0), util.test_signal(name, 1)
            gold += [np.stack([l[f * n:(f + 1) * n], r[f * n:(f + 1) * n]]) for f in range(len(l) // n)]
        g = np.stack(gold).astype(np.int32)
        rows = []
        for shift, bps in ((0, 16), (4, 20), (8, 24)):
            p = Packer(h, torch.from_numpy(g << shift).cuda(), bps)
            rows.append({"content": f"<< {shift} at {bps} bits", "frames": len(g),
                         "bytes_flag_off": p.total_bytes(cfg_of(0)), "bytes_flag_on": p.total_bytes(cfg_of(W))})
        rec["golden_fixtures"] = rows
        print(json.dumps(rows), flush=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
