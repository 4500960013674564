"""Cost and gain of FLACENC_HIP_FLAG_ORDER_SEARCH -> profiles/order_search_rates.json (same box, same process, A/B).

  bench workload   98 304 stereo frames x 4096 16-bit samples (bench.py's shape and material), encode + pack
                   (flacenc_hip_encode_pack_stereo_frames_async): ms at LPC order 8 and 12, flag off / on; bytes off / on
                   and the histogram of the chosen orders (records of the LPC subframes coded)
  big blocks       24-bit stereo frames of 8192 and 16384 samples at order 32 (ALLOW_ORDER_32): ms off / on
  golden fixtures  the real-audio fixtures (tests/golden testsignal.*, tiled as tests/test_gpu_wasted_bits.content does)
                   at orders 8, 12 and 32: bytes off / on, chosen-order histogram

    python tools/time_order_search.py [--frames 98304] [--reps 5] [--out profiles/order_search_rates.json]
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


def histogram(p):
    """Chosen LPC orders of the coded LPC subframes of the last call -> {order: count}."""
    res = p.res.cpu().numpy().view(_capi.FRAME_RESULT_DTYPE)
    orders = res["lpc"]["order"][res["kind"] == 3]
    return {int(o): int(c) for o, c in enumerate(np.bincount(orders)) if c}


def golden(n_frames, b=4096):
    names = ("ras103", "ras22", "sus109", "sus6")
    ch = [np.concatenate([util.test_signal(nm, c) for nm in names]) for c in range(2)]
    total = n_frames * b
    x = np.stack([np.tile(c, total // len(c) + 1)[:total] for c in ch])
    return np.ascontiguousarray(x.reshape(2, n_frames, b).transpose(1, 0, 2).astype(np.int32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=98304)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "order_search_rates.json"))
    args = ap.parse_args()
    OS = _capi.FLAG_ORDER_SEARCH
    F, n = args.frames, 4096
    rec = {"frames": F, "block_size": n, "reps": args.reps, "device": torch.cuda.get_device_name(0)}
    with _capi.Handle(0) as h:
        host = _capi.sigen_frames(F, 2, n, 16, 200.0, 0.4, 0.4, seed=0xF1AC0001)
        x = torch.from_numpy(host).cuda()
        p = Packer(h, x, 16)
        samples = F * n * 2
        rows = []
        for order in (8, 12):
            off, _ = timed(lambda: p(cfg_of(0, order)), args.reps)
            on, on_wall = timed(lambda: p(cfg_of(OS, order)), args.reps)
            b_off = p.total_bytes(cfg_of(0, order))
            b_on = p.total_bytes(cfg_of(OS, order))
            row = {"lpc_order": order, "flag_off_ms": off, "flag_on_ms": on, "flag_on_wall_ms": on_wall,
                   "flag_off_gsps": round(samples / off / 1e6, 2), "flag_on_gsps": round(samples / on / 1e6, 2),
                   "bytes_flag_off": b_off, "bytes_flag_on": b_on, "chosen_orders": histogram(p)}
            rows.append(row)
            print(json.dumps(row), flush=True)
        rec["bench_workload"] = rows
        del p, x
        torch.cuda.empty_cache()
        big = []
        for b in (8192, 16384):
            nf = F * n // b // 4  # a quarter of the bench workload's samples
            xb = torch.from_numpy(_capi.sigen_frames(nf, 2, b, 24, 200.0, 0.4, 0.4, seed=0xF1AC0002)).cuda()
            p = Packer(h, xb, 24)
            off, _ = timed(lambda: p(cfg_of(0, 32)), args.reps)
            on, _ = timed(lambda: p(cfg_of(OS, 32)), args.reps)
            row = {"block_size": b, "frames": nf, "bits": 24, "lpc_order": 32, "flag_off_ms": off, "flag_on_ms": on,
                   "flag_off_gsps": round(nf * b * 2 / off / 1e6, 2), "flag_on_gsps": round(nf * b * 2 / on / 1e6, 2),
                   "bytes_flag_off": p.total_bytes(cfg_of(0, 32)), "bytes_flag_on": p.total_bytes(cfg_of(OS, 32)),
                   "chosen_orders": histogram(p)}
            big.append(row)
            print(json.dumps(row), flush=True)
            del p, xb
            torch.cuda.empty_cache()
        rec["big_blocks"] = big
        g = torch.from_numpy(golden(64)).cuda()
        p = Packer(h, g, 16)
        gold = []
        for order in (8, 12, 32):
            row = {"lpc_order": order, "frames": 64, "bytes_flag_off": p.total_bytes(cfg_of(0, order)),
                   "bytes_flag_on": p.total_bytes(cfg_of(OS, order)), "chosen_orders": histogram(p)}
            gold.append(row)
            print(json.dumps(row), flush=True)
        rec["golden_fixtures"] = gold
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
