"""Cost and gain of the block-size search (flacenc_hip_encode_variable_async) -> profiles/variable_block_rates.json.

  bench workload   98 304 stereo superblocks x 4096 16-bit samples, LPC order 8 (bench.py's shape), levels 1..4: ms of the
                   whole call, G samples/s (channel samples, as bench.py counts), ms of each level's encode+pack call alone
                   at that level's block size (what the search runs per level), the rest (reblock, decide, scans, rehead)
                   as the difference, the share of the call spent packing frames that are not chosen, and the bytes
                   against the fixed 4096-sample stream
  real audio       the golden fixtures (tests/golden testsignal.*) tiled to a batch: bytes at levels 1..4 against fixed
                   blocking at 4096, 2048 and 1024

    python tools/time_variable_block.py [--frames 98304] [--reps 5] [--out profiles/variable_block_rates.json]
    (--quick: level 4 only, two repetitions -- the shape tools/README.md profiles under rocprofv3)
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from flacenc_rs_amd import _capi  # noqa: E402


def timed(fn, reps):
    """Median ms of fn() on the current stream (events around each repetition, after one warm-up)."""
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms))


class Variable:
    """Device buffers for one search shape."""

    def __init__(self, h, cfg, x_dev, total, channels, S, levels, bps):
        self.h, self.cfg, self.x, self.total, self.C, self.S, self.L, self.bps = h, cfg, x_dev, total, channels, S, levels, bps
        self.cap = _capi.variable_bytes_bound(channels, S, levels, bps, total)
        self.mf = _capi.variable_max_frames(S, levels, total)
        self.out = torch.empty(self.cap, dtype=torch.uint8, device="cuda")
        self.off = torch.empty(self.mf, dtype=torch.int64, device="cuda")
        self.ln = torch.empty(self.mf, dtype=torch.int32, device="cuda")
        self.bs = torch.empty(self.mf, dtype=torch.int32, device="cuda")
        self.masks = torch.empty((total + S - 1) // S, dtype=torch.int32, device="cuda")
        self.tot = torch.zeros(2, dtype=torch.int64, device="cuda")

    def __call__(self):
        self.h.encode_variable_device(self.cfg, self.x.data_ptr(), self.total, self.C, self.S, self.L, self.S, self.bps,
                                      44100, 0, self.out.data_ptr(), self.cap, self.off.data_ptr(), self.ln.data_ptr(),
                                      self.bs.data_ptr(), self.mf, self.masks.data_ptr(), self.tot.data_ptr(),
                                      torch.cuda.current_stream().cuda_stream)

    def result(self):
        torch.cuda.synchronize()
        t = self.tot.cpu().numpy().view(np.uint64)
        bs = self.bs.cpu().numpy()[:int(t[0])]
        return int(t[0]), int(t[1]), {int(b): int((bs == b).sum()) for b in np.unique(bs)}


def fixed_pack(h, cfg, x_dev, n, channels, b, bps):
    """One fixed-blocking encode+pack call over n frames of b samples -> (callable, total bytes after a run)."""
    slot = h.frame_bytes_bound(b, bps) if channels == 2 else h.frame_bytes_bound_channels(channels, b, bps)
    out = torch.empty(n * slot, dtype=torch.uint8, device="cuda")
    ln = torch.zeros(n, dtype=torch.int32, device="cuda")
    res = torch.empty(n * (752 if channels == 2 else 368 * channels), dtype=torch.uint8, device="cuda")

    def run():
        s = torch.cuda.current_stream().cuda_stream
        if channels == 2:
            h.encode_pack_stereo_frames_device(cfg, x_dev.data_ptr(), n, b, b, bps, 44100, 0, 1, res.data_ptr(),
                                               out.data_ptr(), slot, ln.data_ptr(), s)
        else:
            h.encode_pack_frames_device(cfg, x_dev.data_ptr(), n, channels, b, b, bps, 44100, 0, 1, res.data_ptr(),
                                        out.data_ptr(), slot, ln.data_ptr(), s)

    def total():
        torch.cuda.synchronize()
        return int(ln.cpu().numpy().astype(np.int64).sum())
    return run, total


def bench_workload(h, n_sb, reps, levels_list):
    S, C, bps = 4096, 2, 16
    cfg = _capi.make_frame_config(_capi.make_config(lpc_order=8))
    x = _capi.sigen_frames(n_sb, C, S, bps, 200.0, 0.4, 0.3, seed=0xBE4C)
    xd = torch.from_numpy(x).cuda()
    samples = n_sb * S * C
    rows, level_ms = [], {}
    fixed_bytes = None
    for L in levels_list:
        # each level's encode+pack alone on that level's frames (the search's own cut of the input)
        for k in range(L):
            if k in level_ms:
                continue
            b = S >> k
            xk = xd.reshape(n_sb, C, 1 << k, b).permute(0, 2, 1, 3).contiguous().reshape(n_sb << k, C, b)
            run, total = fixed_pack(h, cfg, xk, n_sb << k, C, b, bps)
            level_ms[k] = timed(run, reps)
            run()
            if k == 0:
                fixed_bytes = total()
            del xk
        v = Variable(h, cfg, xd, n_sb * S, C, S, L, bps)
        ms = timed(v, reps)
        frames, nbytes, blocks = v.result()
        enc = sum(level_ms[k] for k in range(L))
        # frames packed but not chosen: every level's frames are packed, the chosen ones cover the input once
        chosen_share = {k: sum(n for b, n in blocks.items() if b == S >> k) * (S >> k) / (n_sb * S) for k in range(L)}
        unchosen_ms = sum(level_ms[k] * (1.0 - chosen_share[k]) for k in range(L))
        rows.append(dict(levels=L, ms=round(ms, 3), gsamples_per_s=round(samples / ms / 1e6, 1),
                         level_encode_pack_ms={S >> k: round(level_ms[k], 3) for k in range(L)},
                         rest_ms=round(ms - enc, 3), unchosen_encode_pack_share=round(unchosen_ms / ms, 3),
                         frames=frames, bytes=nbytes, fixed_4096_bytes=fixed_bytes,
                         bytes_vs_fixed=round(nbytes / fixed_bytes, 6), block_sizes=blocks))
        print(json.dumps(rows[-1]), flush=True)
        del v
        torch.cuda.empty_cache()
    return dict(shape=dict(superblocks=n_sb, block_size=S, channels=C, bps=bps, lpc_order=8, use_fixed=False), levels=rows)


def real_audio(h, tiles):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import util
    C, bps, S = 2, 16, 4096
    cfg = _capi.make_frame_config(_capi.make_config(lpc_order=8), use_fixed=True)
    one = np.stack([np.concatenate([util.test_signal(nm, c) for nm in ("ras103", "ras22", "sus109")]) for c in (0, 1)],
                   axis=1)
    pcm = np.tile(one, (tiles, 1))
    total = len(pcm)
    out = dict(samples=total, tiles=tiles, fixed={}, variable={})
    for b in (4096, 2048, 1024):
        n = total // b  # (the fixtures tile to whole blocks of all three sizes)
        xb = torch.from_numpy(np.ascontiguousarray(pcm[:n * b].reshape(n, b, C).transpose(0, 2, 1))).cuda()
        run, tot = fixed_pack(h, cfg, xb, n, C, b, bps)
        run()
        out["fixed"][b] = tot()
    xs = torch.from_numpy(np.ascontiguousarray(pcm.reshape(-1, S, C).transpose(0, 2, 1))).cuda()
    for L in (1, 2, 3, 4):
        v = Variable(h, cfg, xs, total, C, S, L, bps)
        v()
        frames, nbytes, blocks = v.result()
        out["variable"][L] = dict(bytes=nbytes, frames=frames, block_sizes=blocks,
                                  vs_fixed_4096=round(nbytes / out["fixed"][4096], 6),
                                  vs_fixed_2048=round(nbytes / out["fixed"][2048], 6),
                                  vs_fixed_1024=round(nbytes / out["fixed"][1024], 6))
        print(L, json.dumps(out["variable"][L]), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=98304)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--tiles", type=int, default=64)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    with _capi.Handle(0) as h:
        if args.quick:
            bench_workload(h, args.frames, 2, [4])
            return
        res = dict(bench_workload=bench_workload(h, args.frames, args.reps, [1, 2, 3, 4]),
                   real_audio=real_audio(h, args.tiles), device=torch.cuda.get_device_name(0))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
