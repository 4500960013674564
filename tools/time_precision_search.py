"""Cost and gain of FLACENC_HIP_FLAG_PRECISION_SEARCH -> profiles/precision_search_rates.json (same box, same process,
A/B).

  bench workload   bench.py's material (Sine(200, 0.4) + Noise(0.4), 16 bit, stereo) cut into blocks of 4096, 1152 and 256
                   samples -- the same number of samples at every block size, --frames frames at 4096 --, encode + pack
                   (flacenc_hip_encode_pack_stereo_frames_async), no fixed candidate, at LPC orders 8 and 12:
                   REFERENCE_SUM_ORDER, PRECISION_SEARCH at floors 5 and 10, ORDER_SEARCH, ORDER_SEARCH + PRECISION_SEARCH,
                   ORDER_GUESS + PRECISION_SEARCH (K = 1; the last two at floor 5) -- ms, G samples/s, bytes, and the
                   histogram of the chosen precisions (records of the LPC subframes coded)
  golden fixtures  the real-audio fixtures (tests/golden testsignal.*, tiled), the samples of 64 stereo frames x 4096 at
                   the three block sizes and orders 8, 12 and 32: bytes under the same modes
  variable blocks  flacenc_hip_encode_variable (host memory) at 3 levels from S = 4096 on the bench material, order 8,
                   with and without the flag: bytes and wall ms

    python tools/time_precision_search.py [--frames 98304] [--reps 3] [--out profiles/precision_search_rates.json]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
from flacenc_rs_amd import _capi  # noqa: E402
from time_order_search import Packer, cfg_of, golden, timed  # noqa: E402

PS, OS, G, REF = (_capi.FLAG_PRECISION_SEARCH, _capi.FLAG_ORDER_SEARCH, _capi.FLAG_ORDER_GUESS,
                  _capi.FLAG_REFERENCE_SUM_ORDER)
# (name, flags, floor)
MODES = [("reference_sum_order", REF, 5), ("precision_search_floor5", PS, 5), ("precision_search_floor10", PS, 10),
         ("order_search", OS, 5), ("order_precision_search", OS | PS, 5), ("order_guess_precision_search", G | PS, 5)]
BLOCKS = (4096, 1152, 256)


def precisions(p):
    """Chosen precisions of the coded LPC subframes of the last call -> {precision: count}."""
    res = p.res.cpu().numpy().view(_capi.FRAME_RESULT_DTYPE)
    q = res["lpc"]["precision"][res["kind"] == 3]
    return {int(o): int(c) for o, c in enumerate(np.bincount(q)) if c}


def reblock(x, b):
    """Stereo frames [F, 2, n] as one stream cut into blocks of b samples (the tail that fills no block dropped)."""
    flat = x.transpose(1, 0, 2).reshape(2, -1)
    nf = flat.shape[1] // b
    return np.ascontiguousarray(flat[:, :nf * b].reshape(2, nf, b).transpose(1, 0, 2))


def run_modes(h, x, order, reps, time_it=True):
    rows = []
    samples = x.shape[0] * x.shape[2] * 2
    p = Packer(h, x, 16)
    for name, flags, floor in MODES:
        h.set_precision_floor(floor)
        cfg = cfg_of(flags, order)
        row = {"block_size": int(x.shape[2]), "frames": int(x.shape[0]), "lpc_order": order, "mode": name}
        if flags & PS:
            row["floor"] = floor
        if time_it:
            ms, wall = timed(lambda: p(cfg), reps)
            row.update(ms=ms, wall_ms=wall, gsps=round(samples / ms / 1e6, 2))
        row["bytes"] = p.total_bytes(cfg)
        if flags & PS:
            row["chosen_precisions"] = precisions(p)
        rows.append(row)
    h.set_precision_floor(5)
    ref = rows[0]["bytes"]
    for row in rows:
        row["saving_percent"] = round(100.0 * (ref - row["bytes"]) / ref, 4)
        print(json.dumps(row), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=98304)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "precision_search_rates.json"))
    args = ap.parse_args()
    F = args.frames
    rec = {"frames_at_4096": F, "reps": args.reps, "device": torch.cuda.get_device_name(0)}
    with _capi.Handle(0) as h:
        host = _capi.sigen_frames(F, 2, 4096, 16, 200.0, 0.4, 0.4, seed=0xF1AC0001)
        rec["bench_workload"] = []
        for b in BLOCKS:
            x = torch.from_numpy(reblock(host, b)).cuda()
            for order in (8, 12):
                rec["bench_workload"] += run_modes(h, x, order, args.reps)
            del x
            torch.cuda.empty_cache()
        gold = golden(64)
        rec["golden_fixtures"] = []
        for b in BLOCKS:
            x = torch.from_numpy(reblock(gold, b)).cuda()
            for order in (8, 12, 32):
                rec["golden_fixtures"] += run_modes(h, x, order, args.reps, time_it=False)
            del x
        # the block-size search: the superblocks of an eighth of the workload, host memory both ways
        S, levels = 4096, 3
        sb = host[:max(4, F // 8)]
        rows = []
        for name, flags in (("reference_sum_order", REF), ("precision_search_floor5", PS)):
            cfg = cfg_of(flags, 8)
            h.encode_variable(sb, 16, cfg, levels)
            wall = []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                v = h.encode_variable(sb, 16, cfg, levels)
                wall.append((time.perf_counter() - t0) * 1e3)
            sizes = {int(s): int(c) for s, c in zip(*np.unique(v["block_sizes"], return_counts=True))}
            row = {"mode": name, "superblocks": int(len(sb)), "block_size": S, "levels": levels, "lpc_order": 8,
                   "wall_ms": round(float(np.median(wall)), 3), "bytes": int(v["bytes"]), "frames": int(v["frames"]),
                   "block_sizes": sizes}
            rows.append(row)
            print(json.dumps(row), flush=True)
        rec["encode_variable"] = rows
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
