"""Cost and gain of FLACENC_HIP_FLAG_ORDER_GUESS -> profiles/order_guess_rates.json (same box, same process, A/B).

  bench workload   98 304 stereo frames x 4096 16-bit samples (bench.py's shape and material), encode + pack
                   (flacenc_hip_encode_pack_stereo_frames_async), no fixed candidate, at LPC orders 8 and 12:
                   REFERENCE_SUM_ORDER, ORDER_SEARCH, ORDER_GUESS at K = 1 / 2, and the same three with the default
                   extra-window list (WINDOW_SEARCH alone, with ORDER_SEARCH, with ORDER_GUESS at K = 1 / 2) -- ms,
                   G samples/s, bytes; per guessed row the expectation
                       t(GUESS) - t(REF) <= 1.15 (K W + 1) / (W P) (t(SEARCH) - t(REF))
                   with every term from this run (SEARCH: the exhaustive search over the same windows)
  24-bit           12 288 stereo frames x 8192 samples at order 32 (ALLOW_ORDER_32): the same modes without extra windows
  golden fixtures  the real-audio fixtures (tests/golden testsignal.*, tiled), 64 stereo frames x 4096 at orders 8, 12
                   and 32: bytes under REFERENCE_SUM_ORDER, ORDER_SEARCH, ORDER_GUESS at K = 1 / 2 / 4, with and without
                   the default list

    python tools/time_order_guess.py [--frames 98304] [--reps 3] [--out profiles/order_guess_rates.json]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from flacenc_rs_amd import _capi  # noqa: E402
from time_order_search import Packer, cfg_of, golden, histogram, timed  # noqa: E402

G, OS, WS, REF = _capi.FLAG_ORDER_GUESS, _capi.FLAG_ORDER_SEARCH, _capi.FLAG_WINDOW_SEARCH, _capi.FLAG_REFERENCE_SUM_ORDER
# (name, flags, K, windows W, which row is this row's exhaustive search)
MODES = [("reference_sum_order", REF, 0, 1, None), ("order_search", OS, 0, 1, None),
         ("order_guess_k1", G, 1, 1, "order_search"), ("order_guess_k2", G, 2, 1, "order_search"),
         ("window_search", WS, 0, 6, None), ("window_order_search", WS | OS, 0, 6, None),
         ("window_order_guess_k1", WS | G, 1, 6, "window_order_search"),
         ("window_order_guess_k2", WS | G, 2, 6, "window_order_search")]


def run_modes(h, x, bps, order, reps, modes, samples):
    rows = {}
    for name, flags, K, W, _ in modes:
        if K:
            h.set_order_guesses(K)
        p = Packer(h, x, bps)
        ms, wall = timed(lambda: p(cfg_of(flags, order)), reps)
        row = {"lpc_order": order, "mode": name, "ms": ms, "wall_ms": wall, "gsps": round(samples / ms / 1e6, 2),
               "bytes": p.total_bytes(cfg_of(flags, order))}
        if flags & (G | OS):
            row["chosen_orders"] = histogram(p)
        rows[name] = row
        del p
    ref = rows["reference_sum_order"]["ms"]
    for name, _, K, W, search in modes:
        if search is None or search not in rows:
            continue
        bound = 1.15 * (K * W + 1) / (W * order) * (rows[search]["ms"] - ref)
        rows[name]["over_reference_ms"] = round(rows[name]["ms"] - ref, 4)
        rows[name]["expected_at_most_ms"] = round(bound, 4)
        rows[name]["expectation_met"] = bool(rows[name]["ms"] - ref <= bound)
    for row in rows.values():
        print(json.dumps(row), flush=True)
    return list(rows.values())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=98304)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "order_guess_rates.json"))
    args = ap.parse_args()
    F, n = args.frames, 4096
    rec = {"frames": F, "block_size": n, "reps": args.reps, "device": torch.cuda.get_device_name(0),
           "default_windows": [list(e) for e in _capi.DEFAULT_LPC_WINDOWS]}
    with _capi.Handle(0) as h:
        x = torch.from_numpy(_capi.sigen_frames(F, 2, n, 16, 200.0, 0.4, 0.4, seed=0xF1AC0001)).cuda()
        rec["bench_workload"] = []
        for order in (8, 12):
            rec["bench_workload"] += run_modes(h, x, 16, order, args.reps, MODES, F * n * 2)
        del x
        torch.cuda.empty_cache()
        nf, b = max(1, F // 8), 8192
        xb = torch.from_numpy(_capi.sigen_frames(nf, 2, b, 24, 200.0, 0.4, 0.4, seed=0xF1AC0002)).cuda()
        rec["big_blocks_24bit"] = {"block_size": b, "frames": nf, "bits": 24,
                                   "rows": run_modes(h, xb, 24, 32, args.reps, MODES[:4], nf * b * 2)}
        del xb
        torch.cuda.empty_cache()
        p = Packer(h, torch.from_numpy(golden(64)).cuda(), 16)
        gold = []
        for order in (8, 12, 32):
            row = {"lpc_order": order, "frames": 64}
            for ws, tag in ((0, ""), (WS, "_default_list")):
                row["bytes_reference" + tag] = p.total_bytes(cfg_of((ws or REF), order))
                row["bytes_order_search" + tag] = p.total_bytes(cfg_of(ws | OS, order))
                for K in (1, 2, 4):
                    h.set_order_guesses(K)
                    row["bytes_order_guess_k%d%s" % (K, tag)] = p.total_bytes(cfg_of(ws | G, order))
            gold.append(row)
            print(json.dumps(row), flush=True)
        rec["golden_fixtures"] = gold
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
