"""Cost and gain of FLACENC_HIP_FLAG_WINDOW_SEARCH -> profiles/window_search_rates.json (same box, same process, A/B).

  bench workload   98 304 stereo frames x 4096 16-bit samples (bench.py's shape and material), encode + pack
                   (flacenc_hip_encode_pack_stereo_frames_async), no fixed candidate, at LPC orders 8 and 12 in four modes:
                   flag off, the flag with no extra window, the default extra windows, the default extra windows with
                   FLACENC_HIP_FLAG_ORDER_SEARCH -- ms, G samples/s, bytes; and REFERENCE_SUM_ORDER (what the flag without
                   extra windows is) and ORDER_SEARCH alone for comparison
  per candidate    order 8: seven extra windows (8 candidates per subframe) against ORDER_SEARCH (8 candidates)
  24-bit           12 288 stereo frames x 8192 samples at order 32 (ALLOW_ORDER_32), the default list: ms off / on
  golden fixtures  the real-audio fixtures (tests/golden testsignal.*, tiled) at orders 8, 12 and 32: bytes off, with
                   ORDER_SEARCH, with the default list, with both (the DESIGN.md 4.10 table's rows)

    python tools/time_window_search.py [--frames 98304] [--reps 3] [--out profiles/window_search_rates.json]
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
from time_order_search import Packer, cfg_of, golden, timed  # noqa: E402

SEVEN = _capi.DEFAULT_LPC_WINDOWS + ((_capi.WINDOW_PARTIAL_TUKEY, 1.0, 16384, 49152),
                                     (_capi.WINDOW_PUNCHOUT_TUKEY, 0.0, 100, 65000))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=98304)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "window_search_rates.json"))
    args = ap.parse_args()
    WS, OS, REF = _capi.FLAG_WINDOW_SEARCH, _capi.FLAG_ORDER_SEARCH, _capi.FLAG_REFERENCE_SUM_ORDER
    F, n = args.frames, 4096
    rec = {"frames": F, "block_size": n, "reps": args.reps, "device": torch.cuda.get_device_name(0),
           "default_windows": [list(e) for e in _capi.DEFAULT_LPC_WINDOWS]}
    # one handle per extra-window list: the flagged calls of a mode take that handle's list
    with _capi.Handle(0) as h_def, _capi.Handle(0) as h_none, _capi.Handle(0) as h_seven:
        h_none.set_lpc_windows([])
        h_seven.set_lpc_windows(SEVEN)
        host = _capi.sigen_frames(F, 2, n, 16, 200.0, 0.4, 0.4, seed=0xF1AC0001)
        x = torch.from_numpy(host).cuda()
        samples = F * n * 2
        modes = [("flag_off", h_def, 0), ("reference_sum_order", h_def, REF), ("zero_extras", h_none, WS),
                 ("default_list", h_def, WS), ("default_list_order_search", h_def, WS | OS), ("order_search", h_def, OS)]
        rows = []
        for order in (8, 12):
            for name, hh, flags in modes:
                p = Packer(hh, x, 16)
                ms, wall = timed(lambda: p(cfg_of(flags, order)), args.reps)
                row = {"lpc_order": order, "mode": name, "ms": ms, "wall_ms": wall,
                       "gsps": round(samples / ms / 1e6, 2), "bytes": p.total_bytes(cfg_of(flags, order))}
                rows.append(row)
                print(json.dumps(row), flush=True)
                del p
        rec["bench_workload"] = rows
        cand = []
        for name, hh, flags in (("seven_extra_windows", h_seven, WS), ("order_search", h_def, OS)):
            p = Packer(hh, x, 16)
            ms, wall = timed(lambda: p(cfg_of(flags, 8)), args.reps)
            row = {"lpc_order": 8, "mode": name, "candidates_per_subframe": 8, "ms": ms,
                   "gsps": round(samples / ms / 1e6, 2), "bytes": p.total_bytes(cfg_of(flags, 8))}
            cand.append(row)
            print(json.dumps(row), flush=True)
            del p
        cand.append({"ratio_windows_to_orders": round(cand[0]["ms"] / cand[1]["ms"], 3)})
        print(json.dumps(cand[-1]), flush=True)
        rec["per_candidate"] = cand
        del x
        torch.cuda.empty_cache()
        nf, b = 12288, 8192
        xb = torch.from_numpy(_capi.sigen_frames(nf, 2, b, 24, 200.0, 0.4, 0.4, seed=0xF1AC0002)).cuda()
        p = Packer(h_def, xb, 24)
        off, _ = timed(lambda: p(cfg_of(0, 32)), args.reps)
        on, _ = timed(lambda: p(cfg_of(WS, 32)), args.reps)
        row = {"block_size": b, "frames": nf, "bits": 24, "lpc_order": 32, "flag_off_ms": off, "flag_on_ms": on,
               "flag_off_gsps": round(nf * b * 2 / off / 1e6, 2), "flag_on_gsps": round(nf * b * 2 / on / 1e6, 2),
               "bytes_flag_off": p.total_bytes(cfg_of(0, 32)), "bytes_flag_on": p.total_bytes(cfg_of(WS, 32))}
        rec["big_blocks_24bit"] = row
        print(json.dumps(row), flush=True)
        del p, xb
        torch.cuda.empty_cache()
        g = torch.from_numpy(golden(64)).cuda()
        p = Packer(h_def, g, 16)
        gold = []
        for order in (8, 12, 32):
            row = {"lpc_order": order, "frames": 64, "bytes_flag_off": p.total_bytes(cfg_of(0, order)),
                   "bytes_reference_sum_order": p.total_bytes(cfg_of(REF, order)),
                   "bytes_order_search": p.total_bytes(cfg_of(OS, order)),
                   "bytes_window_search": p.total_bytes(cfg_of(WS, order)),
                   "bytes_both": p.total_bytes(cfg_of(WS | OS, order))}
            gold.append(row)
            print(json.dumps(row), flush=True)
        rec["golden_fixtures"] = gold
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
