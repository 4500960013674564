"""Times flacenc_hip_decode_ranges_planar (device memory, float32) against what a training loop had to do without it:
flacenc_hip_decode_ranges into 2-byte packed PCM, then the shortest torch sequence that gives the same [B, C, T] float32
tensor -- one torch.mul of the int16 view, permuted, into a preallocated contiguous tensor.

The two workloads of DESIGN.md section 4.21:
  streams     one crop of 16 000 samples from each of 2 048 mono 16-bit streams of 40 frames of 4096 samples
  one_large   256 crops of 16 000 samples of one stereo stream of 24 576 frames of 4096 samples
Everything lives in device memory; both paths are warmed, then timed alternately in this one process, wall clock around
the blocking call (and torch.cuda.synchronize() behind the torch step); the figure is the median of --reps calls.  The two
tensors are compared bit for bit before anything is timed.  Writes profiles/decode_ranges_planar_rates.json.

    python tools/time_decode_ranges_planar.py
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from flacenc_rs_amd import _capi  # noqa: E402
from time_decode_streams import encode  # noqa: E402

CROP = 16000
PLAN = ("launches", "synchronisations", "transfers", "channel_classes")


def measure(h, name, everything, table, stream_of, firsts, channels, max_frames, reps):
    import torch
    dev = torch.device("cuda:0")
    B = len(firsts)
    ranges = np.zeros(B, _capi.RANGE_DESC_DTYPE)
    ranges["first_sample"] = firsts
    ranges["n_samples"] = CROP
    ranges["stream"] = stream_of
    packed_ranges, planar_ranges = ranges.copy(), ranges.copy()
    packed_ranges["out_offset"] = np.arange(B, dtype=np.uint64) * np.uint64(CROP * channels * 2)
    planar_ranges["out_offset"] = np.arange(B, dtype=np.uint64) * np.uint64(CROP * channels * 4)
    d_in = torch.from_numpy(everything).to(dev)
    d_packed = torch.zeros(B * CROP * channels, dtype=torch.int16, device=dev)
    d_base = torch.zeros((B, channels, CROP), dtype=torch.float32, device=dev)
    d_planar = torch.zeros((B, channels, CROP), dtype=torch.float32, device=dev)
    d_tot = torch.zeros((B, 4), dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    state = {}

    def packed_only():
        state["call"], _ = h.decode_ranges_device(d_in.data_ptr(), d_in.numel(), table, packed_ranges, max_frames,
                                                  d_packed.data_ptr(), d_packed.numel() * 2, d_tot.data_ptr())

    def baseline():
        packed_only()
        torch.mul(d_packed.view(B, CROP, channels).permute(0, 2, 1), 1.0 / 32768.0, out=d_base)
        torch.cuda.synchronize()

    def planar():
        state["call"], _ = h.decode_ranges_planar_device(d_in.data_ptr(), d_in.numel(), table, planar_ranges, max_frames,
                                                         d_planar.data_ptr(), d_planar.numel() * 4, _capi.SAMPLE_F32,
                                                         d_tot.data_ptr())

    for fn in (baseline, planar, baseline, planar):   # warm: scratch grown, torch's kernel loaded
        fn()
    assert state["call"][1] == B * CROP and bool((d_tot[:, 0] == CROP).all())
    assert torch.equal(d_base.view(torch.int32), d_planar.view(torch.int32)), name
    plans = {}
    packed_only()
    plans["decode_ranges"] = dict(zip(PLAN, h.debug_last_decode_ranges_plan()))
    planar()
    plans["decode_ranges_planar"] = dict(zip(PLAN, h.debug_last_decode_ranges_plan()))
    times = {"decode_ranges_alone": [], "decode_ranges_then_torch": [], "decode_ranges_planar": []}
    for _ in range(reps):
        for key, fn in (("decode_ranges_alone", packed_only), ("decode_ranges_then_torch", baseline),
                        ("decode_ranges_planar", planar)):
            t0 = time.perf_counter()
            fn()
            times[key].append(time.perf_counter() - t0)
    out = {"crops": B, "channels": channels, "crop_samples": B * CROP, "compressed_bytes": int(len(everything)),
           "frame_decodes": state["call"][0], "plans": plans, "reps": reps}
    for key, t in times.items():
        out[key] = {"median_ms": round(statistics.median(t) * 1e3, 3), "min_ms": round(min(t) * 1e3, 3),
                    "max_ms": round(max(t) * 1e3, 3)}
    out["planar_over_baseline"] = round(out["decode_ranges_planar"]["median_ms"] / out["decode_ranges_then_torch"]["median_ms"], 3)
    out["planar_over_decode_ranges_alone"] = round(out["decode_ranges_planar"]["median_ms"] / out["decode_ranges_alone"]["median_ms"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=2048)
    ap.add_argument("--distinct", type=int, default=64)
    ap.add_argument("--frames-per-stream", type=int, default=40)
    ap.add_argument("--block-size", type=int, default=4096)
    ap.add_argument("--large-frames", type=int, default=24576)
    ap.add_argument("--large-crops", type=int, default=256)
    ap.add_argument("--reps", type=int, default=24)
    ap.add_argument("--only", choices=("streams", "one_large"), help="run one workload (for a profiler)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decode_ranges_planar_rates.json"))
    args = ap.parse_args()
    assert args.reps >= 20, "the median of at least 20 calls"
    n, bps, per, D = args.block_size, 16, args.frames_per_stream, args.distinct
    h = _capi.Handle(0, hooks=True)
    res = {"what": "device memory, 16-bit streams of frames of %d samples, crops of %d samples at seeded random positions; "
                   "flacenc_hip_decode_ranges_planar (float32) against flacenc_hip_decode_ranges (2-byte samples) followed "
                   "by one torch.mul of the permuted int16 view into a contiguous [B, C, T] float32 tensor" % (n, CROP),
           "timing": "wall clock, warm, the three timed alternately in one process; median, min and max of `reps` calls"}
    if args.only != "one_large":
        count = args.streams
        data, lens, _ = encode(h, D * per, 1, n, bps, 0xF1AC0002)
        ends = np.concatenate([[0], np.cumsum(lens)])
        cuts = ends[::per]                        # stream s = bytes [cuts[s], cuts[s + 1])
        everything = np.tile(data, -(-count // D))
        table = np.zeros(count, _capi.STREAM_DESC_DTYPE)
        for s in range(count):
            table[s] = ((s // D) * len(data) + int(cuts[s % D]), int(cuts[s % D + 1] - cuts[s % D]), 0, 0, 1, bps, n, 2)
        firsts = np.random.default_rng(0xC509 + count).integers(0, per * n - CROP + 1, count)
        res["streams_%d" % count] = measure(h, "streams", everything, table, np.arange(count), firsts, 1, count * per,
                                            args.reps)
    if args.only != "streams":
        F, K = args.large_frames, args.large_crops
        big, _, _ = encode(h, F, 2, n, bps, 0xF1AC0001)
        table = np.zeros(1, _capi.STREAM_DESC_DTYPE)
        table[0] = (0, len(big), 0, 0, 2, bps, n, 2)
        firsts = np.random.default_rng(0xC50A).integers(0, F * n - CROP + 1, K)
        res["one_large"] = measure(h, "one_large", big, table, np.zeros(K, np.int64), firsts, 2, F, args.reps)
    h.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
