"""Times flacenc_hip_encode_streams_planar (device memory, float32, digests and clip counts) against the way to the same
frames and digests without it: the torch passes -- mul, round, clamp, to(int16), permute + contiguous --, then
flacenc_hip_encode_streams on the packed PCM, then flacenc_hip_md5_spans over it.

The two workloads of the decode timings (DESIGN.md sections 4.21, 4.22), at 16 bits:
  streams     2 048 mono streams of 40 frames of 4096 samples, a [2048, 1, 163840] tensor
  one_large   one stereo stream of 24 576 frames of 4096 samples, a [1, 2, 100663296] tensor
Everything lives in device memory.  All rows are warmed, then timed in alternating rounds in this one process (composition,
planar, composition again, ...), wall clock around the blocking calls with torch.cuda.synchronize() behind the torch
passes; the figure is the median of --reps calls.  The composition is timed as two interleaved series: the distance of
their medians is the yardstick's own spread.  Frames, frame lengths, totals and digests of the two ways are compared
byte for byte before anything is timed.  Further rows: both ways without digests (the composition without its
flacenc_hip_md5_spans call, the planar call with digests = NULL), flacenc_hip_encode_streams alone on ready-made packed
PCM (what the tensor input costs over packed input), and the planar call with the fill kernel's other load form
(flacenc_hip_debug_set_planar_fill_form).  MD5 is serial inside one stream and a stream is hashed by one lane (about
90 MB/s), so the one stream of one_large takes seconds to hash on either way: its rows with digests are the median of
--large-digest-reps calls, its rows without digests of --reps.  Prints a line per round; writes
profiles/encode_streams_planar_rates.json.

    python tools/time_encode_streams_planar.py
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
from flacenc_rs_amd import _capi  # noqa: E402

BITS = 16


def measure(h, name, x, block, rate, cfg, reps, digest_reps):
    """x: float32 numpy [B, C, T], every item whole."""
    import torch
    dev = torch.device("cuda:0")
    B, C, T = x.shape
    lib = _capi.load()
    bound = int(lib.flacenc_hip_stereo_frame_bytes_bound(block, BITS) if C == 2 else lib.flacenc_hip_frame_bytes_bound(C, block, BITS))
    per = -(-T // block)
    cap = (per * (bound + 8) + 15) // 16 * 16
    F = B * per
    planar_table = np.zeros(B, _capi.PCM_STREAM_DESC_DTYPE)
    planar_table["offset"] = np.arange(B, dtype=np.uint64) * np.uint64(C * T * 4)
    planar_table["total_samples"] = T
    planar_table["out_offset"] = np.arange(B, dtype=np.uint64) * np.uint64(cap)
    planar_table["out_capacity"] = cap
    planar_table["channels"], planar_table["bits_per_sample"], planar_table["bytes_per_sample"] = C, BITS, 2
    planar_table["sample_rate"] = rate
    packed_table = planar_table.copy()
    packed_table["offset"] = np.arange(B, dtype=np.uint64) * np.uint64(C * T * 2)
    span_lengths = np.full(B, C * T * 2, np.uint64)
    d_x = torch.from_numpy(x).to(dev)
    d_packed = torch.zeros((B, T, C), dtype=torch.int16, device=dev)
    outs = [torch.zeros(B * cap, dtype=torch.uint8, device=dev) for _ in range(2)]
    lens = [torch.zeros(F, dtype=torch.int32, device=dev) for _ in range(2)]
    tots = [torch.zeros((B, 4), dtype=torch.int64, device=dev) for _ in range(2)]
    digs = [torch.zeros((B, 16), dtype=torch.uint8, device=dev) for _ in range(2)]
    d_clip = torch.zeros(B, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    state = {}

    def packed_only():
        state["packed"], _ = h.encode_streams_device(d_packed.data_ptr(), d_packed.numel() * 2, packed_table, cfg, block,
                                                     outs[0].data_ptr(), outs[0].numel(), lens[0].data_ptr(), F,
                                                     tots[0].data_ptr())

    def composition(digests=True):
        v = torch.clamp(torch.round(d_x * 32768.0), -32768.0, 32767.0).to(torch.int16)
        d_packed.copy_(v.permute(0, 2, 1))      # permute + contiguous, into the buffer the encoder reads
        torch.cuda.synchronize()
        packed_only()
        if digests:
            h.md5_spans_device(d_packed.data_ptr(), d_packed.numel() * 2, packed_table["offset"], span_lengths,
                               digs[0].data_ptr())

    def composition_no_digests():
        composition(False)

    def planar(digests=True):
        state["planar"], _ = h.encode_streams_planar_device(
            d_x.data_ptr(), d_x.numel() * 4, _capi.SAMPLE_F32, T, planar_table, cfg, block, outs[1].data_ptr(),
            outs[1].numel(), lens[1].data_ptr(), F, tots[1].data_ptr(), digs[1].data_ptr() if digests else 0, d_clip.data_ptr())

    def planar_no_digests():
        planar(False)

    def planar_dword_loads():
        h.debug_set_planar_fill_form(0)
        try:
            planar(False)
        finally:
            h.debug_set_planar_fill_form(1)

    for fn in (composition, planar, planar_dword_loads, composition_no_digests, planar_no_digests):   # warm: scratch grown, torch's kernels loaded
        fn()
        print(name, "warm", fn.__name__, flush=True)
    assert state["packed"] == state["planar"] and state["planar"][0] == F, name
    assert torch.equal(outs[0], outs[1]) and torch.equal(lens[0], lens[1]) and torch.equal(tots[0], tots[1]), name
    assert torch.equal(digs[0], digs[1]) and not bool(d_clip.any()), name
    plans = {}
    packed_only()
    plans["encode_streams"] = h.debug_last_encode_streams_plan()
    planar()
    plans["encode_streams_planar"] = h.debug_last_encode_streams_planar_plan()
    planar_no_digests()
    plans["encode_streams_planar_no_digests"] = h.debug_last_encode_streams_planar_plan()
    with_digests = (("composition_a", composition), ("encode_streams_planar", planar), ("composition_b", composition))
    without = (("composition_no_digests_a", composition_no_digests), ("encode_streams_planar_no_digests", planar_no_digests),
               ("composition_no_digests_b", composition_no_digests), ("encode_streams_alone", packed_only),
               ("encode_streams_planar_no_digests_dword_loads", planar_dword_loads))
    times = {k: [] for k, _ in with_digests + without}
    for rows, n in ((with_digests, digest_reps), (without, reps)):
        for i in range(n):
            for key, fn in rows:
                t0 = time.perf_counter()
                fn()
                times[key].append(time.perf_counter() - t0)
            print(name, rows[0][0], "round", i + 1, "of", n, flush=True)
    out = {"streams": B, "channels": C, "samples_per_channel": B * T, "frames": F, "tensor_bytes": int(x.nbytes),
           "frame_bytes": state["planar"][1], "plans": plans, "reps": reps, "reps_with_digests": digest_reps}
    for key, t in times.items():
        out[key] = {"median_ms": round(statistics.median(t) * 1e3, 3), "min_ms": round(min(t) * 1e3, 3),
                    "max_ms": round(max(t) * 1e3, 3)}
    for base, mine in (("composition", "encode_streams_planar"), ("composition_no_digests", "encode_streams_planar_no_digests")):
        both = times[base + "_a"] + times[base + "_b"]
        out[base] = {"median_ms": round(statistics.median(both) * 1e3, 3)}
        spread = round(abs(out[base + "_a"]["median_ms"] - out[base + "_b"]["median_ms"]), 3)
        out[base + "_spread_ms"] = spread
        out[mine + "_over_" + base] = round(out[mine]["median_ms"] / out[base]["median_ms"], 3)
        out[mine + "_not_slower_than_" + base + "_by_more_than_its_spread"] = bool(
            out[mine]["median_ms"] <= out[base]["median_ms"] + spread)
    out["planar_no_digests_over_encode_streams_alone"] = round(
        out["encode_streams_planar_no_digests"]["median_ms"] / out["encode_streams_alone"]["median_ms"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=2048)
    ap.add_argument("--distinct", type=int, default=64)
    ap.add_argument("--frames-per-stream", type=int, default=40)
    ap.add_argument("--block-size", type=int, default=4096)
    ap.add_argument("--large-frames", type=int, default=24576)
    ap.add_argument("--reps", type=int, default=24)
    ap.add_argument("--large-digest-reps", type=int, default=3)
    ap.add_argument("--only", choices=("streams", "one_large"), help="run one workload (for a profiler)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "encode_streams_planar_rates.json"))
    args = ap.parse_args()
    assert args.reps >= 24 or args.only, "the median of at least 24 calls"
    n, per, D = args.block_size, args.frames_per_stream, args.distinct
    h = _capi.Handle(0, hooks=True)
    cfg = _capi.make_frame_config(_capi.make_config(lpc_order=8))
    scale = np.float32(2.0 ** -(BITS - 1))
    res = {"what": "device memory, 16-bit streams of frames of %d samples as a float32 [B, C, T] tensor; "
                   "flacenc_hip_encode_streams_planar (digests, clip counts) against torch mul, round, clamp, to(int16), "
                   "permute + contiguous, then flacenc_hip_encode_streams, then flacenc_hip_md5_spans" % n,
           "timing": "wall clock, warm, the rows timed alternately in one process; median, min and max of `reps` calls; "
                     "composition_a / _b are the same composition timed as two interleaved series"}
    if args.only != "one_large":
        count = args.streams
        x = _capi.sigen_frames(D * per, 1, n, BITS, 200.0, 0.4, 0.4, seed=0xF1AC0002)
        x = np.ascontiguousarray(x.reshape(D, 1, per * n)).astype(np.float32) * scale
        x = np.ascontiguousarray(np.tile(x, (-(-count // D), 1, 1))[:count])
        res["streams_%d" % count] = measure(h, "streams", x, n, 16000, cfg, args.reps, args.reps)
        del x
    if args.only != "streams":
        F = args.large_frames
        big = _capi.sigen_frames(F, 2, n, BITS, 200.0, 0.4, 0.4, seed=0xF1AC0001)
        x = np.ascontiguousarray(big.transpose(1, 0, 2).reshape(1, 2, F * n)).astype(np.float32) * scale
        del big
        res["one_large"] = measure(h, "one_large", x, n, 44100, cfg, args.reps, min(args.reps, args.large_digest_reps))
    h.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
