"""Times flacenc_hip_recover_streams, and what its index request costs the calls that share the index, on the README's
batch: 2 048 mono 16-bit streams of 40 frames of 4096 samples, device memory, wall clock around the blocking calls (each
ends in a device synchronise), `--reps` timings after a warm call.

  --mode existing   flacenc_hip_decode_streams and flacenc_hip_decode_ranges (one 16 000-sample crop per stream) only: run
                    it once with this tree's package and once with --package-root pointing at a tree that holds the
                    parent commit's flacenc_rs_amd (library included), alternating, and compare same-box
  --mode recover    flacenc_hip_recover_streams against flacenc_hip_decode_streams of the same library: on the undamaged
                    batch (the price of keeping numbers, the max-scan and an empty zero pass; outputs compared byte for
                    byte) and on the batch with one frame of every stream broken

Prints one JSON line; --out appends it to a file.

    python tools/time_recover.py --mode recover
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATE = 16000


def timings(fn, reps):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return out


def stats(t):
    t = sorted(t)
    return {"min_ms": round(t[0] * 1e3, 3), "median_ms": round(t[len(t) // 2] * 1e3, 3), "max_ms": round(t[-1] * 1e3, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("existing", "recover"), default="recover")
    ap.add_argument("--package-root", default=ROOT, help="the directory that holds the flacenc_rs_amd to load")
    ap.add_argument("--label", default="")
    ap.add_argument("--streams", type=int, default=2048)
    ap.add_argument("--distinct", type=int, default=64)
    ap.add_argument("--frames-per-stream", type=int, default=40)
    ap.add_argument("--block-size", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.package_root))
    from flacenc_rs_amd import _capi
    import torch

    n, bps, per, D, count = args.block_size, 16, args.frames_per_stream, args.distinct, args.streams
    h = _capi.Handle(0)
    x = _capi.sigen_frames(D * per, 1, n, bps, 200.0, 0.4, 0.4, seed=0xF1AC0002)
    pcm = np.ascontiguousarray(x.transpose(0, 2, 1)).astype("<i2").reshape(-1).view(np.uint8)
    data, lens = h.encode_pcm(pcm, 1, _capi.make_frame_config(_capi.make_config(lpc_order=8)), 2, bps, n, RATE)
    data, lens = np.array(data, copy=True), np.asarray(lens, np.int64)
    ends = np.concatenate([[0], np.cumsum(lens)])
    cuts = ends[::per]
    stream_pcm = per * n * 2
    everything = np.tile(data, -(-count // D))
    table = np.zeros(count, _capi.STREAM_DESC_DTYPE)
    for s in range(count):
        lo = (s // D) * len(data) + int(cuts[s % D])
        table[s] = (lo, int(cuts[s % D + 1] - cuts[s % D]), s * stream_pcm, stream_pcm, 1, bps, n, 2)
    # the 64 distinct streams are consecutive pieces of one encode: stream s is numbered from frame (s % D) * per on
    origins = np.array([(s % D) * per * n for s in range(count)], np.uint64)
    broken = everything.copy()
    for s in range(count):   # one bit of frame 17's body in every stream
        f = (s % D) * per + 17
        broken[(s // D) * len(data) + int(ends[f]) + int(lens[f]) // 2] ^= 0x08
    dev = torch.device("cuda:0")
    d_in, d_broken = torch.from_numpy(everything).to(dev), torch.from_numpy(broken).to(dev)
    d_out = torch.zeros(count * stream_pcm, dtype=torch.uint8, device=dev)
    d_ref = torch.zeros(count * stream_pcm, dtype=torch.uint8, device=dev)
    d_tot = torch.zeros((count, 8), dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    frames = count * per
    res = {"label": args.label, "mode": args.mode, "streams": count, "frames": frames, "reps": args.reps,
           "what": "mono 16-bit streams of %d frames of %d samples; device memory; wall clock, ms" % (per, n)}

    def decode_streams(src=d_in, out=d_ref):
        call, _ = h.decode_streams_device(src.data_ptr(), src.numel(), table, frames, out.data_ptr(), out.numel(),
                                          d_tot.data_ptr())
        return call

    if args.mode == "existing":
        ranges = np.zeros(count, _capi.RANGE_DESC_DTYPE)
        for s in range(count):
            ranges[s] = (12345, 16000, s * 32000, s, 0)

        def decode_ranges():
            call, _ = h.decode_ranges_device(d_in.data_ptr(), d_in.numel(), table, ranges, frames, d_out.data_ptr(),
                                             d_out.numel(), d_tot.data_ptr())
            return call
        assert decode_streams() == [frames, frames * n] and decode_ranges()[1] == count * 16000
        # interleaved, so that drift inside the process falls on both alike
        ts, tr = [], []
        for _ in range(args.reps):
            ts += timings(decode_streams, 1)
            tr += timings(decode_ranges, 1)
        res["decode_streams"], res["decode_ranges"] = stats(ts), stats(tr)
    else:
        def recover(src=d_in):
            call, _ = h.recover_streams_device(src.data_ptr(), src.numel(), table, frames, d_out.data_ptr(),
                                               d_out.numel(), d_tot.data_ptr(), origins=origins)
            return call
        assert decode_streams() == [frames, frames * n]
        assert recover() == [frames, frames * n, 0, 0] and torch.equal(d_out, d_ref)
        ts, tu = [], []
        for _ in range(args.reps):
            ts += timings(decode_streams, 1)
            tu += timings(recover, 1)
        res["decode_streams"], res["recover_undamaged"] = stats(ts), stats(tu)
        res["undamaged_ratio_of_medians"] = round(res["recover_undamaged"]["median_ms"] / res["decode_streams"]["median_ms"], 4)
        call = recover(d_broken)
        assert call == [frames - count, frames * n, count, 0], call
        tb, tsb = [], []
        for _ in range(args.reps):
            tsb += timings(lambda: decode_streams(d_broken, d_out), 1)
            tb += timings(lambda: recover(d_broken), 1)
        res["decode_streams_broken_stops_at_frame_17"], res["recover_broken"] = stats(tsb), stats(tb)
        res["broken_ratio_to_undamaged_decode_streams"] = round(res["recover_broken"]["median_ms"] / res["decode_streams"]["median_ms"], 4)
        res["gaps"] = call[2]
    h.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
