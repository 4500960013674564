"""Times flacenc_hip_decode_ranges against what a host had to do without it: decode every stream whole and slice.

The library of tools/time_decode_streams.py: mono 16-bit streams of 40 frames of 4096 samples, 64 distinct ones, the batch
of 2048 holding each 32 times.  One crop of 16 000 samples per stream at a seeded random position.  Host memory on both
sides (pageable), wall clock around the blocking calls, 3 timings on a warm handle, best = their minimum, spread = max -
min:

  (a) decode_streams_then_slice   flacenc_hip_decode_streams of the whole streams, then a numpy slice per stream
  (b) decode_ranges               one flacenc_hip_decode_ranges call over whole-stream spans
  (c) decode_ranges_seek          the same call with each span started at a seek point at most 4 frames before the crop
                                  (a point every 4 frames, as a SEEKTABLE would hold) and ended at the stream's end
  one_large_*                     one stereo stream of 24 576 frames with 256 crops, as (a) and (b)

Every timed output is compared with the PCM that went in.  Writes profiles/decode_ranges_rates.json.

    python tools/time_decode_ranges.py
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from flacenc_rs_amd import _capi  # noqa: E402
from time_decode_streams import encode, timings  # noqa: E402

CROP = 16000
PLAN = ("launches", "synchronisations", "transfers", "channel_classes")


def row(t, samples, **more):
    r = {"s": [round(v, 5) for v in t], "best_s": round(min(t), 5), "spread_s": round(max(t) - min(t), 5),
         "M_crop_samples_per_s": round(samples / min(t) / 1e6, 1)}
    r.update(more)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=2048)
    ap.add_argument("--distinct", type=int, default=64)
    ap.add_argument("--frames-per-stream", type=int, default=40)
    ap.add_argument("--block-size", type=int, default=4096)
    ap.add_argument("--large-frames", type=int, default=24576)
    ap.add_argument("--large-crops", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decode_ranges_rates.json"))
    args = ap.parse_args()
    n, bps, per, D = args.block_size, 16, args.frames_per_stream, args.distinct
    h = _capi.Handle(0, hooks=True)
    data, lens, pcm = encode(h, D * per, 1, n, bps, 0xF1AC0002)
    ends = np.concatenate([[0], np.cumsum(lens)])
    cuts = ends[::per]                        # stream s = bytes [cuts[s], cuts[s + 1])
    stream_samples = per * n
    stream_pcm = stream_samples * 2
    res = {"what": "mono 16-bit streams of %d frames of %d samples, one crop of %d samples per stream at a seeded random "
                   "position; host pageable memory; wall clock" % (per, n, CROP),
           "timing": "3 timings after one warm call; best = their minimum, spread = max - min"}

    def batch(count):
        rng = np.random.default_rng(0xC509 + count)
        firsts = rng.integers(0, stream_samples - CROP + 1, count)
        everything = np.tile(data, -(-count // D))
        table = np.zeros(count, _capi.STREAM_DESC_DTYPE)
        seek_table = np.zeros(count, _capi.STREAM_DESC_DTYPE)
        ranges = np.zeros(count, _capi.RANGE_DESC_DTYPE)
        seek_ranges = np.zeros(count, _capi.RANGE_DESC_DTYPE)
        for s in range(count):
            lo = (s // D) * len(data) + int(cuts[s % D])
            size = int(cuts[s % D + 1] - cuts[s % D])
            table[s] = (lo, size, s * stream_pcm, stream_pcm, 1, bps, n, 2)
            ranges[s] = (int(firsts[s]), CROP, s * CROP * 2, s, 0)
            k = int(firsts[s]) // n // 4 * 4      # the seek point: a frame at most 4 frames before the crop's
            skip = int(ends[(s % D) * per + k] - cuts[s % D])
            seek_table[s] = (lo + skip, size - skip, 0, 0, 1, bps, n, 2)
            seek_ranges[s] = (int(firsts[s]) - k * n, CROP, s * CROP * 2, s, 0)
        whole = np.zeros(count * stream_pcm, np.uint8)
        crops = np.zeros(count * CROP * 2, np.uint8)
        want = np.concatenate([pcm[(s % D) * stream_pcm + 2 * int(firsts[s]):][:2 * CROP] for s in range(count)])
        state = {}

        def a():
            _, state["call"], _ = h.decode_streams(everything, table, count * per, whole)
            rows = whole.reshape(count, stream_pcm)
            state["crops"] = np.concatenate([rows[s, 2 * int(firsts[s]):2 * int(firsts[s]) + 2 * CROP] for s in range(count)])

        def b():
            state["totals"], state["call"], _ = h.decode_ranges(everything, table, ranges, count * per, crops)

        def c():
            state["totals"], state["call"], _ = h.decode_ranges(everything, seek_table, seek_ranges, count * per, crops)
        out = {"streams": count, "crop_samples": count * CROP, "compressed_bytes": int(len(everything)),
               "whole_pcm_bytes": int(whole.size), "crop_pcm_bytes": int(crops.size)}
        a()
        t = timings(a)
        assert np.array_equal(state["crops"], want)
        out["a_decode_streams_then_slice"] = row(t, count * CROP, plan=dict(zip(PLAN, h.debug_last_decode_streams_plan())))
        for name, fn in (("b_decode_ranges", b), ("c_decode_ranges_seek", c)):
            crops[:] = 0
            fn()
            t = timings(fn)
            assert np.array_equal(crops, want) and state["call"][1] == count * CROP, name
            assert (state["totals"][:, 0] == CROP).all() and not state["totals"][:, 1].any()
            out[name] = row(t, count * CROP, frame_decodes=state["call"][0],
                            plan=dict(zip(PLAN, h.debug_last_decode_ranges_plan())))
        gain = out["a_decode_streams_then_slice"]["best_s"] - out["b_decode_ranges"]["best_s"]
        spread = max(out[k]["spread_s"] for k in ("a_decode_streams_then_slice", "b_decode_ranges"))
        out["a_over_b"] = round(out["a_decode_streams_then_slice"]["best_s"] / out["b_decode_ranges"]["best_s"], 2)
        out["a_over_c"] = round(out["a_decode_streams_then_slice"]["best_s"] / out["c_decode_ranges_seek"]["best_s"], 2)
        out["b_faster_than_a_by_more_than_the_spread"] = bool(gain > spread)
        return out

    res["streams_64"] = batch(64)
    res["streams_%d" % args.streams] = batch(args.streams)

    # one large stereo stream, many crops
    F, K = args.large_frames, args.large_crops
    big, big_lens, big_pcm = encode(h, F, 2, n, bps, 0xF1AC0001)
    firsts = np.random.default_rng(0xC50A).integers(0, F * n - CROP + 1, K)
    table = np.zeros(1, _capi.STREAM_DESC_DTYPE)
    table[0] = (0, len(big), 0, big_pcm.size, 2, bps, n, 2)
    ranges = np.zeros(K, _capi.RANGE_DESC_DTYPE)
    for r in range(K):
        ranges[r] = (int(firsts[r]), CROP, r * CROP * 4, 0, 0)
    whole = np.zeros(big_pcm.size, np.uint8)
    crops = np.zeros(K * CROP * 4, np.uint8)
    want = np.concatenate([big_pcm[4 * int(f):4 * int(f) + 4 * CROP] for f in firsts])
    state = {}

    def one_a():
        _, call, _ = h.decode_streams(big, table, F, whole)
        assert call == [F, F * n]
        state["crops"] = np.concatenate([whole[4 * int(f):4 * int(f) + 4 * CROP] for f in firsts])

    def one_b():
        _, state["call"], _ = h.decode_ranges(big, table, ranges, F, crops)
    one_a()
    t = timings(one_a)
    assert np.array_equal(state["crops"], want)
    res["one_large_decode_streams_then_slice"] = row(t, K * CROP, frames=F, crops=K)
    one_b()
    t = timings(one_b)
    assert np.array_equal(crops, want) and state["call"][1] == K * CROP
    res["one_large_decode_ranges"] = row(t, K * CROP, frames=F, crops=K, frame_decodes=state["call"][0])
    h.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
