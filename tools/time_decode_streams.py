"""Times flacenc_hip_decode_streams against the loop of flacenc_hip_decode_pcm it replaces, on a library of short files.

The library: mono 16-bit streams of 40 frames of 4096 samples (about 10 s of 16 kHz audio each).  64 distinct streams are
encoded (flacenc_hip_encode_pcm on synthetic audio); the batch of 2048 streams holds each of them 32 times.  Host memory
on both sides (pageable), wall clock around the blocking calls, best of 3 on a warm handle:

  batch_64 / batch_2048   one flacenc_hip_decode_streams call for 64 / 2048 streams
  loop_64                 flacenc_hip_decode_pcm once per stream over the first 64 streams, same handle (linear in the
                          number of streams by construction); its three timings give the spread the batch must beat
  one_large_*             one stereo stream of 24 576 frames of 4096 samples through both calls (reported, not gated: the
                          batch does not overlap its transfers with decoding)

Every timed output is compared with the PCM that went in.  Writes profiles/decode_streams_rates.json.

    python tools/time_decode_streams.py
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from flacenc_rs_amd import _capi  # noqa: E402

RATE = 16000


def timings(fn, reps=3):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return out


def encode(h, frames, channels, n, bps, seed):
    """-> (stream bytes, frame lengths, the PCM bytes that went in)"""
    x = _capi.sigen_frames(frames, channels, n, bps, 200.0, 0.4, 0.4, seed=seed)
    pcm = np.ascontiguousarray(x.transpose(0, 2, 1)).astype("<i2").reshape(-1).view(np.uint8)
    cfg = _capi.make_frame_config(_capi.make_config(lpc_order=8))
    data, lens = h.encode_pcm(pcm, channels, cfg, 2, bps, n, RATE)
    return np.array(data, copy=True), np.asarray(lens, np.int64), pcm


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=2048)
    ap.add_argument("--distinct", type=int, default=64)
    ap.add_argument("--frames-per-stream", type=int, default=40)
    ap.add_argument("--block-size", type=int, default=4096)
    ap.add_argument("--large-frames", type=int, default=24576)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decode_streams_rates.json"))
    args = ap.parse_args()
    n, bps, per, D = args.block_size, 16, args.frames_per_stream, args.distinct
    h = _capi.Handle(0, hooks=True)
    data, lens, pcm = encode(h, D * per, 1, n, bps, 0xF1AC0002)
    ends = np.concatenate([[0], np.cumsum(lens)])
    cuts = ends[::per]                        # stream s = bytes [cuts[s], cuts[s + 1])
    stream_pcm = per * n * 2
    res = {"what": "mono 16-bit streams of %d frames of %d samples; host pageable memory; wall clock" % (per, n),
           "timing": "3 timings after one warm call; best = their minimum"}

    def batch(count):
        reps = -(-count // D)
        everything = np.tile(data, reps)
        table = np.zeros(count, _capi.STREAM_DESC_DTYPE)
        for s in range(count):
            lo = (s // D) * len(data) + int(cuts[s % D])
            table[s] = (lo, int(cuts[s % D + 1] - cuts[s % D]), s * stream_pcm, stream_pcm, 1, bps, n, 2)
        out = np.zeros(count * stream_pcm, np.uint8)
        state = {}

        def call():
            state["totals"], state["call"], _ = h.decode_streams(everything, table, count * per, out)
        call()
        t = timings(call)
        assert state["call"] == [count * per, count * per * n], state["call"]
        assert (state["totals"][:, 3] == 0).all()
        assert np.array_equal(out[:D * stream_pcm], pcm) and np.array_equal(out[-stream_pcm:], pcm[((count - 1) % D) * stream_pcm:][:stream_pcm])
        plan = h.debug_last_decode_streams_plan()
        return {"streams": count, "frames": count * per, "s": [round(v, 5) for v in t], "best_s": round(min(t), 5),
                "G_samples_per_s": round(count * per * n / min(t) / 1e9, 3), "compressed_bytes": int(len(everything)),
                "pcm_bytes": int(out.size),
                "plan": dict(zip(("launches", "synchronisations", "transfers", "channel_classes"), plan))}

    res["batch_64"] = batch(64)
    res["batch_%d" % args.streams] = batch(args.streams)

    out = np.zeros(stream_pcm, np.uint8)

    def loop():
        for s in range(64):
            got, totals = h.decode_pcm(data[cuts[s]:cuts[s + 1]], 1, bps, n, out=out)
            assert totals[0] == per and totals[3] == 0
    loop()
    t = timings(loop)
    assert np.array_equal(out, pcm[63 * stream_pcm:64 * stream_pcm])
    res["loop_64"] = {"streams": 64, "frames": 64 * per, "s": [round(v, 5) for v in t], "best_s": round(min(t), 5),
                      "spread_s": round(max(t) - min(t), 5), "per_stream_ms": round(min(t) / 64 * 1e3, 3),
                      "G_samples_per_s": round(64 * per * n / min(t) / 1e9, 3)}
    gain = res["loop_64"]["best_s"] - res["batch_64"]["best_s"]
    res["acceptance"] = {"loop_minus_batch_s": round(gain, 5), "loop_spread_s": res["loop_64"]["spread_s"],
                         "batch_64_faster_by_more_than_the_spread": bool(gain > res["loop_64"]["spread_s"]),
                         "speedup": round(res["loop_64"]["best_s"] / res["batch_64"]["best_s"], 2)}

    # one large stream through both calls
    F = args.large_frames
    big, big_lens, big_pcm = encode(h, F, 2, n, bps, 0xF1AC0001)
    out_big = np.zeros(big_pcm.size, np.uint8)
    table = np.zeros(1, _capi.STREAM_DESC_DTYPE)
    table[0] = (0, len(big), 0, out_big.size, 2, bps, n, 2)

    def one_batch():
        _, call, _ = h.decode_streams(big, table, F, out_big)
        assert call == [F, F * n]

    def one_pcm():
        _, totals = h.decode_pcm(big, 2, bps, n, out=out_big)
        assert totals == [F, F * n, len(big), 0]
    for name, fn in (("one_large_decode_streams", one_batch), ("one_large_decode_pcm", one_pcm)):
        out_big[:] = 0
        fn()
        t = timings(fn)
        assert np.array_equal(out_big, big_pcm)
        res[name] = {"frames": F, "s": [round(v, 5) for v in t], "best_s": round(min(t), 5),
                     "G_samples_per_s": round(F * 2 * n / min(t) / 1e9, 3)}
    h.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
    if not res["acceptance"]["batch_64_faster_by_more_than_the_spread"]:
        raise SystemExit("the batch of 64 streams is not faster than the loop by more than the loop's spread")


if __name__ == "__main__":
    main()
