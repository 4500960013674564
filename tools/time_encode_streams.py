"""Times flacenc_hip_encode_streams against the loop of flacenc_hip_encode_pcm it replaces, on a library of short files.

The library: mono 16-bit streams of 40 frames of 4096 samples (about 10 s of 16 kHz audio each) plus a last block;
host memory on both sides (pageable), wall clock around the blocking calls, three timings on a warm handle, best = their
minimum, spread = maximum - minimum.

  rows     64 and 2048 streams, each with (a) a random tail of 64..4095 samples, (b) one tail length for all, (c) no
           tail: the three rows price the tail runs (a corpus with k distinct tail lengths pays k tail runs)
  loop     flacenc_hip_encode_pcm once per stream, same handle, same config; the batch must give the same bytes
  one      one stereo stream of 24 576 frames as a batch of one against flacenc_hip_encode_pcm (reported, not gated: the
           batch does not overlap its transfers with compute)
  fill     streams_fill_kernel alone (flacenc_hip_debug_streams_fill) against flacenc_hip_fill_le_bytes on one stream's
           frames in device memory, in GB/s of PCM read

Writes profiles/encode_streams_rates.json.

    python tools/time_encode_streams.py [--streams 2048] [--large-frames 24576]
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


def row(t):
    return {"s": [round(v, 5) for v in t], "best_s": round(min(t), 5), "spread_s": round(max(t) - min(t), 5)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=2048)
    ap.add_argument("--distinct", type=int, default=64)
    ap.add_argument("--frames-per-stream", type=int, default=40)
    ap.add_argument("--block-size", type=int, default=4096)
    ap.add_argument("--large-frames", type=int, default=24576)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "encode_streams_rates.json"))
    args = ap.parse_args()
    n, bps, per, D = args.block_size, 16, args.frames_per_stream, args.distinct
    h = _capi.Handle(0, hooks=True)
    lib = _capi.load()
    cfg = _capi.make_frame_config(_capi.make_config(lpc_order=8))
    x = _capi.sigen_frames(D * (per + 1), 1, n, bps, 200.0, 0.4, 0.4, seed=0xF1AC0002)
    material = np.ascontiguousarray(x.reshape(D, (per + 1) * n)).astype("<i2")   # D streams of up to per + 1 blocks
    bound = int(lib.flacenc_hip_frame_bytes_bound(1, n, bps))
    rng = np.random.default_rng(7)
    res = {"what": "mono 16-bit streams of %d frames of %d samples + a last block; host pageable memory; wall clock" % (per, n),
           "timing": "3 timings after one warm call; best = their minimum, spread = maximum - minimum"}

    def library(count, tails):
        spans = [material[s % D, :per * n + int(tails[s])].view(np.uint8) for s in range(count)]
        pcm = np.concatenate(spans)
        table = np.zeros(count, _capi.PCM_STREAM_DESC_DTYPE)
        at = out_at = 0
        for s in range(count):
            cap = (per + 1) * bound
            table[s] = (at, per * n + int(tails[s]), out_at, cap, 1, bps, 2, RATE)
            at += spans[s].size
            out_at += cap
        return pcm, table, spans, out_at

    def batch(count, tails, loop):
        pcm, table, spans, out_bytes = library(count, tails)
        out = np.zeros(out_bytes, np.uint8)
        state = {}

        def call():
            state["r"] = h.encode_streams(pcm, table, cfg, n, out)
        call()
        r = dict(streams=count, **row(timings(call)))
        lens, totals, ct, _ = state["r"]
        r.update(frames=ct[0], bytes=ct[1], plan=h.debug_last_encode_streams_plan(), distinct_tails=len(set(map(int, tails))),
                 G_samples_per_s=round(int(table["total_samples"].sum()) / r["best_s"] / 1e9, 3))
        assert (totals[:, 3] == 0).all()
        if loop:
            one_out = np.zeros((per + 1) * bound, np.uint8)
            got = {}

            def run_loop():
                for s in range(count):
                    data, ln = h.encode_pcm(spans[s], 1, cfg, 2, bps, n, RATE, out=one_out)
                    if s in (0, count - 1):
                        got[s] = data.tobytes()
            run_loop()
            lp = row(timings(run_loop))
            for s in (0, count - 1):   # the same bytes
                o = int(table[s]["out_offset"])
                assert out[o:o + int(totals[s][1])].tobytes() == got[s]
            lp["per_stream_ms"] = round(lp["best_s"] / count * 1e3, 3)
            r["loop"] = lp
            r["loop_minus_batch_s"] = round(lp["best_s"] - r["best_s"], 5)
            r["speedup"] = round(lp["best_s"] / r["best_s"], 2)
            r["faster_by_more_than_the_spread"] = bool(lp["best_s"] - r["best_s"] > max(lp["spread_s"], r["spread_s"]))
        return r

    for count in (64, args.streams):
        random_tails = rng.integers(64, n, count)
        res["random_tails_%d" % count] = batch(count, random_tails, True)
        res["equal_tails_%d" % count] = batch(count, np.full(count, 1000), count == 64)
        res["no_tails_%d" % count] = batch(count, np.zeros(count, np.int64), count == 64)

    # one large stereo stream through both calls
    F = args.large_frames
    big = _capi.sigen_frames(F, 2, n, bps, 200.0, 0.4, 0.4, seed=0xF1AC0001)
    big_pcm = np.ascontiguousarray(big.transpose(0, 2, 1)).astype("<i2").reshape(-1).view(np.uint8)
    del big
    sb = int(lib.flacenc_hip_stereo_frame_bytes_bound(n, bps))
    out_big = np.zeros(F * sb, np.uint8)
    table = np.zeros(1, _capi.PCM_STREAM_DESC_DTYPE)
    table[0] = (0, F * n, 0, out_big.size, 2, bps, 2, 44100)
    state = {}

    def one_batch():
        state["b"] = h.encode_streams(big_pcm, table, cfg, n, out_big)

    def one_pcm():
        state["p"] = h.encode_pcm(big_pcm, 2, cfg, 2, bps, n, 44100, out=out_big)
    one_pcm()
    want = state["p"][0].tobytes()
    res["one_large_encode_pcm"] = dict(frames=F, **row(timings(one_pcm)))
    one_batch()
    assert out_big[:int(state["b"][1][0][1])].tobytes() == want
    res["one_large_encode_streams"] = dict(frames=F, **row(timings(one_batch)))
    for k in ("one_large_encode_pcm", "one_large_encode_streams"):
        res[k]["G_samples_per_s"] = round(F * 2 * n / res[k]["best_s"] / 1e9, 3)
    del out_big

    # the fill kernel alone, device memory
    import torch
    fill_frames = min(F, 65535)   # flacenc_hip_fill_le_bytes takes at most 65535 frames
    d_pcm = torch.from_numpy(big_pcm[:fill_frames * n * 4]).cuda()
    rows_a = torch.zeros((fill_frames, 2, n), dtype=torch.int32, device="cuda")
    rows_b = torch.zeros((fill_frames, 2, n), dtype=torch.int32, device="cuda")

    def old():
        h.fill_le_bytes_device(d_pcm.data_ptr(), fill_frames * n, 2, 2, fill_frames, n, rows_a.data_ptr(), n,
                               torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()

    def new():
        h.debug_streams_fill(d_pcm.data_ptr(), fill_frames * n, 2, 2, fill_frames, n, rows_b.data_ptr(), n)
    old()
    new()
    assert torch.equal(rows_a, rows_b)
    for name, fn in (("fill_le_bytes", old), ("streams_fill", new)):
        t = timings(fn, 5)
        res["fill_" + name] = dict(frames=fill_frames, pcm_bytes=int(d_pcm.numel()), **row(t),
                                   GB_per_s_pcm_read=round(d_pcm.numel() / min(t) / 1e9, 1))
    res["fill_streams_fill"]["note"] = "includes the upload of the frame table (16 bytes per frame) and a synchronisation"
    h.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
