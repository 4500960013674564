"""Times the decoders around flacenc_hip_set_max_bits_per_sample, device memory, one process:

  mono16      the README's library -- 2 048 mono 16-bit streams of 40 frames of 4096 samples, 64 distinct ones encoded by
              flacenc_hip_encode_pcm -- through flacenc_hip_decode_streams and, one 16 000-sample float32 crop per
              stream, flacenc_hip_decode_ranges_planar.  With --tree DIR the library and the bindings of another build
              of this repository are timed (its parent: tools/ab_decode_depth32.sh alternates the two on one box).
  --deep      also 2 048 stereo mid/side streams of the same shape at 16 and at 32 bits.  No encoder here writes 32
              bits, so both are written by tests/flac_write.py (LPC order 8, precision 15, shift 14, RICE2; a full-scale
              sinusoid plus noise, right = -left plus noise, so the 32-bit side needs 33 bits): 4 distinct streams,
              each one written frame repeated 40 times (the decoders do not look at frame numbers).

Wall clock around the blocking call, --reps calls after two warm ones; min and median.  The first stream's PCM is
compared with what went in.  Prints one line "AB {json}"; --out FILE also writes the JSON.

    python tools/time_decode_depth32.py --deep --out profiles/decode_depth32_rates.json
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, PER, D, COUNT, CROP = 4096, 40, 64, 2048, 16000


def timed(fn, reps):
    fn()
    fn()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return {"min_ms": round(min(out) * 1e3, 4), "median_ms": round(statistics.median(out) * 1e3, 4)}


def run_batch(_capi, h, data, cuts, channels, bps, width, check_pcm, reps):
    """COUNT streams, stream s = the distinct stream s % (len(cuts) - 1); device memory."""
    import torch
    distinct = len(cuts) - 1
    everything = np.tile(data, -(-COUNT // distinct))
    stream_pcm = PER * N * channels * width
    table = np.zeros(COUNT, _capi.STREAM_DESC_DTYPE)
    for s in range(COUNT):
        lo = (s // distinct) * len(data) + int(cuts[s % distinct])
        table[s] = (lo, int(cuts[s % distinct + 1] - cuts[s % distinct]), s * stream_pcm, stream_pcm, channels, bps, N, width)
    d_in = torch.from_numpy(everything).cuda()
    d_out = torch.zeros(COUNT * stream_pcm, dtype=torch.uint8, device="cuda")
    d_tot = torch.zeros(COUNT * 4, dtype=torch.int64, device="cuda")
    res = {}

    def streams():
        call, _ = h.decode_streams_device(d_in.data_ptr(), len(everything), table, COUNT * PER, d_out.data_ptr(),
                                          d_out.numel(), d_tot.data_ptr())
        assert call == [COUNT * PER, COUNT * PER * N], call
    res["decode_streams"] = timed(streams, reps)
    assert np.array_equal(d_out[: len(check_pcm)].cpu().numpy(), check_pcm)
    res["decode_streams"]["G_samples_per_s"] = round(COUNT * PER * N * channels / res["decode_streams"]["min_ms"] / 1e6, 3)
    del d_out
    ranges = np.zeros(COUNT, _capi.RANGE_DESC_DTYPE)
    ranges["first_sample"] = 3 * N + 100 + 37 * (np.arange(COUNT) % 50)
    ranges["n_samples"] = CROP
    ranges["stream"] = np.arange(COUNT)
    ranges["out_offset"] = np.arange(COUNT, dtype=np.uint64) * (CROP * channels * 4)
    d_pl = torch.zeros(COUNT * CROP * channels, dtype=torch.float32, device="cuda")
    d_rt = torch.zeros(COUNT * 4, dtype=torch.int64, device="cuda")

    def planar():
        call, _ = h.decode_ranges_planar_device(d_in.data_ptr(), len(everything), table, ranges, COUNT * PER,
                                                d_pl.data_ptr(), d_pl.numel() * 4, _capi.SAMPLE_F32, d_rt.data_ptr())
        assert call[1] == COUNT * CROP, call
    res["decode_ranges_planar"] = timed(planar, reps)
    return res


def written_streams(bps, n_distinct=4):
    """-> (bytes, cuts, the first stream's PCM) of `n_distinct` stereo mid/side streams written by tests/flac_write.py."""
    sys.path.insert(0, os.path.join(HERE, "tests"))
    import depth32_cases as d32
    import flac_write as fw
    rng = np.random.default_rng(bps)
    parts, cuts, first = [], [0], None
    hi, width = (1 << (bps - 1)) - 1, 4 if bps == 32 else 2
    for _ in range(n_distinct):
        left = d32.sinusoid(rng, N, bps=bps, period=rng.uniform(300, 900), noise_bits=bps - 12)
        right = np.clip(-left + rng.integers(-(1 << (bps - 12)), (1 << (bps - 12)) + 1, N), -hi, hi)
        x = np.stack([left, right])
        sf = dict(kind="lpc", order=8, coefs=[16383, 0, 0, 0, 1, -1, 0, 0], precision=15, shift=14, method=1, porder=4)
        c = d32.make_case("timed", x, 10, [sf, sf], bps=bps, ss_code=7 if bps == 32 else fw.SS_CODES[bps])
        parts.append(c["data"] * PER)
        cuts.append(cuts[-1] + len(parts[-1]))
        if first is None:
            one = np.ascontiguousarray(x.T.astype("<i4").reshape(-1).view(np.uint8).reshape(-1, 4)[:, :width]).reshape(-1)
            first = np.tile(one, PER)
    return np.frombuffer(b"".join(parts), np.uint8).copy(), np.array(cuts), first


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=HERE, help="the checkout whose library, bindings and tools are timed")
    ap.add_argument("--deep", action="store_true", help="also the 16-bit and 32-bit stereo mid/side batches (this tree only)")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out")
    args = ap.parse_args()
    tree = os.path.abspath(args.tree)
    sys.path.insert(0, tree)
    sys.path.insert(0, os.path.join(tree, "tools"))
    from flacenc_rs_amd import _capi
    from time_decode_streams import encode

    out = {"tree": os.path.relpath(tree, HERE), "reps": args.reps,
           "what": "%d streams of %d frames of %d samples, device memory, wall clock in ms" % (COUNT, PER, N)}
    h = _capi.Handle(0, hooks=True)
    data, lens, pcm = encode(h, D * PER, 1, N, 16, 0xF1AC0002)
    cuts = np.concatenate([[0], np.cumsum(lens)])[::PER]
    out["mono16"] = run_batch(_capi, h, data, cuts, 1, 16, 2, pcm, args.reps)
    if args.deep:
        for bps in (16, 32):
            d, c, first = written_streams(bps)
            if bps == 32:
                h.set_max_bits_per_sample(32)
            key = "midside%d" % bps
            out[key] = run_batch(_capi, h, d, c, 2, bps, 4 if bps == 32 else 2, first, args.reps)
            out[key]["compressed_bytes_per_stream"] = int(c[1])
    h.close()
    print("AB " + json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
