"""Times flacenc_hip_encode_streams around flacenc_hip_set_max_encode_bits_per_sample, device
memory, one process:

  library     2 048 mono streams of 40 frames of 4096 samples (64 distinct ones, repeated)
  long        one stereo stream of 24 576 frames of 4096 samples
each at 32 bits in 4-byte samples (the wide path) and at 24 bits in 3-byte samples (the existing path), with
use_lpc = 0, use_fixed = 1 and OrderSel::BitCount: the same candidates on both paths.  The material is a sinusoid of 0.4
of full scale plus noise of bits - 12 bits, the right channel of the stereo stream minus the left plus noise.
  --unchanged the library at 16 bits in 2-byte samples with the default config of tools/encode_many.py (LPC order 8 and
              the fixed predictors): the path no depth setting touches.  With --tree DIR the library and the bindings of
              another build of this repository are timed (its parent: tools/ab_encode_depth32.sh alternates the two).

Wall clock around the blocking call, --reps calls after two warm ones; min and median.  The call's totals are checked and
the first frame is parsed back by tests/flac_parse.py.  Prints one line "AB {json}"; --out FILE also writes the JSON.

    python tools/time_encode_depth32.py --out profiles/encode_depth32_rates.json
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, PER, D, COUNT, LONG = 4096, 40, 64, 2048, 24576


def timed(fn, reps):
    fn()
    fn()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return {"min_ms": round(min(out) * 1e3, 4), "median_ms": round(statistics.median(out) * 1e3, 4)}


def material(rng, total, channels, bps):
    """int32 [channels, total]"""
    hi = (1 << (bps - 1)) - 1
    t = np.arange(total) + rng.uniform(0, 500)
    left = np.round(0.4 * hi * np.sin(2 * np.pi * t / rng.uniform(300, 900))).astype(np.int64)
    noise = 1 << max(bps - 12, 1)
    rows = [left + rng.integers(-noise, noise + 1, total)]
    for _ in range(1, channels):
        rows.append(-left + rng.integers(-noise, noise + 1, total))
    return np.clip(np.stack(rows), -hi, hi).astype(np.int32)


def packed(x, width):
    flat = np.ascontiguousarray(x.T).reshape(-1).astype("<i4")
    return np.ascontiguousarray(flat.view(np.uint8).reshape(-1, 4)[:, :width]).reshape(-1)


def run(_capi, h, cfg, distinct, repeat, channels, bps, width, frames_per_stream, reps):
    """`repeat` copies of the `distinct` streams (uint8 arrays of one length) in one call, device memory."""
    import torch
    lib = _capi.load()
    one = len(distinct[0])
    d_pcm = torch.from_numpy(np.concatenate(distinct)).cuda().repeat(repeat)
    count = len(distinct) * repeat
    bound = int(lib.flacenc_hip_stereo_frame_bytes_bound(N, bps) if channels == 2 else lib.flacenc_hip_frame_bytes_bound(channels, N, bps))
    cap = frames_per_stream * bound
    table = np.zeros(count, _capi.PCM_STREAM_DESC_DTYPE)
    for s in range(count):
        table[s] = (s * one, frames_per_stream * N, s * cap, cap, channels, bps, width, 44100)
    frames = count * frames_per_stream
    d_out = torch.zeros(count * cap, dtype=torch.uint8, device="cuda")
    d_len = torch.zeros(frames, dtype=torch.int32, device="cuda")
    d_tot = torch.zeros(count * 4, dtype=torch.int64, device="cuda")
    got = {}

    def call():
        got["call"], _ = h.encode_streams_device(d_pcm.data_ptr(), d_pcm.numel(), table, cfg, N, d_out.data_ptr(),
                                                 d_out.numel(), d_len.data_ptr(), frames, d_tot.data_ptr())
        assert got["call"][0] == frames, got["call"]
    res = timed(call, reps)
    res["G_samples_per_s"] = round(frames * N * channels / res["min_ms"] / 1e6, 3)
    res["bytes"] = int(got["call"][1])
    res["of_the_pcm"] = round(res["bytes"] / (frames * N * channels * width), 4)
    first = d_out[: int(d_len[0])].cpu().numpy().tobytes()
    return res, first


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=HERE, help="the checkout whose library and bindings are timed")
    ap.add_argument("--unchanged", action="store_true", help="only the 16-bit library on the default config")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out")
    args = ap.parse_args()
    tree = os.path.abspath(args.tree)
    sys.path.insert(0, tree)
    sys.path.insert(0, os.path.join(HERE, "tests"))
    from flacenc_rs_amd import _capi
    import flac_parse

    out = {"tree": os.path.relpath(tree, HERE), "reps": args.reps, "what": "device memory, wall clock in ms"}
    rng = np.random.default_rng(0xE32)
    with _capi.Handle(0) as h:
        if args.unchanged:
            cfg = _capi.make_frame_config(_capi.make_config(lpc_order=8), use_fixed=True)
            streams = [packed(material(rng, PER * N, 1, 16), 2) for _ in range(D)]
            out["library16"], _ = run(_capi, h, cfg, streams, COUNT // D, 1, 16, 2, PER, args.reps)
        else:
            h.set_max_encode_bits_per_sample(32)
            cfg = _capi.make_frame_config(_capi.make_config(lpc_order=8), use_fixed=True, use_lpc=False,
                                          fixed_order_sel=_capi.ORDERSEL_BITCOUNT)
            for bps, width in ((32, 4), (24, 3)):
                lib_x = [material(rng, PER * N, 1, bps) for _ in range(D)]
                res, first = run(_capi, h, cfg, [packed(x, width) for x in lib_x], COUNT // D, 1, bps, width, PER, args.reps)
                back = flac_parse.parse_frame(first, stream_bps=bps, wasted_ok=True)
                assert np.array_equal(back["channels"], lib_x[0][:, :N])
                out["library%d" % bps] = res
                long_x = material(rng, LONG * N, 2, bps)
                res, first = run(_capi, h, cfg, [packed(long_x, width)], 1, 2, bps, width, LONG, args.reps)
                back = flac_parse.parse_frame(first, stream_bps=bps, wasted_ok=True)
                assert np.array_equal(back["channels"], long_x[:, :N])
                out["long%d" % bps] = res
    print("AB " + json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
