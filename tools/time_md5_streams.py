"""Times the STREAMINFO MD5 check of a library of short files: the host loop tools/decode_many.py runs by default against
the digests flacenc_hip_decode_streams_md5 computes on the device.

The library of tools/time_decode_streams.py: mono 16-bit streams of 40 frames of 4096 samples, 64 distinct ones, the batch
of 2048 holding each 32 times; and one stereo stream of 24 576 frames as the documented bad case (MD5 is serial inside a
stream, and one stream is one lane).  Host memory on both sides (pageable).  Rows, per shape:

  (a) decode_then_hashlib   flacenc_hip_decode_streams, then hashlib.md5 over every slot, one after another
  (b) decode_streams_md5    one flacenc_hip_decode_streams_md5 call
  (c) md5_spans_device      flacenc_hip_md5_spans alone on the PCM in device memory, in GB/s
  ordering                  (c) on 2048 spans of mixed lengths (4 KiB .. 1.25 MiB, log-uniform), handed over in random
                            order and in descending length order.  The call hands spans to lanes in descending length
                            order itself, so the two rows should agree; before it did, this pair of rows measured what
                            the ordering buys

Every timing is a host clock around a blocking call that ends in a synchronisation of the handle's stream (the library
has no stream-taking form of these calls to put events around).  Each row: one warm call, then `--reps` timings, (a) and
(b) alternating; best = their minimum, and all timings are kept so that the spread can be seen.  Every digest timed is
compared with hashlib.  Writes profiles/md5_streams_rates.txt.

    python tools/time_md5_streams.py
"""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from flacenc_rs_amd import _capi  # noqa: E402
from time_decode_streams import encode  # noqa: E402


def clock(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def alternate(fns, reps):
    """One warm call of each, then `reps` timings of each, alternating.  -> {name: [seconds]}"""
    for fn in fns.values():
        fn()
    out = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            out[k].append(clock(fn))
    return out


def row(times, nbytes):
    best = min(times)
    return {"s": [round(t, 5) for t in times], "best_s": round(best, 5), "spread_s": round(max(times) - best, 5),
            "GB_per_s": round(nbytes / best / 1e9, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=2048)
    ap.add_argument("--distinct", type=int, default=64)
    ap.add_argument("--frames-per-stream", type=int, default=40)
    ap.add_argument("--block-size", type=int, default=4096)
    ap.add_argument("--large-frames", type=int, default=24576)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "md5_streams_rates.txt"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing here can be measured without one")
    dev = torch.device("cuda:0")
    n, bps, per, D = args.block_size, 16, args.frames_per_stream, args.distinct
    h = _capi.Handle(0, hooks=True)
    data, lens, pcm = encode(h, D * per, 1, n, bps, 0xF1AC0002)
    cuts = np.concatenate([[0], np.cumsum(lens)])[::per]      # stream s = bytes [cuts[s], cuts[s + 1])
    stream_pcm = per * n * 2
    truth = [hashlib.md5(pcm[s * stream_pcm:(s + 1) * stream_pcm].tobytes()).digest() for s in range(D)]
    res = {"box": torch.cuda.get_device_name(0), "command": "python tools/time_md5_streams.py",
           "what": "mono 16-bit streams of %d frames of %d samples (%d bytes of PCM each); host pageable memory; host "
                   "clock around blocking calls; one warm call, then %d timings, (a) and (b) alternating"
                   % (per, n, stream_pcm, args.reps)}

    def library(count):
        reps = -(-count // D)
        everything = np.tile(data, reps)
        table = np.zeros(count, _capi.STREAM_DESC_DTYPE)
        for s in range(count):
            lo = (s // D) * len(data) + int(cuts[s % D])
            table[s] = (lo, int(cuts[s % D + 1] - cuts[s % D]), s * stream_pcm, stream_pcm, 1, bps, n, 2)
        out = np.zeros(count * stream_pcm, np.uint8)
        state = {}

        def host_path():
            totals, call, _ = h.decode_streams(everything, table, count * per, out)
            assert call == [count * per, count * per * n]
            state["host"] = [hashlib.md5(out[s * stream_pcm:s * stream_pcm + int(totals[s][1]) * 2]).digest()
                             for s in range(count)]

        def device_path():
            totals, call, _, digests = h.decode_streams_md5(everything, table, count * per, out)
            assert call == [count * per, count * per * n]
            state["device"] = digests

        t = alternate({"a": host_path, "b": device_path}, args.reps)
        plan = h.debug_last_decode_streams_plan()
        want = [truth[s % D] for s in range(count)]
        assert state["host"] == want and [d.tobytes() for d in state["device"]] == want
        # (c): the PCM in device memory, the kernel alone behind one upload of the span table
        d_pcm = torch.from_numpy(out).to(dev)
        d_dig = torch.zeros(count * 16, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        off = np.arange(count, dtype=np.uint64) * np.uint64(stream_pcm)
        ln = np.full(count, stream_pcm, np.uint64)
        tc = alternate({"c": lambda: h.md5_spans_device(d_pcm.data_ptr(), out.size, off, ln, d_dig.data_ptr())}, args.reps)
        assert [bytes(r) for r in d_dig.cpu().numpy().reshape(count, 16)] == want
        r = {"streams": count, "pcm_bytes": int(out.size), "a_decode_then_hashlib": row(t["a"], out.size),
             "b_decode_streams_md5": row(t["b"], out.size), "c_md5_spans_device": row(tc["c"], out.size),
             "b_plan": dict(zip(("launches", "synchronisations", "transfers", "channel_classes"), plan))}
        r["a_over_b"] = round(r["a_decode_then_hashlib"]["best_s"] / r["b_decode_streams_md5"]["best_s"], 2)
        return r, d_pcm

    res["streams_64"], _ = library(64)
    res["streams_%d" % args.streams], d_pcm = library(args.streams)

    # the optional length ordering: the same mixed-length spans in random order and sorted by descending length
    rng = np.random.default_rng(0x0DE2)
    count = args.streams
    ln = np.exp(rng.uniform(np.log(4096), np.log(1.25 * (1 << 20)), count)).astype(np.uint64)
    off = (rng.integers(0, d_pcm.numel() - int(ln.max()), count)).astype(np.uint64)
    order = np.argsort(-ln.astype(np.int64), kind="stable")
    d_dig = torch.zeros(count * 16, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    got = {}

    def spans(name, o, l_):
        def fn():
            h.md5_spans_device(d_pcm.data_ptr(), d_pcm.numel(), o, l_, d_dig.data_ptr())
            got[name] = d_dig.cpu().numpy().reshape(count, 16).copy()
        return fn
    t = alternate({"as_given": spans("as_given", off, ln), "descending": spans("descending", off[order], ln[order])},
                  args.reps)
    assert np.array_equal(got["as_given"][order], got["descending"])
    host = d_pcm.cpu().numpy()
    for s in order[:3].tolist() + order[-3:].tolist():
        assert got["as_given"][s].tobytes() == hashlib.md5(host[int(off[s]):int(off[s]) + int(ln[s])]).digest()
    mixed_bytes = int(ln.sum())
    res["ordering"] = {"spans": count, "bytes": mixed_bytes, "as_given": row(t["as_given"], mixed_bytes),
                       "descending": row(t["descending"], mixed_bytes),
                       "note": "timings include the download of the digests (32 KiB)"}
    del d_pcm, host

    # the documented bad case: one stream, one lane
    F = args.large_frames
    if F:
        big, big_lens, big_pcm = encode(h, F, 2, n, bps, 0xF1AC0001)
        out_big = np.zeros(big_pcm.size, np.uint8)
        table = np.zeros(1, _capi.STREAM_DESC_DTYPE)
        table[0] = (0, len(big), 0, out_big.size, 2, bps, n, 2)
        state = {}

        def host_path():
            _, call, _ = h.decode_streams(big, table, F, out_big)
            assert call == [F, F * n]
            state["host"] = hashlib.md5(out_big).digest()

        def device_path():
            _, call, _, digests = h.decode_streams_md5(big, table, F, out_big)
            assert call == [F, F * n]
            state["device"] = digests[0].tobytes()
        t = alternate({"a": host_path, "b": device_path}, max(1, args.reps - 1))
        assert state["host"] == state["device"] == hashlib.md5(big_pcm).digest()
        res["one_stream"] = {"frames": F, "channels": 2, "pcm_bytes": int(out_big.size),
                             "a_decode_then_hashlib": row(t["a"], out_big.size),
                             "b_decode_streams_md5": row(t["b"], out_big.size)}
    h.close()
    res["acceptance"] = {"b_faster_than_a_at_%d_streams" % args.streams:
                         bool(res["streams_%d" % args.streams]["b_decode_streams_md5"]["best_s"]
                              < res["streams_%d" % args.streams]["a_decode_then_hashlib"]["best_s"])}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))
    if not all(res["acceptance"].values()):
        raise SystemExit("decode_streams_md5 is not faster than decode_streams + hashlib at %d streams" % args.streams)


if __name__ == "__main__":
    main()
