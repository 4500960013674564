"""Decode, verify and index rates on the bench workload, and the same core on host threads.

The workload is bench.py's: 98 304 stereo frames of 4096 16-bit samples of sigen audio (Sine(200, 0.4) + Noise(0.4)),
LPC order 8, encoded and packed on the device by flacenc_hip_encode_pack_stereo_frames_async.  Timed on the device
with events (median of --reps after --warmup):
  decode   flacenc_hip_decode_frames_async on the strided pack output -> channel-major int32 rows
  verify   flacenc_hip_verify_frames_async of the same frames against the encoder's input
  index    flacenc_hip_index_frames_async on the frames placed back to back (flacenc_hip_place_frames_async)
  encode   the encode + pack launch the frames came from, for scale
  pack     flacenc_hip_pack_le_bytes on device pointers: the decoded rows -> packed interleaved 16-bit PCM (the call runs
           on the handle's stream and returns when it is done: host wall clock, not events)
HBM traffic counts the compressed bytes read plus 4 bytes per sample written (decode) or read (verify), against 8 TB/s;
for pack, 4 bytes per sample read plus 2 written.
The host boundary, wall clock and best of 3 on the first --host-frames frames (bench.py's streaming workload: 24 576),
frame bytes in host memory to interleaved PCM in host memory:
  decode_pcm pinned / pageable   flacenc_hip_decode_pcm with both buffers page-locked / both ordinary memory
  pieces                         what tools/decode_flac.py did before that call existed: upload + index, decode_frames to
                                 int32 host rows, numpy interleave per frame
The CPU baseline runs flac_decode_cpu.cpp (the same flac_decode_core.h, g++ -O2) on --threads host threads.
Writes profiles/decode_rates.json.

    python tools/time_decode.py [--frames 98304] [--threads 16]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from flacenc_rs_amd import _capi, decode_cpu  # noqa: E402

HBM_BYTES_PER_S = 8.0e12


def best_of(fn, reps=3):
    best = None
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        dt = time.perf_counter() - t0
        best = dt if best is None or dt < best else best
    return best


def host_boundary(h, args, x, stream_buf, starts, lens, n, bps):
    """Frame bytes in host memory -> interleaved PCM in host memory: flacenc_hip_decode_pcm, and the pieces without it."""
    import torch
    hf = min(args.host_frames, len(lens))
    n_bytes = int(starts[hf - 1]) + int(lens[hf - 1])
    pcm_bytes = hf * n * 2 * 2
    want = x[:hf].transpose(1, 2).contiguous().to(torch.int16).cpu().numpy().view(np.uint8).reshape(-1)
    src_pin, out_pin = _capi.pinned_array(n_bytes), _capi.pinned_array(pcm_bytes)
    src_pin[:] = stream_buf[:n_bytes].cpu().numpy()
    src_page, out_page = np.array(src_pin, copy=True), np.zeros(pcm_bytes, np.uint8)
    rows = {}
    for name, src, out in (("decode_pcm_pinned", src_pin, out_pin), ("decode_pcm_pageable", src_page, out_page)):
        def call():
            got, totals = h.decode_pcm(src, 2, bps, n, out=out)
            assert totals == [hf, hf * n, n_bytes, 0], totals
        call()   # warm: staging and scratch are allocated
        dt = best_of(call)
        assert np.array_equal(out, want)
        rows[name] = {"s": round(dt, 4), "G_samples_per_s": round(hf * 2 * n / dt / 1e9, 3),
                      "pcie_GB_per_s_in": round(n_bytes / dt / 1e9, 2), "pcie_GB_per_s_out": round(pcm_bytes / dt / 1e9, 2)}

    got = {}

    def pieces():
        off, ln, ok = h.index_frames(src_page, 2, bps, n_bytes // 9 + 1)
        assert ok
        out, bs, _, st = h.decode_frames(src_page, off, ln, 2, bps, n)
        assert not st.any()
        got["pcm"] = np.concatenate([out[f, :, :bs[f]].T for f in range(len(bs))])
    pieces()
    dt = best_of(pieces)
    assert np.array_equal(np.ascontiguousarray(got["pcm"].astype("<i2")).view(np.uint8).reshape(-1), want)
    rows["pieces"] = {"s": round(dt, 4), "G_samples_per_s": round(hf * 2 * n / dt / 1e9, 3),
                      "what": "index_frames + decode_frames to int32 host rows + numpy interleave per frame (the tool "
                              "before flacenc_hip_decode_pcm); its samples are still int32"}
    rows.update(frames=hf, compressed_bytes=n_bytes, pcm_bytes=pcm_bytes, timing="wall clock, best of 3 after one warm call")
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=98304)
    ap.add_argument("--block-size", type=int, default=4096)
    ap.add_argument("--lpc-order", type=int, default=8)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--cpu-frames", type=int, default=8192, help="frames the CPU baseline decodes")
    ap.add_argument("--host-frames", type=int, default=24576, help="frames of the host-boundary rows")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decode_rates.json"))
    args = ap.parse_args()
    import torch

    F, n, bps = args.frames, args.block_size, 16
    dev = torch.device("cuda", 0)
    h = _capi.Handle(0)
    x = torch.from_numpy(_capi.sigen_frames(F, 2, n, bps, 200.0, 0.4, 0.4, seed=0xF1AC0001)).to(dev)
    cfg = _capi.make_frame_config(_capi.make_config(lpc_order=args.lpc_order))
    stride = h.frame_bytes_bound(n, bps)
    stride = (stride + 15) // 16 * 16
    packed = torch.empty((F, stride), dtype=torch.uint8, device=dev)
    out_len = torch.zeros(F, dtype=torch.int32, device=dev)
    results = torch.empty((F, _capi.FRAME_RESULT_DTYPE.itemsize), dtype=torch.uint8, device=dev)
    s = torch.cuda.current_stream().cuda_stream

    def encode():
        h.encode_pack_stereo_frames_device(cfg, x.data_ptr(), F, n, n, bps, 44100, 0, 1, results.data_ptr(),
                                           packed.data_ptr(), stride, out_len.data_ptr(), stream=s)

    encode()
    torch.cuda.synchronize()
    lens = out_len.cpu().numpy().view(np.uint32)
    offsets = torch.arange(F, dtype=torch.int64, device=dev) * stride
    out = torch.empty((F * 2, n), dtype=torch.int32, device=dev)
    bs = torch.zeros(F, dtype=torch.int32, device=dev)
    nums = torch.zeros(F, dtype=torch.int64, device=dev)
    st = torch.zeros(F, dtype=torch.int32, device=dev)
    # the stream layout for the index: frames back to back
    starts = np.concatenate([np.zeros(1, np.uint64), np.cumsum(lens[:-1], dtype=np.uint64)])
    total = int(lens.sum(dtype=np.uint64))
    assert starts.dtype == np.uint64 and int(starts[-1]) + int(lens[-1]) == total and (lens > 0).all()
    soff = torch.from_numpy(starts.view(np.int64)).to(dev)
    stream_buf = torch.empty(total, dtype=torch.uint8, device=dev)
    h.place_frames_device(packed.data_ptr(), offsets.data_ptr(), out_len.data_ptr(), F, stream_buf.data_ptr(),
                          soff.data_ptr(), stream=s)
    ioff = torch.zeros(F + 8, dtype=torch.int64, device=dev)
    ilen = torch.zeros(F + 8, dtype=torch.int32, device=dev)
    inf = torch.zeros(1, dtype=torch.int64, device=dev)

    def decode():
        h.decode_frames_device(packed.data_ptr(), offsets.data_ptr(), out_len.data_ptr(), F, 2, bps, n, out.data_ptr(),
                               n, bs.data_ptr(), nums.data_ptr(), st.data_ptr(), stream=s)

    def verify():
        h.verify_frames_device(packed.data_ptr(), offsets.data_ptr(), out_len.data_ptr(), F, 2, bps, n, x.data_ptr(),
                               n, st.data_ptr(), stream=s)

    def index():
        h.index_frames_device(stream_buf.data_ptr(), total, 2, bps, F + 8, ioff.data_ptr(), ilen.data_ptr(),
                              inf.data_ptr(), stream=s)

    def timed(fn, blocking=False):
        for _ in range(args.warmup):
            fn()
        ms = []
        for _ in range(args.reps if not blocking else 0):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        for _ in range(args.reps if blocking else 0):   # the call synchronises its own stream: the host's clock
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            ms.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ms)), [round(v, 4) for v in ms]

    samples = F * 2 * n
    res = {"workload": f"bench.py's: {F} stereo frames x {n} samples, 16-bit sigen Sine(200,0.4)+Noise(0.4), "
                       f"LPC order {args.lpc_order}, encode_pack_stereo_frames_async output",
           "compressed_bytes": total, "samples": samples}
    pcm = torch.empty(samples * 2, dtype=torch.uint8, device=dev)
    ptotal = torch.zeros(1, dtype=torch.int64, device=dev)
    decode()   # rows and block sizes for pack
    torch.cuda.synchronize()

    def pack():
        h.pack_le_bytes_device(out.data_ptr(), n, bs.data_ptr(), F, 2, 2, pcm.data_ptr(), samples * 2, None,
                               ptotal.data_ptr())

    for name, fn in (("encode", encode), ("decode", decode), ("verify", verify), ("index", index), ("pack", pack)):
        med, all_ms = timed(fn, blocking=name == "pack")
        entry = {"ms_median": round(med, 4), "ms": all_ms, "G_samples_per_s": round(samples / med / 1e6, 2)}
        if name in ("decode", "verify"):
            traffic = total + 4 * samples
            entry["hbm_bytes"] = traffic
            entry["hbm_frac"] = round(traffic / (med * 1e-3) / HBM_BYTES_PER_S, 4)
        elif name == "index":
            entry["hbm_bytes"] = total
            entry["hbm_frac"] = round(total / (med * 1e-3) / HBM_BYTES_PER_S, 4)
        elif name == "pack":
            traffic = 6 * samples
            entry["hbm_bytes"] = traffic
            entry["hbm_GB_per_s"] = round(traffic / (med * 1e-3) / 1e9, 1)
            entry["hbm_frac"] = round(traffic / (med * 1e-3) / HBM_BYTES_PER_S, 4)
        res[name] = entry
    torch.cuda.synchronize()
    # correctness of what was timed
    decode()
    torch.cuda.synchronize()
    assert not st.any() and torch.equal(out.view(F, 2, n), x)
    verify()
    torch.cuda.synchronize()
    assert not st.any()
    index()
    torch.cuda.synchronize()
    assert int(inf.item()) == F and torch.equal(ioff[:F], soff)
    pack()
    torch.cuda.synchronize()
    want_pcm = x.transpose(1, 2).contiguous().to(torch.int16).view(torch.uint8).reshape(-1)   # [F, n, 2] int16
    assert int(ptotal.item()) == F * n and torch.equal(pcm, want_pcm)
    del want_pcm
    res["checked"] = "decode == input, verify all zero, index == place_frames offsets, pack == interleaved int16 input"
    res["host_boundary"] = host_boundary(h, args, x, stream_buf, starts, lens, n, bps)
    # CPU baseline: the same core on host threads
    cf = min(args.cpu_frames, F)
    host_bytes = packed[:cf].cpu().numpy().reshape(-1)
    host_off = np.arange(cf, dtype=np.uint64) * stride
    cpu = decode_cpu.DecoderCpu(decode_cpu.build())
    cpu.decode_frames(host_bytes, host_off, lens[:cf], 2, bps, n, threads=args.threads)
    t0 = time.perf_counter()
    cout, _, _, cst = cpu.decode_frames(host_bytes, host_off, lens[:cf], 2, bps, n, threads=args.threads)
    dt = time.perf_counter() - t0
    assert not cst.any() and np.array_equal(cout, x[:cf].cpu().numpy())
    res["cpu_baseline"] = {"threads": args.threads, "frames": cf, "s": round(dt, 4),
                           "G_samples_per_s": round(cf * 2 * n / dt / 1e9, 3),
                           "what": "flac_decode_cpu.cpp (flac_decode_core.h, g++ -O2), one frame per thread"}
    res["decode_vs_encode"] = round(res["decode"]["ms_median"] / res["encode"]["ms_median"], 3)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: (v if not isinstance(v, dict) else {kk: vv for kk, vv in v.items() if kk != "ms"})
                      for k, v in res.items()}))


if __name__ == "__main__":
    main()
