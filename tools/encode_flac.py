"""End-to-end demo: PCM -> .flac with every per-frame stage on the GPU.

Reads a 16/24/32-bit stereo WAV (or synthesises one), cuts it into 4096-sample frames, runs
flacenc_hip_encode_stereo_frames (analysis + encode_frame's decisions) and
flacenc_hip_pack_stereo_frames (Frame::write), and writes "fLaC" + STREAMINFO + the frames.
What stays on the host is what the reference keeps serial too: the container's 42 bytes and the
MD5 of the input (src/source.rs:406-428).  A short tail block is a second (one-frame) batch: the
frame-level entry points take any block size.

    python tools/encode_flac.py [in.wav] out.flac [--seconds 10] [--levels L] [--wasted-bits] [--order-search]
                                  [--window-search] [--order-guess [K]] [--precision-search [FLOOR]] [--rice-escape]
                                  [--seektable SECONDS] [--bits N]

More than 24 bits per sample -- a 32-bit WAV, or --bits N on the synthetic source -- go through flacenc_hip_encode_pcm on
the wide path after flacenc_hip_set_max_encode_bits_per_sample(h, 32): fixed predictors on 64-bit integers, of the
switches only --wasted-bits and --seektable apply, and STREAMINFO says the depth.
With --levels L the stream is variable-blocking: flacenc_hip_encode_variable codes each superblock of 4096 samples as
the tiling into blocks of 4096 .. 4096 / 2^(L-1) that is shortest, and STREAMINFO announces the smallest chosen block
(the last frame aside) and 4096 as the block-size range.
With --wasted-bits (FLACENC_HIP_FLAG_WASTED_BITS) a subframe whose samples all end in k zero bits -- 16-bit content in a
24-bit WAV, say -- is coded as x >> k at bits_per_sample - k bits; the reference never writes them, every decoder reads
them.
With --order-search (FLACENC_HIP_FLAG_ORDER_SEARCH) every LPC subframe's order is the one of 1..--lpc-order whose exact
bit count is smallest; the histogram of the chosen orders is printed.
With --window-search (FLACENC_HIP_FLAG_WINDOW_SEARCH) every LPC subframe is also analysed under the default extra windows
(partial and punch-out Tukey windows, _capi.DEFAULT_LPC_WINDOWS) and the shortest result is coded.
With --order-guess [K] (FLACENC_HIP_FLAG_ORDER_GUESS, libFLAC's default mode) the order of every LPC subframe is guessed
from the Levinson prediction error: --lpc-order and the K guesses (default 1) per window are coded and the shortest kept;
the histogram of the chosen orders is printed.  Not together with --order-search.
With --precision-search [FLOOR] (FLACENC_HIP_FLAG_PRECISION_SEARCH, libFLAC's -p) every LPC subframe is coded at each
coefficient precision from 15 down to FLOOR (default 5) and the shortest kept; the histogram of the chosen precisions is
printed.  Composes with the three searches above.
With --rice-escape (FLACENC_HIP_FLAG_RICE_ESCAPE) a Rice partition is stored escaped -- raw samples of a 5-bit-coded
width, 9 bits for a partition of digital silence -- where that is strictly shorter; how many partitions and frames
escaped is printed.  The flag trades the fused kernels for the general path.  tools/decode_flac.py reads the result back.
With --seektable SECONDS a SEEKTABLE block follows STREAMINFO: one point per SECONDS, from the frame lengths the call
returned (sample number, byte offset from the first frame, block size).  Without it the file is what it has always been.
"""
import argparse
import hashlib
import os
import struct
import sys
import wave

import numpy as np

sys.path.insert(0, os.environ.get("GRAFT_REPO_ROOT", os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from flacenc_rs_amd import _capi  # noqa: E402
import flac_metadata  # noqa: E402


def stream_info_block(block_size, min_frame, max_frame, rate, channels, bps, total, md5, min_block=None, last=True):
    """MetadataBlock(StreamInfo)::write, src/component/bitrepr.rs:199-270 (last-block flag set unless a SEEKTABLE
    follows); min_block for a variable-blocking stream (default: block_size, a fixed-blocking one)."""
    body = struct.pack(">HH", block_size if min_block is None else min_block, block_size)
    body += min_frame.to_bytes(3, "big") + max_frame.to_bytes(3, "big")
    packed = (rate << 44) | ((channels - 1) << 41) | ((bps - 1) << 36) | total
    body += packed.to_bytes(8, "big") + md5
    return bytes([0x80 if last else 0]) + len(body).to_bytes(3, "big") + body


def seektable_for(frame_lengths, block_sizes, rate, seconds):
    """The SEEKTABLE block (the last metadata block) with one point per `seconds`, from what the encoder already has."""
    points = flac_metadata.seek_points(frame_lengths, block_sizes, max(1, int(round(seconds * rate))))
    return flac_metadata.seektable_block(points, last=True)


def md5_of(frames, bps):
    """Source MD5: interleaved little-endian samples of ceil(bps / 8) bytes, src/source.rs:406-428."""
    inter = np.ascontiguousarray(frames.transpose(0, 2, 1)).reshape(-1)
    nbytes = (bps + 7) // 8
    raw = inter.astype("<i4").view(np.uint8).reshape(-1, 4)[:, :nbytes]
    return hashlib.md5(raw.tobytes()).digest()


def encode_pcm(pcm, bps, rate, handle, block_size=4096, use_fixed=True, lpc_order=8, flags=0, seektable=None):
    """pcm int32 [n_samples, 2] -> (.flac bytes, per-frame decision records).  Like
    encode_with_fixed_block_size (src/coding.rs:645-700): whole blocks, then the shorter last one.  seektable: seconds
    between seek points of a SEEKTABLE block behind STREAMINFO (None: none, the file as it has always been)."""
    cfg = _capi.make_frame_config(_capi.make_config(lpc_order=lpc_order, flags=flags), use_fixed=use_fixed)
    n_full = pcm.shape[0] // block_size
    groups = []
    if n_full:
        groups.append(np.ascontiguousarray(pcm[: n_full * block_size].reshape(n_full, block_size, 2).transpose(0, 2, 1)))
    tail = pcm.shape[0] - n_full * block_size
    if tail:
        groups.append(np.ascontiguousarray(pcm[n_full * block_size:].T[None]))
    packed, records, first = [], [], 0
    for g in groups:
        if g.shape[2] < 64:   # blocks below MIN_BLOCK_SIZE_FOR_PREDICTION (constant.rs:51) never reach the GPU path
            raise ValueError("a tail block shorter than 64 samples is not supported by this demo")
        res, resid = handle.encode_stereo_frames(g, bps, cfg)
        packed += handle.pack_stereo_frames(g, res, resid, bps, rate, first_frame_number=first)
        records.append(res)
        first += g.shape[0]
    inter = np.ascontiguousarray(pcm).reshape(-1)
    nbytes = (bps + 7) // 8
    md5 = hashlib.md5(inter.astype("<i4").view(np.uint8).reshape(-1, 4)[:, :nbytes].tobytes()).digest()
    sizes = list(map(len, packed))
    # fixed-block streams announce the block size as both min and max (src/coding.rs:676-690)
    head = b"fLaC" + stream_info_block(block_size, min(sizes), max(sizes), rate, 2, bps, pcm.shape[0], md5,
                                       last=seektable is None)
    if seektable is not None:
        head += seektable_for(sizes, [g.shape[2] for g in groups for _ in range(g.shape[0])], rate, seektable)
    return head + b"".join(packed), np.concatenate(records)


def encode_pcm_deep(pcm, bps, rate, handle, block_size=4096, flags=0, seektable=None):
    """pcm int32 [n_samples, channels] of 25..32 bits -> (.flac bytes, frame lengths): flacenc_hip_encode_pcm on the wide
    path (Constant, Verbatim, fixed predictors by exact bit counts; a 33-bit side channel for two channels), which the
    handle takes after flacenc_hip_set_max_encode_bits_per_sample(h, 32).  STREAMINFO says `bps`."""
    handle.set_max_encode_bits_per_sample(32)
    cfg = _capi.make_frame_config(_capi.make_config(flags=flags & _capi.FLAG_WASTED_BITS), use_fixed=True,
                                  fixed_order_sel=_capi.ORDERSEL_BITCOUNT)
    total, channels = pcm.shape
    raw = np.ascontiguousarray(pcm).astype("<i4").view(np.uint8).reshape(-1)
    data, lens = handle.encode_pcm(raw, channels, cfg, 4, bps, block_size, rate, frame_number_step=1)
    sizes = [int(v) for v in lens]
    head = b"fLaC" + stream_info_block(block_size, min(sizes), max(sizes), rate, channels, bps, total,
                                       hashlib.md5(raw.tobytes()).digest(), last=seektable is None)
    if seektable is not None:
        blocks = [min(block_size, total - t) for t in range(0, total, block_size)]
        head += seektable_for(sizes, blocks, rate, seektable)
    return head + data.tobytes(), np.array(sizes)


def encode_pcm_variable(pcm, bps, rate, handle, block_size=4096, levels=3, use_fixed=True, lpc_order=8, flags=0,
                        seektable=None):
    """pcm int32 [n_samples, channels] -> (.flac bytes, dict of encode_variable's outputs): the block-size search over
    superblocks of block_size samples, written as a variable-blocking stream."""
    cfg = _capi.make_frame_config(_capi.make_config(lpc_order=lpc_order, flags=flags), use_fixed=use_fixed)
    total, channels = pcm.shape
    n_sb = (total + block_size - 1) // block_size
    rows = np.zeros((n_sb * block_size, channels), np.int32)
    rows[:total] = pcm
    frames = np.ascontiguousarray(rows.reshape(n_sb, block_size, channels).transpose(0, 2, 1))
    v = handle.encode_variable(frames, bps, cfg, levels, total_samples=total, sample_rate=rate)
    inter = np.ascontiguousarray(pcm).reshape(-1)
    nbytes = (bps + 7) // 8
    md5 = hashlib.md5(inter.astype("<i4").view(np.uint8).reshape(-1, 4)[:, :nbytes].tobytes()).digest()
    sizes, blocks = v["lengths"], v["block_sizes"]
    # RFC 9639 section 8.2: the minimum block size excludes the last block
    min_block = int(blocks[:-1].min()) if len(blocks) > 1 else int(blocks[0])
    head = b"fLaC" + stream_info_block(block_size, int(sizes.min()), int(sizes.max()), rate, channels, bps, total, md5,
                                       min_block=min_block, last=seektable is None)
    if seektable is not None:
        head += seektable_for(sizes, blocks, rate, seektable)
    return head + v["data"], v


def encode(frames, bps, rate, handle, use_fixed=True, lpc_order=8):
    """frames int32 [n_frames, 2, n] (whole blocks only) -> (.flac bytes, records)."""
    pcm = np.ascontiguousarray(frames.transpose(0, 2, 1)).reshape(-1, 2)
    return encode_pcm(pcm, bps, rate, handle, block_size=frames.shape[2], use_fixed=use_fixed, lpc_order=lpc_order)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("paths", nargs="+")
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--levels", type=int, default=0, help="block-size search over 1..5 levels (variable blocking)")
    ap.add_argument("--wasted-bits", action="store_true",
                    help="code subframes whose low bits are all zero at reduced width (FLACENC_HIP_FLAG_WASTED_BITS)")
    ap.add_argument("--order-search", action="store_true",
                    help="search the LPC order of every subframe (FLACENC_HIP_FLAG_ORDER_SEARCH)")
    ap.add_argument("--window-search", action="store_true",
                    help="analyse every LPC subframe under the config's window and the default extra windows, keep the "
                         "shortest (FLACENC_HIP_FLAG_WINDOW_SEARCH); composes with --order-search")
    ap.add_argument("--order-guess", type=int, nargs="?", const=1, default=0, metavar="K",
                    help="guess the LPC order of every subframe from the Levinson error and code --lpc-order and the K "
                         "guesses per window, K in 1..32, default 1 (FLACENC_HIP_FLAG_ORDER_GUESS); composes with "
                         "--window-search, not with --order-search")
    ap.add_argument("--precision-search", type=int, nargs="?", const=_capi.DEFAULT_PRECISION_FLOOR, default=0,
                    metavar="FLOOR",
                    help="code every LPC subframe at each coefficient precision from 15 down to FLOOR, 1..15, default 5, "
                         "and keep the shortest (FLACENC_HIP_FLAG_PRECISION_SEARCH); composes with the other searches")
    ap.add_argument("--rice-escape", action="store_true",
                    help="store a Rice partition escaped (raw samples of a 5-bit-coded width) where that is strictly "
                         "shorter (FLACENC_HIP_FLAG_RICE_ESCAPE: the general path for every shape); composes with every "
                         "other switch")
    ap.add_argument("--seektable", type=float, default=None, metavar="SECONDS",
                    help="write a SEEKTABLE block with one seek point per SECONDS (tools/crop_flac.py starts at them)")
    ap.add_argument("--lpc-order", type=int, default=8)
    ap.add_argument("--bits", type=int, default=0, metavar="N",
                    help="the synthetic source at N bits per sample (16-bit content shifted); more than 24 bits, like a "
                         "32-bit WAV, takes the wide path (flacenc_hip_set_max_encode_bits_per_sample) and STREAMINFO says N")
    args = ap.parse_args()
    if args.order_guess and args.order_search:
        ap.error("--order-guess and --order-search exclude each other")
    if args.order_guess < 0 or args.order_guess > 32:
        ap.error("--order-guess K must be in 1..32")
    flags = (_capi.FLAG_WASTED_BITS if args.wasted_bits else 0) | (_capi.FLAG_ORDER_SEARCH if args.order_search else 0)
    flags |= _capi.FLAG_WINDOW_SEARCH if args.window_search else 0  # (a fresh handle holds DEFAULT_LPC_WINDOWS)
    flags |= _capi.FLAG_ORDER_GUESS if args.order_guess else 0
    if args.precision_search < 0 or args.precision_search > 15:
        ap.error("--precision-search FLOOR must be in 1..15")
    flags |= _capi.FLAG_PRECISION_SEARCH if args.precision_search else 0
    flags |= _capi.FLAG_RICE_ESCAPE if args.rice_escape else 0
    handle = _capi.Handle(0)
    if args.precision_search:
        handle.set_precision_floor(args.precision_search)
    if args.order_guess:
        handle.set_order_guesses(args.order_guess)
    n = 4096
    if len(args.paths) == 2:
        with wave.open(args.paths[0], "rb") as w:
            assert w.getnchannels() == 2 and w.getsampwidth() in (2, 3, 4)
            bps, rate = 8 * w.getsampwidth(), w.getframerate()
            raw = np.frombuffer(w.readframes(w.getnframes()), np.uint8).reshape(-1, 2, w.getsampwidth())
        pad = np.zeros(raw.shape[:2] + (4 - raw.shape[2],), np.uint8)
        pcm = (np.concatenate([pad, raw], axis=2).view("<i4")[..., 0] >> (32 - bps)).astype(np.int32)
    else:
        bps, rate = 16, 44100
        nsamp = max(n, int(args.seconds * rate))
        nf = (nsamp + n - 1) // n
        pcm = np.ascontiguousarray(_capi.sigen_frames(nf, 2, n, bps, rate / 440.0, 0.8, 0.2, seed=1)
                                   .transpose(0, 2, 1)).reshape(-1, 2)[:nsamp]
    if args.bits:
        assert len(args.paths) == 1 and 8 <= args.bits <= 32, "--bits N (8..32) goes with the synthetic source"
        bps, pcm = args.bits, pcm << (args.bits - 16) if args.bits >= 16 else pcm >> (16 - args.bits)
    if bps > 24:
        if args.levels:
            ap.error("--levels stops at 24 bits per sample")
        data, sizes = encode_pcm_deep(pcm, bps, rate, handle, block_size=n, flags=flags, seektable=args.seektable)
        with open(args.paths[-1], "wb") as f:
            f.write(data)
        print(f"{len(sizes)} frames, {len(data)} bytes, {len(data) / (pcm.shape[0] * 2 * 4):.4f} of the PCM size; "
              f"{bps} bits per sample on the wide path")
        return
    if args.levels:
        data, v = encode_pcm_variable(pcm, bps, rate, handle, block_size=n, levels=args.levels,
                                      lpc_order=args.lpc_order, flags=flags, seektable=args.seektable)
        with open(args.paths[-1], "wb") as f:
            f.write(data)
        sizes = np.bincount(v["block_sizes"]).nonzero()[0]
        print(f"{v['frames']} frames, {len(data)} bytes, {len(data) / (pcm.shape[0] * 2 * bps / 8):.4f} of the PCM "
              f"size; block sizes {dict((int(b), int((v['block_sizes'] == b).sum())) for b in sizes)}")
        return
    data, res = encode_pcm(pcm, bps, rate, handle, block_size=n, lpc_order=args.lpc_order, flags=flags,
                           seektable=args.seektable)
    nf = len(res)
    with open(args.paths[-1], "wb") as f:
        f.write(data)
    kinds = np.bincount(res["kind"].ravel(), minlength=4)
    wasted = int((res["pad"] != 0).sum())
    print(f"{nf} frames, {len(data)} bytes, {len(data) / (pcm.shape[0] * 2 * bps / 8):.4f} of the PCM size; "
          f"subframes constant/verbatim/fixed/lpc = {kinds.tolist()}, with wasted bits {wasted}")
    if args.order_search or args.order_guess:
        orders = res["lpc"]["order"][res["kind"] == 3]
        hist = np.bincount(orders, minlength=args.lpc_order + 1)
        print("chosen LPC orders: " + ", ".join(f"{o}: {int(c)}" for o, c in enumerate(hist) if c))
    if args.rice_escape:
        coded = (res["kind"] >= 2)[..., None] & (np.arange(256) < (1 << res["lpc"]["rice_order"].astype(np.int64))[..., None])
        marks = coded & ((res["lpc"]["rice_params"] & 0x80) != 0)
        print(f"escaped partitions: {int(marks.sum())} of {int(coded.sum())}, in {int(marks.any(axis=(1, 2)).sum())} of "
              f"{nf} frames")
    if args.precision_search:
        hist = np.bincount(res["lpc"]["precision"][res["kind"] == 3], minlength=16)
        print("chosen LPC precisions: " + ", ".join(f"{q}: {int(c)}" for q, c in enumerate(hist) if c))


if __name__ == "__main__":
    main()
