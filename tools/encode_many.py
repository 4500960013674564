"""Many WAV files to .flac files with ONE encode call and ONE digest call.

    python tools/encode_many.py a.wav b.wav ... --out-dir flacs [--block-size 4096] [--lpc-order 8] [--wasted-bits]
                                                  [--rice-escape] [--order-guess [K]]

Reads every WAV with the standard `wave` module (8 / 16 / 24-bit PCM, 1..8 channels; 8-bit WAV is offset binary and is
recentred), lays their samples back to back in one buffer, encodes all of them with flacenc_hip_encode_streams and takes
their STREAMINFO digests from flacenc_hip_md5_spans over the same spans.  Each .flac is "fLaC" + the 42-byte STREAMINFO
tools/encode_flac.py writes + the stream's frames; tools/decode_flac.py reads it back and checks the MD5.  Files may
differ in channels, width and rate: streams of one (channels, bits, bytes, rate) share their launches.

    python tools/encode_many.py --npy FILE [--lengths FILE] --bits N --rate R --out-dir DIR [the options above]

A [B, C, T] float32 (samples in [-1, 1)) or int32 array from a .npy file, item b valid up to lengths[b] samples (a .npy
of B integers; default T), to DIR/item00000.flac ...: ONE flacenc_hip_encode_streams_planar call
(flacenc_rs_amd.crops.encode_crops) reads the array as it lies and gives the frames and the STREAMINFO digests; no
packed copy of the samples is made on the way.  Prints how many elements clipped.
"""
import argparse
import os
import sys
import wave

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from flacenc_rs_amd import _capi  # noqa: E402
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from encode_flac import stream_info_block  # noqa: E402


def read_wav(path):
    """-> (packed interleaved little-endian signed PCM as uint8, channels, bits, width, rate, samples per channel)."""
    with wave.open(path, "rb") as w:
        ch, width, rate, n = w.getnchannels(), w.getsampwidth(), w.getframerate(), w.getnframes()
        if not (1 <= ch <= 8 and width in (1, 2, 3, 4)):
            raise SystemExit(f"{path}: {ch} channels of {8 * width} bits are not supported")
        raw = np.frombuffer(w.readframes(n), np.uint8)
    if width == 1:
        raw = (raw.astype(np.int16) - 128).astype(np.int8).view(np.uint8)
    return np.ascontiguousarray(raw), ch, 8 * width, width, rate, raw.size // (ch * width)


def encode_many(handle, wavs, block_size=4096, lpc_order=8, flags=0):
    """wavs: the tuples of read_wav -> one .flac byte string per file."""
    cfg = _capi.make_frame_config(_capi.make_config(lpc_order=lpc_order, flags=flags), use_fixed=True)
    lib = _capi.load()
    table = np.zeros(len(wavs), _capi.PCM_STREAM_DESC_DTYPE)
    at = out_at = 0
    for i, (raw, ch, bps, width, rate, n) in enumerate(wavs):
        bound = int(lib.flacenc_hip_stereo_frame_bytes_bound(block_size, bps) if ch == 2
                    else lib.flacenc_hip_frame_bytes_bound(ch, block_size, bps))
        cap = -(-n // block_size) * bound
        table[i] = (at, n, out_at, cap, ch, bps, width, rate)
        at += raw.size
        out_at += cap
    pcm = np.concatenate([w[0] for w in wavs]) if wavs else np.zeros(0, np.uint8)
    out = np.empty(max(1, out_at), np.uint8)
    if any(w[2] > 24 for w in wavs):  # 32-bit WAVs: the wide path, opt-in per handle
        handle.set_max_encode_bits_per_sample(32)
    lens, totals, call, _ = handle.encode_streams(pcm, table, cfg, block_size, out)
    digests = handle.md5_spans(pcm, table["offset"], [w[0].size for w in wavs])
    files = []
    for i, (raw, ch, bps, width, rate, n) in enumerate(wavs):
        frames, nbytes, first, why = (int(v) for v in totals[i])
        assert why == 0 and frames == -(-n // block_size)   # (every slot has the bound's room)
        sizes = lens[first:first + frames]
        head = stream_info_block(block_size, int(sizes.min()) if frames else 0, int(sizes.max()) if frames else 0, rate,
                                 ch, bps, n, digests[i].tobytes())
        o = int(table[i]["out_offset"])
        files.append(b"fLaC" + head + out[o:o + nbytes].tobytes())
    return files, call


def encode_array(handle, x, lengths, bits, rate, block_size=4096, lpc_order=8, flags=0):
    """x: [B, C, T] float32 / int32 numpy array -> (one .flac byte string per item, clip counts [B])."""
    import torch
    from flacenc_rs_amd import crops

    cfg = _capi.make_frame_config(_capi.make_config(lpc_order=lpc_order, flags=flags), use_fixed=True)
    if bits > 24:  # int32 elements alone; the wide path, opt-in per handle
        handle.set_max_encode_bits_per_sample(32)
    B, C, T = x.shape
    n = np.full(B, T, np.int64) if lengths is None else np.asarray(lengths, np.int64).reshape(-1)
    r = crops.encode_crops(handle, torch.from_numpy(np.ascontiguousarray(x)), n, bits, rate, cfg, block_size)
    frames, items, sizes = r["frames"].numpy(), r["items"].numpy(), r["frame_lengths"].numpy()
    first = np.concatenate([[0], np.cumsum(items[:, 2])])
    files = []
    for b in range(B):
        mine = sizes[first[b]:first[b + 1]]
        head = stream_info_block(block_size, int(mine.min()) if len(mine) else 0, int(mine.max()) if len(mine) else 0, rate,
                                 C, bits, int(n[b]), r["digests"][b].numpy().tobytes())
        files.append(b"fLaC" + head + frames[int(items[b, 0]):int(items[b, 0]) + int(items[b, 1])].tobytes())
    return files, r["clipped"].numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("wavs", nargs="*")
    ap.add_argument("--npy", help="a [B, C, T] float32 or int32 array in place of WAV files")
    ap.add_argument("--lengths", help="with --npy: a .npy of B valid lengths")
    ap.add_argument("--bits", type=int, help="with --npy: bits per sample, 8..24, or 25..32 for int32 elements (the wide path)")
    ap.add_argument("--rate", type=int, help="with --npy: the sample rate")
    ap.add_argument("--out-dir", required=True)
    ap.add_argument("--block-size", type=int, default=4096)
    ap.add_argument("--lpc-order", type=int, default=8)
    ap.add_argument("--wasted-bits", action="store_true")
    ap.add_argument("--rice-escape", action="store_true")
    ap.add_argument("--order-guess", type=int, nargs="?", const=1, default=0, metavar="K")
    args = ap.parse_args()
    flags = (_capi.FLAG_WASTED_BITS if args.wasted_bits else 0) | (_capi.FLAG_RICE_ESCAPE if args.rice_escape else 0)
    flags |= _capi.FLAG_ORDER_GUESS if args.order_guess else 0
    os.makedirs(args.out_dir, exist_ok=True)
    if args.npy:
        if args.wavs or args.bits is None or args.rate is None:
            raise SystemExit("--npy takes --bits and --rate and no WAV file")
        x = np.load(args.npy)
        if x.ndim != 3 or x.dtype not in (np.float32, np.int32):
            raise SystemExit(f"{args.npy}: a [B, C, T] float32 or int32 array is needed, not {x.dtype} {x.shape}")
        lengths = np.load(args.lengths) if args.lengths else None
        with _capi.Handle(0) as h:
            if args.order_guess:
                h.set_order_guesses(args.order_guess)
            files, clipped = encode_array(h, x, lengths, args.bits, args.rate, args.block_size, args.lpc_order, flags)
        for b, data in enumerate(files):
            with open(os.path.join(args.out_dir, "item%05d.flac" % b), "wb") as f:
                f.write(data)
        print(f"{len(files)} files, {sum(len(d) for d in files)} bytes, {int(clipped.sum())} elements clipped, one call")
        return
    if not args.wavs:
        raise SystemExit("WAV files or --npy are needed")
    wavs = [read_wav(p) for p in args.wavs]
    with _capi.Handle(0) as h:
        if args.order_guess:
            h.set_order_guesses(args.order_guess)
        files, call = encode_many(h, wavs, args.block_size, args.lpc_order, flags)
    pcm_bytes = 0
    for path, data, w in zip(args.wavs, files, wavs):
        name = os.path.splitext(os.path.basename(path))[0] + ".flac"
        with open(os.path.join(args.out_dir, name), "wb") as f:
            f.write(data)
        pcm_bytes += w[0].size
    print(f"{len(files)} files, {call[0]} frames, {call[1]} frame bytes, "
          f"{call[1] / max(1, pcm_bytes):.4f} of the PCM size, one encode call and one digest call")


if __name__ == "__main__":
    main()
