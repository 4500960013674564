"""The counterpart of `flacenc decode`: .flac -> .wav with the frames indexed and decoded on the GPU.

The host reads the metadata blocks (it takes the stream's parameters and MD5 from STREAMINFO and skips every other
block), flacenc_hip_index_frames_async finds the frames, flacenc_hip_decode_frames decodes them, and the host
interleaves the samples, checks the MD5 against STREAMINFO (an all-zero digest means "not checked") and writes the
WAV (8 / 16 / 24-bit PCM).

    python tools/decode_flac.py in.flac out.wav
"""
import argparse
import hashlib
import os
import struct
import sys
import wave

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from flacenc_rs_amd import _capi  # noqa: E402


def read_metadata(data: bytes):
    """-> (STREAMINFO fields, byte offset of the first frame)."""
    if data[:4] != b"fLaC":
        raise ValueError("not a FLAC stream")
    pos, info = 4, None
    while True:
        head = data[pos]
        kind, size = head & 0x7F, int.from_bytes(data[pos + 1:pos + 4], "big")
        body = data[pos + 4:pos + 4 + size]
        if kind == 0:
            max_block = struct.unpack(">H", body[2:4])[0]
            packed = int.from_bytes(body[10:18], "big")
            info = dict(max_block_size=max_block, sample_rate=packed >> 44, channels=((packed >> 41) & 7) + 1,
                        bits_per_sample=((packed >> 36) & 31) + 1, total_samples=packed & ((1 << 36) - 1),
                        md5=bytes(body[18:34]))
        pos += 4 + size
        if head & 0x80:
            break
    if info is None:
        raise ValueError("no STREAMINFO block")
    return info, pos


def decode(data: bytes, handle):
    """-> (interleaved int32 samples [total, channels], STREAMINFO)."""
    info, start = read_metadata(data)
    frames = data[start:]
    ch, bps = info["channels"], info["bits_per_sample"]
    max_frames = len(frames) // 9 + 1  # a frame is at least 9 bytes
    offsets, lengths, ok = handle.index_frames(frames, ch, bps, max_frames)
    if not ok:
        raise ValueError("the frames do not chain from the first to the end of the file")
    out, bs, _, st = handle.decode_frames(frames, offsets, lengths, ch, bps, info["max_block_size"])
    if st.any():
        f = int(np.flatnonzero(st)[0])
        raise ValueError(f"frame {f} at byte {start + int(offsets[f])}: decode status {int(st[f]):#x}")
    pcm = np.concatenate([out[f, :, :bs[f]].T for f in range(len(bs))]) if len(bs) else np.zeros((0, ch), np.int32)
    return pcm, info


def md5_of(pcm, bps):
    """Interleaved little-endian samples of ceil(bps / 8) bytes (src/source.rs:406-428 of the reference)."""
    nbytes = (bps + 7) // 8
    raw = np.ascontiguousarray(pcm, "<i4").reshape(-1).view(np.uint8).reshape(-1, 4)[:, :nbytes]
    return hashlib.md5(raw.tobytes()).digest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("input")
    ap.add_argument("output")
    args = ap.parse_args()
    data = open(args.input, "rb").read()
    with _capi.Handle(0) as h:
        pcm, info = decode(data, h)
    bps = info["bits_per_sample"]
    if info["total_samples"] and pcm.shape[0] != info["total_samples"]:
        raise SystemExit(f"decoded {pcm.shape[0]} samples, STREAMINFO says {info['total_samples']}")
    if info["md5"] == bytes(16):
        status = "MD5 not checked (STREAMINFO has none)"
    elif md5_of(pcm, bps) == info["md5"]:
        status = "MD5 OK"
    else:
        raise SystemExit("MD5 mismatch")
    width = (bps + 7) // 8
    shifted = pcm.astype(np.int64) << (8 * width - bps)
    if width == 1:
        raw = (shifted + 128).astype(np.uint8).tobytes()
    else:
        raw = np.ascontiguousarray(shifted, "<i4").reshape(-1).view(np.uint8).reshape(-1, 4)[:, :width].tobytes()
    with wave.open(args.output, "wb") as w:
        w.setnchannels(info["channels"])
        w.setsampwidth(width)
        w.setframerate(info["sample_rate"])
        w.writeframes(raw)
    print(f"{pcm.shape[0]} samples x {info['channels']} channels, {bps} bits: {status}")


if __name__ == "__main__":
    main()
