"""The counterpart of `flacenc decode`: .flac -> .wav with the frames indexed and decoded on the GPU.

The host reads the metadata blocks (it takes the stream's parameters and MD5 from STREAMINFO and skips every other
block); flacenc_hip_decode_pcm finds the frames, decodes them and returns the samples as packed interleaved
little-endian PCM -- the byte string the STREAMINFO MD5 is defined over.  The host checks that MD5 (an all-zero digest
means "not checked") and writes the WAV (8 / 16 / 24 / 32-bit PCM; a file of more than 24 bits per sample sets the
handle's depth limit to 32).

    python tools/decode_flac.py in.flac out.wav

With --through-errors a damaged file is decoded through its errors (flacenc_hip_recover_streams, tools/decode_many.py's
recover_all on the one file): silence where samples are lost, the damage printed, and "damaged" where the MD5 of a
file that lost anything could only mismatch.
"""
import argparse
import hashlib
import os
import sys
import wave

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from flacenc_rs_amd import _capi  # noqa: E402
import flac_metadata  # noqa: E402


def read_metadata(data: bytes):
    """-> (STREAMINFO fields, byte offset of the first frame)."""
    info, _, pos = flac_metadata.read_blocks(data)
    return info, pos


STOP_NAMES = {_capi.DECODE_NO_ROOM: "the output has no room", _capi.DECODE_CHAIN: "no verified frame starts here"}


def allow_depth(handle, bits_per_sample):
    """A file of more than 24 bits per sample raises the handle's limit to 32 (flacenc_hip_set_max_bits_per_sample);
    shallower files decode the same under either limit.  The limit is never lowered again: a caller's handle that
    has met one deep file (decode_many.py and crop_flac.py pass theirs in) stays at 32 for every later call on it."""
    if bits_per_sample > 24:
        handle.set_max_bits_per_sample(32)


def decode(data: bytes, handle):
    """-> (packed interleaved little-endian PCM, ceil(bits / 8) bytes per sample, as a uint8 array; STREAMINFO)."""
    info, start = read_metadata(data)
    frames = np.frombuffer(data, np.uint8)[start:]
    ch, bps = info["channels"], info["bits_per_sample"]
    allow_depth(handle, bps)
    width = (bps + 7) // 8
    if info["total_samples"]:
        room = info["total_samples"] * ch * width
    else:   # an unknown length: a frame is at least 9 bytes
        room = (len(frames) // 9 + 1) * info["max_block_size"] * ch * width
    out = np.empty(max(1, room), np.uint8)
    pcm, totals = handle.decode_pcm(frames, ch, bps, info["max_block_size"], out=out, out_capacity=room)
    if totals[3]:
        why = STOP_NAMES.get(totals[3], f"decode status {totals[3]:#x}")
        raise ValueError(f"frame {totals[0]} at byte {start + totals[2]}: {why}")
    return pcm, info


def wav_payload(pcm, bps):
    """The call's PCM bytes as the data of an 8 / 16 / 24 / 32-bit PCM WAV."""
    width = (bps + 7) // 8
    if 8 * width == bps and width > 1:
        return pcm.tobytes()   # 16 / 24 / 32 bits: the WAV payload as it stands
    # a depth that does not fill its bytes sits in the high bits of the WAV sample; 8-bit WAV is offset binary
    wide = np.zeros((pcm.size // width, 4), np.uint8)
    wide[:, :width] = pcm.reshape(-1, width)
    v = (wide.view("<i4").reshape(-1) << (32 - 8 * width)) >> (32 - 8 * width)   # sign-extend
    shifted = v.astype(np.int64) << (8 * width - bps)
    if width == 1:
        return (shifted + 128).astype(np.uint8).tobytes()
    return np.ascontiguousarray(shifted, "<i4").reshape(-1).view(np.uint8).reshape(-1, 4)[:, :width].tobytes()


def write_wav(path, pcm, info):
    with wave.open(path, "wb") as w:
        w.setnchannels(info["channels"])
        w.setsampwidth((info["bits_per_sample"] + 7) // 8)
        w.setframerate(info["sample_rate"])
        w.writeframes(wav_payload(pcm, info["bits_per_sample"]))


def md5_status(pcm, info):
    """The bytes the call returns are the ones the STREAMINFO MD5 is defined over; an all-zero digest means unchecked."""
    if info["md5"] == bytes(16):
        return "MD5 not checked (STREAMINFO has none)"
    if hashlib.md5(pcm).digest() == info["md5"]:
        return "MD5 OK"
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("input")
    ap.add_argument("output")
    ap.add_argument("--through-errors", action="store_true",
                    help="resynchronise behind damage and write silence where samples are lost")
    args = ap.parse_args()
    data = open(args.input, "rb").read()
    if args.through_errors:
        import decode_many
        with _capi.Handle(0) as h:
            pcm, info, totals, gaps = decode_many.recover_all([data], h)[0]
        write_wav(args.output, pcm, info)
        print(f"{totals[0]} frames, {totals[1]} samples x {info['channels']} channels, {info['bits_per_sample']} bits, "
              f"{totals[2]} of silence in {len(gaps)} gaps, {totals[3]} frames dropped, {totals[5]} breaks: "
              f"{decode_many.recovered_status(pcm, info, totals)}")
        return
    with _capi.Handle(0) as h:
        pcm, info = decode(data, h)
    bps = info["bits_per_sample"]
    width = (bps + 7) // 8
    samples = pcm.size // (info["channels"] * width)
    if info["total_samples"] and samples != info["total_samples"]:
        raise SystemExit(f"decoded {samples} samples, STREAMINFO says {info['total_samples']}")
    status = md5_status(pcm, info)
    if status is None:
        raise SystemExit("MD5 mismatch")
    write_wav(args.output, pcm, info)
    print(f"{samples} samples x {info['channels']} channels, {bps} bits: {status}")


if __name__ == "__main__":
    main()
