"""Many .flac files -> .wav files with ONE call into the GPU library (flacenc_hip_decode_streams).

The host reads every file's metadata blocks (tools/decode_flac.py's parser), lays the files back to back in one buffer
and points one descriptor per file behind that file's metadata; the call indexes, decodes and packs all of them with a
number of launches that does not depend on how many there are.  The host then checks each STREAMINFO MD5 over the bytes
of that file's slot and writes the WAVs.  With --device-md5 the digests come out of the same call
(flacenc_hip_decode_streams_md5: one lane of the device per file hashes the PCM before it leaves the device) and the host
only compares 16 bytes per file; the lines printed and the exit codes are the same.

    python tools/decode_many.py a.flac b.flac ... --out-dir wavs [--device-md5]

With --through-errors (what `flac -F` does) the call is flacenc_hip_recover_streams: a damaged file no longer stops at
its first bad frame -- the decoder resynchronises on the next verified frame, places every frame where its header says
it belongs and writes silence where samples are lost.  Every file's recovered WAV is written and its frames, silence,
dropped frames and breaks are printed; the MD5 line of a file that lost anything reads "damaged".

    python tools/decode_many.py a.flac b.flac ... --out-dir wavs --through-errors
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from flacenc_rs_amd import _capi  # noqa: E402
import decode_flac  # noqa: E402


def device_md5_status(digest, info):
    """decode_flac.md5_status with the digest the device computed over the bytes of the file's slot."""
    if info["md5"] == bytes(16):
        return "MD5 not checked (STREAMINFO has none)"
    if bytes(digest) == info["md5"]:
        return "MD5 OK"
    return None


def decode_all(files, handle, device_md5=False):
    """files: the bytes of each .flac.  -> per file (PCM uint8 array, STREAMINFO) and, with device_md5, the 16 digest
    bytes of that PCM as the device computed them; raises on a stream that stops early."""
    table = np.zeros(len(files), _capi.STREAM_DESC_DTYPE)
    infos, at, out_at = [], 0, 0
    for i, data in enumerate(files):
        info, start = decode_flac.read_metadata(data)
        ch, bps = info["channels"], info["bits_per_sample"]
        decode_flac.allow_depth(handle, bps)
        width = (bps + 7) // 8
        n = len(data) - start
        room = (info["total_samples"] or (n // 9 + 1) * info["max_block_size"]) * ch * width
        table[i] = (at + start, n, out_at, room, ch, bps, info["max_block_size"], width)
        infos.append(info)
        at += len(data)
        out_at += room
    everything = np.frombuffer(b"".join(files), np.uint8)
    out = np.empty(max(1, out_at), np.uint8)
    max_frames = len(everything) // 9 + len(files)   # a frame is at least 9 bytes
    if device_md5:
        totals, call, _, digests = handle.decode_streams_md5(everything, table, max_frames, out)
    else:
        totals, call, _ = handle.decode_streams(everything, table, max_frames, out)
    if call[0] & _capi.INDEX_ERROR:
        raise ValueError("more frames or candidate headers than the call was given room for")
    results = []
    for i, info in enumerate(infos):
        frames, samples, consumed, why = (int(v) for v in totals[i])
        if why:
            name = decode_flac.STOP_NAMES.get(why, f"decode status {why:#x}")
            raise ValueError(f"file {i}: frame {frames} at byte {int(table[i]['offset']) - sum(map(len, files[:i])) + consumed}: {name}")
        lo = int(table[i]["out_offset"])
        pcm = out[lo:lo + samples * info["channels"] * int(table[i]["bytes_per_sample"])]
        results.append((pcm, info, digests[i].tobytes()) if device_md5 else (pcm, info))
    return results


def recover_all(files, handle):
    """files: the bytes of each .flac, damaged or not.  -> per file (PCM uint8 array: the defined prefix of its slot,
    silence where samples are lost; STREAMINFO; the file's eight totals of flacenc_hip_recover_streams; its gaps as
    (first sample, samples))."""
    table = np.zeros(len(files), _capi.STREAM_DESC_DTYPE)
    infos, at, out_at = [], 0, 0
    for i, data in enumerate(files):
        info, start = decode_flac.read_metadata(data)
        ch, bps = info["channels"], info["bits_per_sample"]
        decode_flac.allow_depth(handle, bps)
        width = (bps + 7) // 8
        n = len(data) - start
        room = (info["total_samples"] or (n // 9 + 1) * info["max_block_size"]) * ch * width
        table[i] = (at + start, n, out_at, room, ch, bps, info["max_block_size"], width)
        infos.append(info)
        at += len(data)
        out_at += room
    everything = np.frombuffer(b"".join(files), np.uint8)
    out = np.empty(max(1, out_at), np.uint8)
    max_frames = len(everything) // 9 + len(files)
    _, totals, gaps, call = handle.recover_streams(everything, table, max_frames, out, max_gaps=max_frames)
    if call[0] & _capi.INDEX_ERROR:
        raise ValueError("more frames or candidate headers than the call was given room for")
    results = []
    for i, info in enumerate(infos):
        lo = int(table[i]["out_offset"])
        W = info["channels"] * int(table[i]["bytes_per_sample"])
        mine = [(int(a), int(n)) for s, a, n in gaps if int(s) == i]
        results.append((out[lo:lo + int(totals[i][1]) * W], info, [int(v) for v in totals[i]], mine))
    return results


def recovered_status(pcm, info, totals):
    """The MD5 line of a recovered file: "damaged" in place of a mismatch."""
    complete = not any(totals[2:7]) and (not info["total_samples"] or totals[1] == info["total_samples"])
    return (decode_flac.md5_status(pcm, info) if complete else None) or "damaged"


def main_through_errors(args):
    files = [open(p, "rb").read() for p in args.inputs]
    with _capi.Handle(0) as h:
        results = recover_all(files, h)
    for path, (pcm, info, totals, gaps) in zip(args.inputs, results):
        wav = os.path.join(args.out_dir, os.path.splitext(os.path.basename(path))[0] + ".wav")
        decode_flac.write_wav(wav, pcm, info)
        print(f"{wav}: {totals[0]} frames, {totals[1]} samples x {info['channels']} channels, {totals[2]} of silence in "
              f"{len(gaps)} gaps, {totals[3]} frames dropped, {totals[5]} breaks"
              f"{', the output had no room' if totals[6] else ''}: {recovered_status(pcm, info, totals)}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("inputs", nargs="+")
    ap.add_argument("--out-dir", required=True)
    ap.add_argument("--device-md5", action="store_true",
                    help="take every file's MD5 from the device (flacenc_hip_decode_streams_md5), not from hashlib")
    ap.add_argument("--through-errors", action="store_true",
                    help="decode damaged files through their errors (flacenc_hip_recover_streams): silence where "
                         "samples are lost, every file's WAV written, its damage printed")
    args = ap.parse_args()
    os.makedirs(args.out_dir, exist_ok=True)
    if args.through_errors:
        return main_through_errors(args)
    files = [open(p, "rb").read() for p in args.inputs]
    with _capi.Handle(0) as h:
        results = decode_all(files, h, device_md5=args.device_md5)
    for path, (pcm, info, *digest) in zip(args.inputs, results):
        width = (info["bits_per_sample"] + 7) // 8
        samples = pcm.size // (info["channels"] * width)
        if info["total_samples"] and samples != info["total_samples"]:
            raise SystemExit(f"{path}: decoded {samples} samples, STREAMINFO says {info['total_samples']}")
        status = device_md5_status(digest[0], info) if args.device_md5 else decode_flac.md5_status(pcm, info)
        if status is None:
            raise SystemExit(f"{path}: MD5 mismatch")
        wav = os.path.join(args.out_dir, os.path.splitext(os.path.basename(path))[0] + ".wav")
        decode_flac.write_wav(wav, pcm, info)
        print(f"{wav}: {samples} samples x {info['channels']} channels, {info['bits_per_sample']} bits: {status}")


if __name__ == "__main__":
    main()
