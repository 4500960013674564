"""The same crop out of many .flac files -> .wav files with ONE call into the GPU library (flacenc_hip_decode_ranges).

The host reads every file's STREAMINFO and, if it has one, its SEEKTABLE (tools/flac_metadata.py); each file's span
starts at the last seek point at or before the crop (placeholder points are skipped; without a SEEKTABLE, at the first
frame) and ends with the file, and its range is the crop counted from that seek point's sample number.  The call
decodes only the frames the crops touch and returns only the crops.  A crop that runs past a file's end is written as
far as the file goes.

    python tools/crop_flac.py a.flac b.flac ... --start S --seconds T --out-dir wavs

--npy FILE also writes the crops as one float32 array [files, channels, samples], the batch a model is fed, from one
flacenc_hip_decode_ranges_planar call; the files must then agree on channels and sample rate.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from flacenc_rs_amd import _capi  # noqa: E402
import decode_flac  # noqa: E402
import flac_metadata  # noqa: E402


def crop_all(files, handle, start_seconds, seconds):
    """files: the bytes of each .flac.  -> per file (PCM uint8 array of the crop, STREAMINFO, the seek point used)."""
    table = np.zeros(len(files), _capi.STREAM_DESC_DTYPE)
    ranges = np.zeros(len(files), _capi.RANGE_DESC_DTYPE)
    infos, seeks, at, out_at = [], [], 0, 0
    for i, data in enumerate(files):
        info, points, first_frame = flac_metadata.read_blocks(data)
        ch, bps = info["channels"], info["bits_per_sample"]
        decode_flac.allow_depth(handle, bps)
        width = (bps + 7) // 8
        first = int(round(start_seconds * info["sample_rate"]))
        n = int(round(seconds * info["sample_rate"]))
        seek = flac_metadata.last_point_at_or_before(points, first)
        begin = first_frame + seek[1]
        if begin > len(data):
            raise ValueError(f"file {i}: a seek point behind the end of the file")
        table[i] = (at + begin, len(data) - begin, 0, 0, ch, bps, info["max_block_size"], width)
        ranges[i] = (first - seek[0], n, out_at, i, 0)
        infos.append(info)
        seeks.append(seek)
        at += len(data)
        out_at += n * ch * width
    everything = np.frombuffer(b"".join(files), np.uint8)
    out = np.empty(max(1, out_at), np.uint8)
    max_frames = len(everything) // 9 + len(files)   # a frame is at least 9 bytes
    totals, call, _ = handle.decode_ranges(everything, table, ranges, max_frames, out)
    if call[0] & _capi.INDEX_ERROR:
        raise ValueError("more frames or candidate headers than the call was given room for")
    results = []
    for i, info in enumerate(infos):
        written, why = int(totals[i][0]), int(totals[i][1])
        if why not in (0, _capi.DECODE_RANGE_END):
            name = decode_flac.STOP_NAMES.get(why, f"decode status {why:#x}")
            raise ValueError(f"file {i}: stopped {written} samples into the crop: {name}")
        lo = int(ranges[i]["out_offset"])
        results.append((out[lo:lo + written * info["channels"] * int(table[i]["bytes_per_sample"])], info, seeks[i]))
    return results


def crop_all_planar(files, handle, start_seconds, seconds):
    """The same crops as one float32 array [files, channels, samples] in [-1, 1) from ONE
    flacenc_hip_decode_ranges_planar call: the files must agree on the channel count and on the crop's length in
    samples; a crop that runs past its file's end is zero from there on.  -> (the array, per file (samples written,
    STREAMINFO, the seek point used))."""
    table = np.zeros(len(files), _capi.STREAM_DESC_DTYPE)
    ranges = np.zeros(len(files), _capi.RANGE_DESC_DTYPE)
    infos, seeks, at = [], [], 0
    shape = None
    for i, data in enumerate(files):
        info, points, first_frame = flac_metadata.read_blocks(data)
        ch, bps = info["channels"], info["bits_per_sample"]
        decode_flac.allow_depth(handle, bps)
        first = int(round(start_seconds * info["sample_rate"]))
        n = int(round(seconds * info["sample_rate"]))
        shape = shape or (ch, n)
        if (ch, n) != shape:
            raise ValueError(f"file {i}: {ch} channels x {n} samples, the first file has {shape[0]} x {shape[1]}: one "
                             "array holds one shape")
        seek = flac_metadata.last_point_at_or_before(points, first)
        begin = first_frame + seek[1]
        if begin > len(data):
            raise ValueError(f"file {i}: a seek point behind the end of the file")
        table[i] = (at + begin, len(data) - begin, 0, 0, ch, bps, info["max_block_size"], (bps + 7) // 8)
        ranges[i] = (first - seek[0], n, i * ch * n * 4, i, 0)
        infos.append(info)
        seeks.append(seek)
        at += len(data)
    everything = np.frombuffer(b"".join(files), np.uint8)
    out = np.empty((len(files),) + shape, np.float32)
    room = out if out.size else np.empty(1, np.float32)
    max_frames = len(everything) // 9 + len(files)   # a frame is at least 9 bytes
    totals, call, _ = handle.decode_ranges_planar(everything, table, ranges, max_frames, room, _capi.SAMPLE_F32)
    if call[0] & _capi.INDEX_ERROR:
        raise ValueError("more frames or candidate headers than the call was given room for")
    notes = []
    for i, info in enumerate(infos):
        written, why = int(totals[i][0]), int(totals[i][1])
        if why not in (0, _capi.DECODE_RANGE_END):
            name = decode_flac.STOP_NAMES.get(why, f"decode status {why:#x}")
            raise ValueError(f"file {i}: stopped {written} samples into the crop: {name}")
        notes.append((written, info, seeks[i]))
    return out, notes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("inputs", nargs="+")
    ap.add_argument("--start", type=float, required=True, help="where the crop begins, in seconds")
    ap.add_argument("--seconds", type=float, required=True, help="how long the crop is")
    ap.add_argument("--out-dir", required=True)
    ap.add_argument("--npy", metavar="FILE", help="also write the crops as one float32 array [files, channels, samples] "
                                                  "in [-1, 1), zero behind a file's end (flacenc_hip_decode_ranges_planar)")
    args = ap.parse_args()
    if args.start < 0 or args.seconds < 0:
        ap.error("--start and --seconds are not negative")
    os.makedirs(args.out_dir, exist_ok=True)
    files = [open(p, "rb").read() for p in args.inputs]
    with _capi.Handle(0) as h:
        results = crop_all(files, h, args.start, args.seconds)
        if args.npy:
            batch, notes = crop_all_planar(files, h, args.start, args.seconds)
            np.save(args.npy, batch)
            print(f"{args.npy}: float32 {list(batch.shape)}, samples written per file {[w for w, _, _ in notes]}")
    for path, (pcm, info, seek) in zip(args.inputs, results):
        width = (info["bits_per_sample"] + 7) // 8
        samples = pcm.size // (info["channels"] * width)
        wav = os.path.join(args.out_dir, os.path.splitext(os.path.basename(path))[0] + ".wav")
        decode_flac.write_wav(wav, pcm, info)
        print(f"{wav}: {samples} samples x {info['channels']} channels from sample "
              f"{int(round(args.start * info['sample_rate']))}, decoded from the seek point at sample {seek[0]}")


if __name__ == "__main__":
    main()
