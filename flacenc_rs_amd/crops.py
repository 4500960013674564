"""A batch of crops of FLAC streams as one torch tensor: flacenc_hip_decode_ranges_planar writes every crop's samples as
planar float32 (or int32) rows straight into a [B, C, T] tensor, so nothing touches the data between the decoder and the
model -- no widening, no transpose, no scaling, no padding, no per-crop copy."""
import numpy as np

from . import _capi

__all__ = ["decode_crops"]


def decode_crops(handle, d_bytes, streams, crops, T, dtype=None, max_frames=None):
    """Crops of T samples from streams of one channel count C -> (tensor [B, C, T], totals).

    handle     a _capi.Handle
    d_bytes    1-D torch.uint8 tensor that holds every stream's frames; on the handle's GPU (the call runs in device
               memory) or on the CPU (host memory)
    streams    the stream table of Handle.decode_streams / decode_ranges (STREAM_DESC_DTYPE array or rows)
    crops      B rows (stream index, first_sample), or an integer array [B, 2]
    dtype      torch.float32 (default; samples scaled to [-1, 1)) or torch.int32 (the decoded values)
    max_frames room for the index; by default a bound from the streams' byte lengths (a frame takes at least 10 bytes),
               which is safe and generous -- pass the real count where it is known

    Crop b is samples [first_sample, first_sample + T) of its stream in out[b]; where the stream ends (or stops
    decoding) before the crop does, the rest of every row is zero.  totals is an int64 tensor [B, 4] on the same device:
    samples written, stop reason, seek offset, seek position (flacenc_hip_decode_ranges).  The range table is built with
    array arithmetic; no Python work is done per crop on the data."""
    import torch

    dtype = torch.float32 if dtype is None else dtype
    if dtype not in (torch.float32, torch.int32):
        raise ValueError("decode_crops: dtype must be torch.float32 or torch.int32")
    if d_bytes.dtype != torch.uint8 or d_bytes.dim() != 1 or not d_bytes.is_contiguous():
        raise ValueError("decode_crops: d_bytes must be a contiguous 1-D uint8 tensor")
    table = _capi.stream_descs(streams)
    picks = np.asarray(crops, np.int64).reshape(-1, 2)
    B, T = len(picks), int(T)
    if T < 0 or (B and (picks.min() < 0 or picks[:, 0].max() >= len(table))):
        raise ValueError("decode_crops: a crop names no stream of the table, or a negative sample or length")
    counts = np.unique(table["channels"][picks[:, 0]]) if B else np.unique(table["channels"])
    if len(counts) > 1:
        raise ValueError("decode_crops: the crops' streams have %s channels; one tensor holds one channel count"
                         % sorted(int(c) for c in counts))
    C = int(counts[0]) if len(counts) else 1
    out = torch.empty((B, C, T), dtype=dtype, device=d_bytes.device)
    totals = torch.zeros((B, 4), dtype=torch.int64, device=d_bytes.device)
    if B == 0:
        return out, totals
    rtable = np.zeros(B, _capi.RANGE_DESC_DTYPE)
    rtable["first_sample"] = picks[:, 1]
    rtable["n_samples"] = T
    rtable["out_offset"] = np.arange(B, dtype=np.uint64) * np.uint64(C * T * 4)
    rtable["stream"] = picks[:, 0]
    if max_frames is None:
        frames = table["n_bytes"].astype(np.int64) // 10 + 1   # per stream, at the most
        max_frames = int(max(frames.sum(), np.minimum(frames[picks[:, 0]], max(T, 1)).sum()))
    fmt = _capi.SAMPLE_F32 if dtype == torch.float32 else _capi.SAMPLE_I32
    room = out if out.numel() else torch.empty(1, dtype=dtype, device=d_bytes.device)   # (T == 0: never a null pointer)
    if d_bytes.is_cuda:
        torch.cuda.synchronize(d_bytes.device)   # the call runs on the handle's own stream
        call, _ = handle.decode_ranges_planar_device(d_bytes.data_ptr(), d_bytes.numel(), table, rtable, max_frames,
                                                     room.data_ptr(), out.numel() * 4, fmt, totals.data_ptr())
    else:
        _, call, _ = handle.decode_ranges_planar(d_bytes.numpy(), table, rtable, max_frames, room.numpy(), fmt,
                                                 totals.numpy().view(np.uint64))
    if call[0] & _capi.INDEX_ERROR:
        raise RuntimeError("decode_crops: the streams or the crops hold more frames than max_frames = %d" % max_frames)
    return out, totals
