"""A batch of crops of FLAC streams as one torch tensor: flacenc_hip_decode_ranges_planar writes every crop's samples as
planar float32 (or int32) rows straight into a [B, C, T] tensor, so nothing touches the data between the decoder and the
model -- no widening, no transpose, no scaling, no padding, no per-crop copy.  encode_crops is the way back:
flacenc_hip_encode_streams_planar reads such a tensor as it lies and gives frames, digests and clip counts."""
import numpy as np

from . import _capi

__all__ = ["decode_crops", "encode_crops"]


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


def encode_crops(handle, x, lengths, bits_per_sample, sample_rate, cfg, block_size, bytes_per_sample=None, md5=True):
    """A [B, C, T] tensor, item b valid up to lengths[b] samples -> one FLAC frame sequence per item.

    handle            a _capi.Handle
    x                 contiguous torch.float32 (samples in [-1, 1), quantised as the inverse of decode_crops's scaling:
                      times 2^(bits_per_sample - 1), round to nearest even, clamp; NaN is 0) or torch.int32 (the samples)
                      tensor on the handle's GPU (the call runs in device memory) or on the CPU (host memory)
    lengths           B sample counts <= T, or None for T everywhere
    cfg               a _capi.FrameConfig (flags included)
    bytes_per_sample  the sample width of the packed PCM the digests are taken over; default ceil(bits_per_sample / 8),
                      which makes them the STREAMINFO digests
    md5               False: no digest is computed (and no packed image of the samples is ever built)

    -> dict(frames, items, frame_lengths, digests, clipped), every tensor on x's device: `frames` the uint8 buffer that
    holds every item's frames, items int64 [B, 3] = (offset into frames, bytes, frames) per item, frame_lengths int32
    over all items in order (item b's start at the sum of the items' frame counts before it), digests uint8 [B, 16] (None
    with md5=False), clipped int64 [B]: the elements of the item that clamped or were NaN (0 for int32).  Slots are sized
    from the frame-bytes bounds, so every frame of every item is there.  The tables are built with array arithmetic; no
    Python work is done per item on the data."""
    import torch

    if x.dtype not in (torch.float32, torch.int32) or x.dim() != 3 or not x.is_contiguous():
        raise ValueError("encode_crops: x must be a contiguous [B, C, T] float32 or int32 tensor")
    B, C, T = (int(v) for v in x.shape)
    n = np.full(B, T, np.int64) if lengths is None else np.asarray(lengths, np.int64).reshape(-1)
    if len(n) != B or (B and (n.min() < 0 or n.max() > T)) or not 1 <= C <= 8:
        raise ValueError("encode_crops: one length in 0..T per item, 1..8 channels")
    bps = (bits_per_sample + 7) // 8 if bytes_per_sample is None else int(bytes_per_sample)
    bound = handle.frame_bytes_bound(block_size, bits_per_sample) if C == 2 else \
        handle.frame_bytes_bound_channels(C, block_size, bits_per_sample)
    n_frames = -(-n // block_size)
    room = (n_frames * (bound + 8) + 15) // 16 * 16       # (+ 8: a frame number takes up to 5 bytes more than number 0)
    table = np.zeros(B, _capi.PCM_STREAM_DESC_DTYPE)
    table["offset"] = np.arange(B, dtype=np.uint64) * np.uint64(C * T * 4)
    table["total_samples"] = n
    table["out_offset"] = np.cumsum(room) - room
    table["out_capacity"] = room
    table["channels"], table["bits_per_sample"], table["bytes_per_sample"], table["sample_rate"] = C, bits_per_sample, bps, sample_rate
    total_frames, out_bytes = int(n_frames.sum()), int(room.sum())
    dev = x.device
    frames = torch.zeros(max(out_bytes, 1), dtype=torch.uint8, device=dev)
    flen = torch.zeros(max(total_frames, 1), dtype=torch.int32, device=dev)
    totals = torch.zeros((max(B, 1), 4), dtype=torch.int64, device=dev)
    digests = torch.zeros((max(B, 1), 16), dtype=torch.uint8, device=dev) if md5 else None
    clipped = torch.zeros(max(B, 1), dtype=torch.int64, device=dev)
    fmt = _capi.SAMPLE_F32 if x.dtype == torch.float32 else _capi.SAMPLE_I32
    if B:
        src = x if x.numel() else torch.zeros(1, dtype=x.dtype, device=dev)   # (T == 0: never a null pointer)
        if x.is_cuda:
            torch.cuda.synchronize(dev)   # the call runs on the handle's own stream
            handle.encode_streams_planar_device(src.data_ptr(), x.numel() * 4, fmt, T, table, cfg, block_size,
                                                frames.data_ptr(), out_bytes, flen.data_ptr(), max(total_frames, 1),
                                                totals.data_ptr(), digests.data_ptr() if md5 else 0, clipped.data_ptr())
        else:
            _, _, _, dig, clip, _ = handle.encode_streams_planar(
                src.numpy(), fmt, T, table, cfg, block_size, frames.numpy()[:out_bytes],
                flen.numpy().view(np.uint32), totals.numpy().view(np.uint64), digests=md5, samples_bytes=x.numel() * 4)
            if md5:
                digests.numpy()[:B] = dig
            clipped.numpy()[:B] = clip.astype(np.int64)
    items = torch.stack([torch.from_numpy(table["out_offset"].astype(np.int64)).to(dev), totals[:B, 1], totals[:B, 0]], 1) \
        if B else torch.zeros((0, 3), dtype=torch.int64, device=dev)
    return dict(frames=frames[:out_bytes], items=items, frame_lengths=flen[:total_frames],
                digests=digests[:B] if md5 else None, clipped=clipped[:B])
