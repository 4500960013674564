"""What flacenc_hip_encode_streams must write, stated without the library's frame path: a stream is cut into blocks of
`block` samples and a last shorter one; frame i is the oracle's controller and bit writer (stream_seam_cases.Model: the
statement tests/test_gpu_stream_seams.py holds flacenc_hip_encode_pcm to) on block i with frame number i; the slot holds
the longest prefix of whole frames that fits its capacity."""
import numpy as np

import stream_seam_cases as seams
from flacenc_rs_amd import _capi


def configs(order=8, use_fixed=True, flags=0):
    """-> (the library's frame config, the model of its frames; None for flags nothing models)."""
    return seams.configs(order, use_fixed, flags)


def frames(model, s, block):
    """The frames of stream `s` (encode_streams_cases.Stream), each as bytes."""
    total = s.x.shape[1]
    out = []
    for i, at in enumerate(range(0, total, block)):
        x = np.ascontiguousarray(s.x[:, at:at + block], np.int32)
        out.append(model.frame(x, s.bps, s.rate, i))
    return out


def cut(lengths, capacity):
    """How many whole frames of `lengths` fit `capacity` bytes back to back: the longest prefix."""
    used = j = 0
    for n in lengths:
        if used + int(n) > capacity:
            break
        used += int(n)
        j += 1
    return j, used


def totals(lengths, capacity, first):
    """totals[s] of the call for a stream with these frame lengths in a slot of `capacity` bytes, whose first entry in
    frame_lengths is `first`."""
    j, used = cut(lengths, capacity)
    return [j, used, first, _capi.ENCODE_NO_ROOM if j < len(lengths) else 0]


def coded_number_bytes(v):
    return 1 if v < 1 << 7 else 2 if v < 1 << 11 else 3 if v < 1 << 16 else 4 if v < 1 << 21 else 5 if v < 1 << 26 else 6
