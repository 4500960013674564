"""What flacenc_hip_encode_streams must write, stated without the library's frame path: a stream is cut into blocks of
`block` samples and a last shorter one; frame i is the oracle's controller and bit writer (stream_seam_cases.Model: the
statement tests/test_gpu_stream_seams.py holds flacenc_hip_encode_pcm to) on block i with frame number i; the slot holds
the longest prefix of whole frames that fits its capacity."""
import functools

import numpy as np

import stream_seam_cases as seams
from flacenc_rs_amd import _capi
from oracle import oracle as orc


def configs(order=8, use_fixed=True, flags=0):
    """-> (the library's frame config, the model of its frames; None for flags nothing models)."""
    return seams.configs(order, use_fixed, flags)


_P, _E = _capi.FLAG_PRECISION_SEARCH, _capi.FLAG_RICE_ESCAPE
_SAME_FRAMES = _capi.FLAG_ALLOW_ORDER_32 | _capi.FLAG_FUSED_PACK   # admits an order; chooses a kernel


class RunModel:
    """The frames under FLACENC_HIP_FLAG_PRECISION_SEARCH (tests/precision_model.py, a fresh handle's floor),
    FLACENC_HIP_FLAG_RICE_ESCAPE (tests/escape_model.py) or both: the escape pass sits between the candidates and the
    decision, so with both the LPC candidate is the precision search's winner, chosen unescaped, and the pass runs on it
    and on the fixed candidate (tests/test_gpu_rice_escape.py states the records so).  A frame is stated once per
    (model, samples, number)."""

    def __init__(self, mine, ofc):
        self.key = (mine, bytes(ofc))

    def frame(self, x, bps, rate, number):
        return _run_frame(self.key, x.tobytes(), x.shape[0], x.shape[1], bps, rate, number)


def run_configs(order=8, use_fixed=True, flags=0):
    """-> (the library's frame config, the model of its frames) for every config of tests/encode_runs_cases.py: configs()
    where that has a model (FLACENC_HIP_FLAG_ALLOW_ORDER_32 admits an order, FLACENC_HIP_FLAG_FUSED_PACK chooses a kernel:
    neither changes a frame), a RunModel under the two flags above; None for anything else."""
    cfg = _capi.make_frame_config(_capi.make_config(lpc_order=order, flags=flags), use_fixed=use_fixed)
    mine = flags & (_P | _E)
    if not mine:
        return cfg, seams.configs(order, use_fixed, flags & ~_SAME_FRAMES)[1]
    if flags & ~(_P | _E | _SAME_FRAMES):
        return cfg, None
    import order_model
    return cfg, RunModel(mine, orc.make_frame_config(order_model.config(order), use_fixed=use_fixed))


def _precision_winner(x, w, qlpc):
    """precision_model.search's winner with the keys of oracle.estimated_qlpc that escape_model.subframe reads."""
    import precision_model
    best, _ = precision_model.search(x, w, qlpc)
    if best["status"] != 0:
        return {"status": int(best["status"])}
    qp = best["qp"]
    return dict(status=0, order=int(qp.order), precision=int(qp.precision), shift=int(qp.shift),
                coefs=[int(c) for c in qp.coefs[:int(qp.order)]], residual=best["residual"],
                rice_order=best["rice_order"], rice_params=best["rice_params"], code_bits=best["code_bits"],
                sum_quotients=best["sum_quotients"], subframe_bits=best["subframe_bits"])


@functools.lru_cache(4096)
def _run_frame(key, xbytes, C, n, bps, rate, number):
    mine, ofc_bytes = key
    x = np.frombuffer(xbytes, np.int32).reshape(C, n)
    ofc = orc.FrameConfig.from_buffer_copy(ofc_bytes)
    if mine == _P:
        import precision_model
        m = precision_model.Model()
        if C == 2:
            return m.stereo_frame_bytes(x[0], x[1], bps, ofc, number=number, sample_rate=rate)
        return m.channel_frame_bytes(list(x), bps, ofc, number=number, sample_rate=rate)
    import escape_model
    assert rate == 44100   # (flac_write, the writer of frames with escaped partitions: its default rate code)
    analyse = _precision_winner if mine & _P else None
    if C == 2:
        return escape_model.stereo_frame_bytes(x[0], x[1], bps, ofc, number=number, analyse=analyse)
    return escape_model.channel_frame_bytes(list(x), bps, ofc, number=number, analyse=analyse)


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
