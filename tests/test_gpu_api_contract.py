"""The argument contract of the C ABI's entry points: every blocking and async call with each class of bad input --
null pointers, n == 0, stride < block_size, channels 0 and 9, bits_per_sample outside the call's range, an unaligned
or short out_stride, a frame number that reaches 2^31, memory_kind 2, FLACENC_HIP_FLAG_WASTED_BITS on the candidate
batches -- must return the code written here.  The codes are what the library returned before the host layer was split
into units (recorded by running this table against that build); where include/flacenc_hip.h documents a code, it agrees.

Every case starts from a call that is valid -- real buffers of the right size, decision records and residual rows that a
real encode produced -- and changes one argument, so a case that a wrapper accepts simply runs on 2 frames of 256 samples.
The wrappers differ on purpose (flacenc_hip_encode_stereo_frames with n_frames == 0 on host memory returns
flacenc_hip_verify_config's code; the host-memory paths of the frame-level calls meet a short stride only in the 2-D
copy, which is the device error); the table pins each as it is.  A GPU test only because a handle needs a device."""
import ctypes as C

import numpy as np
import pytest

from flacenc_rs_amd import _capi

pytestmark = pytest.mark.gpu

OK, CONFIG, ARG, DEVICE, UNSUP = _capi.OK, _capi.ERR_BAD_CONFIG, _capi.ERR_BAD_ARGUMENT, _capi.ERR_DEVICE, _capi.ERR_UNSUPPORTED
N, B, CH, BPS, RATE = 2, 256, 3, 16, 44100  # frames, block size, channels of the Independent(n) calls


class Env:
    """One handle and the valid arguments of every call, in host memory and (torch tensors) in device memory."""

    def __init__(self):
        import torch

        self.handle = _capi.Handle(0)
        self.L, self.h = self.handle._lib, self.handle._h
        self.qcfg = _capi.make_config(lpc_order=8)
        self.wasted = _capi.make_config(lpc_order=8, flags=_capi.FLAG_WASTED_BITS)
        self.fcfg = _capi.make_frame_config(self.qcfg, use_fixed=True)
        self.fwasted = _capi.make_frame_config(self.wasted, use_fixed=True)
        stereo = _capi.sigen_frames(N, 2, B, BPS, 200.0, 0.4, 0.4, seed=0xC0417AC7)
        multi = _capi.sigen_frames(N, CH, B, BPS, 200.0, 0.4, 0.4, seed=0xC0417AC8)
        sres, sresid = self.handle.encode_stereo_frames(stereo, BPS, self.fcfg)
        cres, cresid = self.handle.encode_frames(multi, BPS, self.fcfg)
        packed = self.handle.pack_stereo_frames(stereo, sres, sresid, BPS, RATE)
        stream = np.frombuffer(b"".join(packed), dtype=np.uint8).copy()
        lengths = np.array([len(p) for p in packed], dtype=np.uint32)
        self.sbound = self.L.flacenc_hip_stereo_frame_bytes_bound(B, BPS)
        self.cbound = self.L.flacenc_hip_frame_bytes_bound(CH, B, BPS)
        self.wire = self.L.flacenc_hip_frame_wire_bytes(B)
        host = dict(
            stereo=stereo, multi=multi, sres=sres, sresid=sresid, cres=cres, cresid=cresid, stream=stream,
            lengths=lengths, offsets=(np.cumsum(lengths, dtype=np.uint64) - lengths).astype(np.uint64),
            pcm=np.ascontiguousarray(stereo.transpose(0, 2, 1), dtype="<i2").view(np.uint8).reshape(-1),
            bps=np.full(N * 4, BPS, dtype=np.uint8), params=np.zeros(N * 4 * 352, dtype=np.uint8),
            rows=np.zeros(N * 8 * B, dtype=np.int32), keys=np.zeros(N * 8, dtype=np.uint64),
            out=np.zeros(N * 8 * max(self.sbound, self.cbound), dtype=np.uint8), words=np.zeros(64, dtype=np.uint32),
            longs=np.zeros(64, dtype=np.uint64), more=np.zeros(64, dtype=np.uint64))
        host = {k: np.ascontiguousarray(v) for k, v in host.items()}
        self.keep = [host, {k: torch.from_numpy(v.view(np.uint8).reshape(-1).copy()).cuda() for k, v in host.items()}]
        self.mem = [{k: v.ctypes.data for k, v in host.items()}, {k: v.data_ptr() for k, v in self.keep[1].items()}]

    def close(self):
        self.handle.close()


@pytest.fixture(scope="module")
def env():
    e = Env()
    yield e
    e.close()


def _valid(e, name, kind):
    """The valid argument list of entry point `name` as an ordered dict; kind 0 / 1: the blocking call on host / device
    memory, 2: the async call (device memory, the handle's own stream is not reachable: the null stream)."""
    m = e.mem[1 if kind else 0]
    last = dict(stream=None) if kind == 2 else dict(memory_kind=kind)
    q, f = C.byref(e.qcfg), C.byref(e.fcfg)
    table = {
        "qlpc_batch": lambda: dict(h=e.h, cfg=q, samples=m["stereo"], n=N * 2, block_size=B, stride=B, bps=m["bps"],
                                   params=m["params"], residual=m["rows"], residual_stride=B, autocorr=None, lpc=None),
        "stereo_qlpc_batch": lambda: dict(h=e.h, cfg=q, samples=m["stereo"], n=N, block_size=B, stride=B, bits=BPS,
                                          params=m["params"], residual=m["rows"], residual_stride=B),
        "fixed_lpc_batch": lambda: dict(h=e.h, cfg=f, samples=m["stereo"], n=N * 2, block_size=B, stride=B, bps=None,
                                        bits=BPS, layout=0, params=m["params"], residual=m["rows"], residual_stride=B,
                                        keys=m["keys"]),
        "encode_frames": lambda: dict(h=e.h, cfg=f, samples=m["multi"], n=N, channels=CH, block_size=B, stride=B, bits=BPS,
                                      results=m["params"], residual=m["rows"], residual_stride=B),
        "encode_stereo_frames": lambda: dict(h=e.h, cfg=f, samples=m["stereo"], n=N, block_size=B, stride=B, bits=BPS,
                                             results=m["params"], residual=m["rows"], residual_stride=B),
        "pack_frames": lambda: dict(h=e.h, samples=m["multi"], n=N, channels=CH, block_size=B, stride=B, results=m["cres"],
                                    residual=m["cresid"], residual_stride=B, bits=BPS, rate=RATE, first=0, step=1,
                                    out=m["out"], out_stride=e.cbound, out_len=m["words"]),
        "pack_stereo_frames": lambda: dict(h=e.h, samples=m["stereo"], n=N, block_size=B, stride=B, results=m["sres"],
                                           residual=m["sresid"], residual_stride=B, bits=BPS, rate=RATE, first=0, step=1,
                                           out=m["out"], out_stride=e.sbound, out_len=m["words"]),
        "encode_pack_stereo_frames": lambda: dict(h=e.h, cfg=f, samples=m["stereo"], n=N, block_size=B, stride=B, bits=BPS,
                                                  rate=RATE, first=0, step=1, results=m["params"], out=m["out"],
                                                  out_stride=e.sbound, out_len=m["words"]),
        "encode_pack_frames": lambda: dict(h=e.h, cfg=f, samples=m["multi"], n=N, channels=CH, block_size=B, stride=B,
                                           bits=BPS, rate=RATE, first=0, step=1, results=m["params"], out=m["out"],
                                           out_stride=e.cbound, out_len=m["words"]),
        "stereo_frame_lengths": lambda: dict(h=e.h, results=m["sres"], n=N, block_size=B, bits=BPS, rate=RATE, first=0,
                                             step=1, out_len=m["words"]),
        "stereo_frame_wire": lambda: dict(h=e.h, results=m["sres"], n=N, block_size=B, bits=BPS, rate=RATE, first=0, step=1,
                                          out=m["out"], out_stride=e.wire, out_len=m["words"]),
        "fill_le_bytes": lambda: dict(h=e.h, samples=m["pcm"], total=N * B, channels=2, width=2, n=N, block_size=B,
                                      results=m["rows"], stride=B),
        "decode_frames": lambda: dict(h=e.h, samples=m["stream"], **({} if kind == 2 else dict(n_bytes=len(e.keep[0]["stream"]))),
                                      offsets=m["offsets"], lengths=m["lengths"], n=N, channels=2, bits=BPS, block_size=B,
                                      results=m["rows"], stride=B, block_sizes=m["words"], numbers=m["longs"],
                                      status=m["more"]),
        "verify_frames": lambda: dict(h=e.h, samples=m["stream"], offsets=m["offsets"], lengths=m["lengths"], n=N,
                                      channels=2, bits=BPS, block_size=B, results=m["stereo"], stride=B, status=m["more"]),
        "index_frames": lambda: dict(h=e.h, samples=m["stream"], n_bytes=len(e.keep[0]["stream"]), channels=2, bits=BPS, n=8,
                                     offsets=m["longs"], lengths=m["words"], results=m["more"]),
        "encode_variable": lambda: dict(h=e.h, cfg=f, samples=m["stereo"], total=N * B, channels=2, block_size=B, levels=1,
                                        stride=B, bits=BPS, rate=RATE, first=0, out=m["out"], capacity=N * e.sbound,
                                        offsets=m["longs"], lengths=m["words"], block_sizes=m["keys"], n=N, masks=m["bps"],
                                        results=m["more"]),
        "stream_offsets": lambda: dict(h=e.h, samples=m["lengths"], n=N, world=1, header=0, lengths=m["words"],
                                       offsets=m["longs"], results=m["more"]),
        "place_frames": lambda: dict(h=e.h, samples=m["stream"], offsets=m["offsets"], lengths=m["lengths"], n=N,
                                     out=m["out"], results=m["offsets"]),
    }
    if name == "encode_pcm":  # host memory only, no memory_kind
        mh = e.mem[0]
        return dict(h=e.h, cfg=f, samples=mh["pcm"], total=N * B, channels=2, width=2, bits=BPS, block_size=B, rate=RATE,
                    first=0, step=1, out=mh["out"], capacity=N * e.sbound, out_len=mh["words"],
                    results=C.cast(mh["more"], C.POINTER(C.c_uint64)))
    return {**table[name](), **last}


# name -> (kinds it exists in, {mutation: expected code or {kind: code}})
NULL_H, NULL_CFG, EMPTY = dict(h=None), dict(cfg=None), dict(n=0)
BATCH = {"h": ARG, "cfg": ARG, "n": OK, "samples": ARG, "params": ARG, "residual": ARG, "stride": ARG,
         "residual_stride": ARG, "memory_kind": ARG, "wasted": UNSUP}
FRAMES = {"h": ARG, "cfg": ARG, "n": OK, "samples": ARG, "results": ARG, "residual": ARG, "bits7": ARG, "bits25": ARG,
          "memory_kind": ARG}
PACK = {"h": ARG, "n": OK, "samples": ARG, "results": ARG, "residual": ARG, "out": ARG, "out_len": ARG, "stride": ARG,
        "residual_stride": ARG, "bits7": ARG, "bits25": ARG, "short_out": ARG, "frame_number": ARG, "memory_kind": ARG}
CONTRACT = {
    "qlpc_batch": ((0, 1, 2), BATCH),
    "stereo_qlpc_batch": ((0, 1, 2), {**BATCH, "bits7": ARG, "bits25": ARG}),
    "fixed_lpc_batch": ((0, 1, 2), {**BATCH, "bits7": ARG, "bits26": ARG, "layout": ARG}),
    "encode_frames": ((0, 1, 2), {**FRAMES, "stride": ARG, "residual_stride": ARG, "channels0": ARG, "channels9": ARG}),
    # host memory: no stride check in front of the 2-D copies (in: before anything ran; out: after the encode)
    "encode_stereo_frames": ((0, 1, 2), {**FRAMES, "stride": {0: DEVICE, 1: ARG, 2: ARG},
                                         "residual_stride": {0: DEVICE, 1: ARG, 2: ARG}}),
    # host memory: out_stride is only compared with the bound (the staging buffer has its own, aligned stride)
    "pack_frames": ((0, 1, 2), {**PACK, "odd_out": {0: OK, 1: ARG, 2: ARG}, "channels0": ARG, "channels9": ARG}),
    "pack_stereo_frames": ((0, 1, 2), {**PACK, "odd_out": {0: OK, 1: ARG, 2: ARG}}),
    "encode_pack_stereo_frames": ((2,), {"h": ARG, "cfg": ARG, "n": OK, "samples": ARG, "results": ARG, "out": ARG,
                                         "out_len": ARG, "stride": ARG, "bits7": ARG, "bits25": ARG, "short_out": ARG,
                                         "odd_out": ARG, "frame_number": ARG}),
    "encode_pack_frames": ((2,), {"h": ARG, "cfg": ARG, "n": OK, "samples": ARG, "results": ARG, "out": ARG, "out_len": ARG,
                                  "stride": ARG, "bits7": ARG, "bits25": ARG, "short_out": ARG, "odd_out": ARG,
                                  "frame_number": ARG, "channels0": ARG, "channels9": ARG}),
    "stereo_frame_lengths": ((2,), {"h": ARG, "n": OK, "results": ARG, "out_len": ARG, "frame_number": ARG}),
    "stereo_frame_wire": ((2,), {"h": ARG, "n": OK, "results": ARG, "out": ARG, "short_out": ARG, "frame_number": ARG}),
    "fill_le_bytes": ((0, 1, 2), {"h": ARG, "n": OK, "samples": ARG, "results": ARG, "stride": ARG, "channels0": ARG,
                                  "channels9": ARG, "memory_kind": ARG}),
    "decode_frames": ((0, 1, 2), {"h": ARG, "n": OK, "samples": ARG, "results": ARG, "block_sizes": ARG, "stride": ARG,
                                  "channels0": ARG, "channels9": ARG, "bits25": UNSUP, "memory_kind": ARG}),
    "verify_frames": ((2,), {"h": ARG, "n": OK, "samples": ARG, "results": ARG, "stride": ARG, "channels0": ARG,
                             "channels9": ARG, "bits25": UNSUP}),
    "index_frames": ((2,), {"h": ARG, "samples": ARG, "results": ARG, "channels0": ARG, "channels9": ARG, "bits25": UNSUP}),
    "encode_variable": ((0, 1, 2), {"h": ARG, "cfg": ARG, "total0": OK, "samples": ARG, "results": ARG, "stride": ARG,
                                    "channels0": ARG, "channels9": ARG, "bits7": ARG, "bits25": ARG, "memory_kind": ARG}),
    "encode_pcm": ((0,), {"h": ARG, "cfg": ARG, "total0": OK, "samples": ARG, "out": ARG, "out_len": ARG, "results": ARG,
                          "channels0": ARG, "channels9": ARG, "bits7": ARG, "bits25": ARG}),
    "stream_offsets": ((2,), {"h": ARG, "n": OK, "samples": ARG, "offsets": ARG, "results": ARG}),
    "place_frames": ((2,), {"h": ARG, "n": OK, "samples": ARG, "out": ARG, "results": ARG}),
}


def _mutate(e, args, mutation):
    if mutation in args and mutation not in ("n", "stride", "residual_stride", "memory_kind", "layout"):
        args[mutation] = None  # a null pointer
    elif mutation == "n":
        args["n"] = 0
    elif mutation == "total0":
        args["total"] = 0
    elif mutation in ("stride", "residual_stride"):
        args[mutation] = B - 1
    elif mutation in ("memory_kind", "layout"):
        args[mutation] = 2
    elif mutation == "wasted":
        args["cfg"] = C.byref(e.fwasted if isinstance(args["cfg"]._obj, _capi.FrameConfig) else e.wasted)
    elif mutation.startswith("bits"):
        args["bits"] = int(mutation[4:])
    elif mutation.startswith("channels"):
        args["channels"] = int(mutation[8:])
    elif mutation == "short_out":
        args["out_stride"] -= 16
    elif mutation == "odd_out":
        args["out_stride"] += 8
    elif mutation == "frame_number":  # the last of the N frames gets number 2^31
        args["first"] = (1 << 31) - N + 1
    else:
        raise KeyError(mutation)


CASES = [(name, kind, mutation, want[kind] if isinstance(want, dict) else want)
         for name, (kinds, table) in CONTRACT.items() for kind in kinds for mutation, want in table.items()
         if not (mutation == "memory_kind" and kind == 2)]


def run_case(e, name, kind, mutation):
    args = _valid(e, name, kind)
    _mutate(e, args, mutation)
    fn = getattr(e.L, "flacenc_hip_" + name + ("_async" if kind == 2 else ""))
    rc = fn(*args.values())
    e.L.flacenc_hip_synchronize(e.h)
    if kind == 2:
        import torch

        torch.cuda.synchronize()  # (the async cases run on the null stream)
    return rc


@pytest.mark.parametrize("name,kind,mutation,want", CASES, ids=["%s-%s-%s" % (c[0], ("host", "device", "async")[c[1]], c[2]) for c in CASES])
def test_return_code_of_bad_input(env, name, kind, mutation, want):
    got = run_case(env, name, kind, mutation)
    print("%s kind %d %s: returned %d, contract %d" % (name, kind, mutation, got, want))
    assert got == want


@pytest.mark.parametrize("name,kind", [(n, k) for n, (kinds, _) in CONTRACT.items() for k in kinds])
def test_the_unchanged_call_is_accepted(env, name, kind):
    """Each table row changes one argument of a call that is valid: the starting point itself returns OK."""
    args = _valid(env, name, kind)
    fn = getattr(env.L, "flacenc_hip_" + name + ("_async" if kind == 2 else ""))
    assert fn(*args.values()) == OK
    assert env.L.flacenc_hip_synchronize(env.h) == OK
    if kind == 2:
        import torch

        torch.cuda.synchronize()  # (the async calls run on the null stream)
