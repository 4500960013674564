"""The case table of the stream-contract suite (tests/test_gpu_stream_contract.py on the GPU, tests/stream_capture_child.py
for capture and replay, tests/test_stream_cases_cpu.py for completeness): one entry or more per `*_async` export of
include/flacenc_hip.h, each at the smallest shape that still reaches its kernel family.

A case names its export, builds its device arguments, and states what the call must write by running the BLOCKING form of
the same call (host pointers, the form the rest of the suite holds to the oracle) on a separate reference handle; exports
without a blocking form are stated by the host forms they compose (encode + pack) or by numpy / flacenc_rs_amd.shard.
Every case has two inputs of one shape: the real one, X, and a decoy, D, from another seed, chosen so that every frame's
outputs differ -- a call that read its inputs too early, or not on the caller's stream, writes D's results.  Cases that
produce frame bytes also parse the first and the last frame with tests/flac_parse.py and require X back.

All outputs are integers and bytes (the two floating-point outputs of qlpc_batch are compared as bit patterns): every
comparison is exact."""
import collections
import functools
import itertools
import os
import re

import numpy as np

import flac_parse
from flacenc_rs_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "flacenc_hip.h")
CANARY = 256          # bytes of 0xAB behind every output's extent
RATE = 44100
F = _capi

# inputs / expected: name -> array resp. canonical value; frames: one hashable per frame (what must differ between X and D)
Data = collections.namedtuple("Data", "inputs expected frames")


def header_async_exports():
    """Every export of include/flacenc_hip.h whose name ends in _async, from its declaration."""
    text = open(HEADER).read()
    decl = set(re.findall(r"^int (flacenc_hip_\w+_async)\(", text, re.M))
    assert decl == set(re.findall(r"\b(flacenc_hip_\w+_async)\(", text)), "an _async export that is not `int name(`"
    return sorted(decl)


class Case:
    """name, export, family (the kernels it reaches), out_bytes (name -> extent in bytes), make(ref, k) -> Data for seed
    number k (0: X, 1..: decoy candidates), inputs(k) -> those inputs alone where no handle is needed to build them (a
    process can then launch a case before any reference has run in it), call(h, I, O, stream) with I / O name -> device pointer, canon(raw) from the
    outputs' bytes to the form of Data.expected.  syncs: the header documents one stream synchronise (WASTED_BITS);
    capturable: the header makes the call capturable; comm: needs the handle's 1-rank communicator."""

    def __init__(self, name, export, family, out_bytes, make, call, canon, syncs=False, capturable=True, comm=False,
                 inputs=None):
        self.name, self.export, self.family = name, export, family
        self._out_bytes, self.make, self.call, self.canon = out_bytes, make, call, canon
        self.syncs, self.capturable, self.comm = syncs, capturable, comm
        self.inputs = inputs   # k -> the inputs of make(ref, k) without any call into a handle (None: they need one)
        self._data = None

    @property
    def out_bytes(self):
        """name -> extent in bytes (a callable where the library states a size: asked on first use)."""
        if callable(self._out_bytes):
            self._out_bytes = self._out_bytes()
        return self._out_bytes

    def data(self, ref):
        """(X, D): D is the first decoy candidate all of whose frames differ from X's."""
        if self._data is None:
            X = self.make(ref, 0)
            for k in range(1, 9):
                D = self.make(ref, k)
                assert {a: (v.shape, v.dtype) for a, v in D.inputs.items()} == \
                       {a: (v.shape, v.dtype) for a, v in X.inputs.items()}, self.name
                if all(a != b for a, b in itertools.zip_longest(X.frames, D.frames)):
                    break
            else:
                raise AssertionError("%s: no decoy whose every frame differs from X's" % self.name)
            assert X.expected != D.expected
            self._data = (X, D)
        return self._data

    def __repr__(self):
        return self.name


def same(got, want):
    """Exact equality of two canonical values (dicts of bytes / lists / ints)."""
    return got.keys() == want.keys() and all(got[k] == want[k] for k in want)


def first_difference(got, want):
    for k in want:
        if got.get(k) != want[k]:
            return k
    return None


# ---------------------------------------------------------------------------------------------------- material
def frame_cfg(order=8, flags=0, use_fixed=True, **kw):
    return F.make_frame_config(F.make_config(lpc_order=order, flags=flags, **kw), use_fixed=use_fixed)


def sigen(nf, ch, n, bps, seed):
    return F.sigen_frames(nf, ch, n, bps, 120.0 + seed % 5, 0.4, 0.3, seed=1000 + seed)


def marked(nf, n, seed):
    """The 24-bit material of test_marked_lists_across_mixed_pipelines: rows of +-(2^23 - 1), which the sub-wave kernel
    marks for the generic kernel's clean-up launch, with every third frame ordinary."""
    rng = np.random.default_rng(11 + seed)
    base = (rng.integers(0, 2, (8, n)) * 2 - 1).astype(np.int32) * (2 ** 23 - 1)
    x = np.ascontiguousarray(np.stack([base[rng.integers(0, 8, nf)], base[rng.integers(0, 8, nf)]], axis=1))
    x[1::3] = sigen(len(x[1::3]), 2, n, 24, seed)
    return x


def shifted(nf, n, bps, seed):
    """Odd frames with two, three, .. wasted bits in both channels."""
    x = sigen(nf, 2, n, bps, seed)
    for f in range(1, nf, 2):
        k = 2 + (f // 2) % 3
        x[f] = (x[f] >> k) << k
    return x


def changing(n_sb, ch, S, bps, seed):
    """Superblocks whose quarters are independent frames, so that the block-size search has something to split."""
    q = F.sigen_frames(n_sb * 4, ch, S // 4, bps, 150.0, 0.5, 0.2, seed=2000 + seed)
    return np.ascontiguousarray(q.reshape(n_sb, 4, ch, S // 4).transpose(0, 2, 1, 3).reshape(n_sb, ch, S))


MATERIAL = {"sigen": lambda nf, ch, n, bps, seed: sigen(nf, ch, n, bps, seed),
            "marked": lambda nf, ch, n, bps, seed: marked(nf, n, seed),
            "shifted": lambda nf, ch, n, bps, seed: shifted(nf, n, bps, seed)}


def u8(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


@functools.lru_cache(None)
def slot_bytes(ch, n, bps):
    """The packer's slot of one frame (the library's bound; asked when a case is first used, not when the table is built)."""
    lib = F.load()
    return int(lib.flacenc_hip_stereo_frame_bytes_bound(n, bps) if ch == 2 else lib.flacenc_hip_frame_bytes_bound(ch, n, bps))


def split_frames(out, lens, slot):
    return [bytes(out[f * slot:f * slot + int(lens[f])]) for f in range(len(lens))]


def anchor(frames, x, bps, first=0, step=1, wasted_ok=False):
    """The first and the last frame parse (tests/flac_parse.py: sync, both CRCs, every field) back to the real input."""
    for f in (0, len(frames) - 1):
        p = flac_parse.parse_frame(frames[f], stream_bps=bps, stream_rate=RATE, wasted_ok=wasted_ok)
        assert p["number"] == first + f * step and p["block_size"] == x.shape[2], (f, p["number"], p["block_size"])
        assert np.array_equal(p["channels"], x[f]), f


def pack_flags_off(cfg):
    c = F.FrameConfig.from_buffer_copy(cfg)
    c.qlpc.flags &= ~(F.FLAG_FUSED_PACK | F.FLAG_TWO_STAGE_PACK)
    return c


# ---------------------------------------------------------------------------------------------------- encode cases
ENC_S, ENC_PS = "flacenc_hip_encode_stereo_frames_async", "flacenc_hip_encode_pack_stereo_frames_async"
ENC_C, ENC_PC = "flacenc_hip_encode_frames_async", "flacenc_hip_encode_pack_frames_async"
QLPC, SQLPC, FIXED = "flacenc_hip_qlpc_batch_async", "flacenc_hip_stereo_qlpc_batch_async", \
    "flacenc_hip_fixed_lpc_batch_async"
RES, CRES, PAR = F.FRAME_RESULT_DTYPE.itemsize, F.CHANNEL_RESULT_DTYPE.itemsize, F.PARAMS_DTYPE.itemsize


def frames_case(name, export, family, n, bps, order, flags=0, nf=6, ch=2, material="sigen", use_fixed=True, qkw=None,
                want_fp=True, syncs=False, seed=0, first=3, step=2):
    """One launch of `nf` frames (rows for the candidate batches) of `n` samples through a frame- or candidate-level call."""
    cfg = frame_cfg(order, flags, use_fixed, **(qkw or {}))
    wasted = bool(flags & F.FLAG_WASTED_BITS)
    if export in (ENC_S, ENC_PS, SQLPC):
        assert ch == 2
    rows = nf * (4 if export == SQLPC else ch)
    slot = lambda: slot_bytes(ch, n, bps)  # noqa: E731
    rec = RES if ch == 2 else ch * CRES
    out_bytes = {ENC_S: lambda: {"results": nf * RES, "residual": nf * 2 * n * 4},
                 ENC_PS: lambda: {"results": nf * RES, "out": nf * slot(), "out_len": nf * 4},
                 ENC_C: lambda: {"results": nf * rec, "residual": nf * ch * n * 4},
                 ENC_PC: lambda: {"results": nf * rec, "out": nf * slot(), "out_len": nf * 4},
                 SQLPC: lambda: {"params": rows * PAR, "residual": rows * n * 4},
                 QLPC: lambda: dict({"params": rows * PAR, "residual": rows * n * 4},
                                    **({"autocorr": rows * 33 * 8, "lpc_coefs": rows * 32 * 8} if want_fp else {})),
                 FIXED: lambda: {"params": rows * PAR, "residual": rows * n * 4, "keys": rows * 8}}[export]

    def per_frame(*arrays):
        return [tuple(bytes(u8(a[f])) for a in arrays) for f in range(nf)]

    def inputs_of(k):
        x = MATERIAL[material](nf, ch, n, bps, seed * 16 + k)
        if export in (QLPC, FIXED):
            sub = np.ascontiguousarray(x.reshape(rows, n))
            return dict({"frames": sub}, **({"bps": np.full(rows, bps, np.uint8)} if export == QLPC else {}))
        return {"frames": x}

    def make(ref, k):
        inputs = inputs_of(k)
        x = inputs["frames"]
        if export == ENC_S:
            res, resid = ref.encode_stereo_frames(x, bps, cfg)
            return Data(inputs, {"results": res.tobytes(), "residual": resid.tobytes()}, per_frame(res, resid))
        if export == ENC_C:
            res, resid = ref.encode_frames(x, bps, cfg)
            return Data(inputs, {"results": res.tobytes(), "residual": resid.tobytes()}, per_frame(res, resid))
        if export in (ENC_PS, ENC_PC):
            plain = pack_flags_off(cfg)
            if ch == 2:
                res, resid = ref.encode_stereo_frames(x, bps, plain)
                frames = ref.pack_stereo_frames(x, res, resid, bps, RATE, first, step)
            else:
                res, resid = ref.encode_frames(x, bps, plain)
                frames = ref.pack_frames(x, res, resid, bps, RATE, first, step)
            if k == 0:
                anchor(frames, x, bps, first, step, wasted_ok=wasted)
            return Data(inputs, {"results": res.tobytes(), "frames": frames}, frames)
        if export == SQLPC:
            par, resid = ref.stereo_qlpc_batch(x, bps, cfg.qlpc)
            return Data(inputs, {"params": par.tobytes(), "residual": resid.tobytes()}, per_frame(par, resid))
        sub = x
        if export == QLPC:
            par, resid, R, A = ref.qlpc_batch(sub, inputs["bps"], cfg.qlpc, want_fp=want_fp)
            exp = {"params": par.tobytes(), "residual": resid.tobytes()}
            if want_fp:
                exp.update(autocorr=R.tobytes(), lpc_coefs=A.tobytes())
            return Data(inputs, exp, [(bytes(u8(par[f])), bytes(u8(resid[f]))) for f in range(rows)])
        par, resid, keys = ref.fixed_lpc_batch(sub, bps, cfg)
        return Data(inputs, {"params": par.tobytes(), "residual": resid.tobytes(), "keys": keys.tobytes()},
                    [(bytes(u8(par[f])), bytes(u8(resid[f]))) for f in range(rows)])

    def call(h, I, O, s):
        if export == ENC_S:
            h.encode_stereo_frames_device(cfg, I["frames"], nf, n, n, bps, O["results"], O["residual"], n, s)
        elif export == ENC_C:
            h.encode_frames_device(cfg, I["frames"], nf, ch, n, n, bps, O["results"], O["residual"], n, s)
        elif export == ENC_PS:
            h.encode_pack_stereo_frames_device(cfg, I["frames"], nf, n, n, bps, RATE, first, step, O["results"],
                                               O["out"], slot(), O["out_len"], s)
        elif export == ENC_PC:
            h.encode_pack_frames_device(cfg, I["frames"], nf, ch, n, n, bps, RATE, first, step, O["results"], O["out"],
                                        slot(), O["out_len"], s)
        elif export == SQLPC:
            h.stereo_qlpc_batch_device(cfg.qlpc, I["frames"], nf, n, n, bps, O["params"], O["residual"], n, s)
        elif export == QLPC:
            h.qlpc_batch_device(cfg.qlpc, I["frames"], rows, n, n, I["bps"], O["params"], O["residual"], n,
                                O.get("autocorr", 0), O.get("lpc_coefs", 0), stream=s)
        else:
            h.fixed_lpc_batch_device(cfg, I["frames"], rows, n, n, None, bps, F.LAYOUT_SUBFRAMES, O["params"],
                                     O["residual"], n, O["keys"], s)

    def canon(raw):
        if export in (ENC_PS, ENC_PC):
            return {"results": raw["results"].tobytes(),
                    "frames": split_frames(raw["out"], raw["out_len"].view(np.uint32), slot())}
        return {k: v.tobytes() for k, v in raw.items()}

    return Case(name, export, family, out_bytes, make, call, canon, syncs=syncs, capturable=not syncs, inputs=inputs_of)


# ---------------------------------------------------------------------------------------------------- records -> bytes
def records_case(name, export, family, n, bps, nf=6, ch=2, first=5, step=3):
    """The calls that start from decision records: Frame::write, the frames' lengths and the wire form."""
    cfg = frame_cfg(8)
    slot = lambda: slot_bytes(ch, n, bps)  # noqa: E731
    wb = lambda: int(F.load().flacenc_hip_frame_wire_bytes(n))  # noqa: E731
    out_bytes = {"pack": lambda: {"out": nf * slot(), "out_len": nf * 4}, "lengths": lambda: {"out_len": nf * 4},
                 "wire": lambda: {"wire": nf * wb(), "out_len": nf * 4}}[family]

    def make(ref, k):
        from flacenc_rs_amd import shard
        import torch
        x = sigen(nf, ch, n, bps, 300 + 16 * n % 97 + k)
        if ch == 2:
            res, resid = ref.encode_stereo_frames(x, bps, cfg)
            frames = ref.pack_stereo_frames(x, res, resid, bps, RATE, first, step)
        else:
            res, resid = ref.encode_frames(x, bps, cfg)
            frames = ref.pack_frames(x, res, resid, bps, RATE, first, step)
        lens = np.array([len(b) for b in frames], np.uint32)
        inputs = {"frames": x, "results": u8(res), "residual": resid}
        if family == "pack":
            if k == 0:
                anchor(frames, x, bps, first, step)
            return Data(inputs, {"frames": frames}, frames)
        if family == "lengths":
            return Data({"results": u8(res)}, {"out_len": lens.tobytes()}, lens.tolist())
        assert shard.wire_record_bytes(n) == wb()
        wire = shard.records_to_wire(torch.from_numpy(u8(res).reshape(nf, RES).copy()), n).numpy()
        return Data({"results": u8(res)}, {"wire": wire.tobytes(), "out_len": lens.tobytes()},
                    [bytes(wire[f]) for f in range(nf)])

    def call(h, I, O, s):
        if family == "pack" and ch == 2:
            h.pack_stereo_frames_device(I["frames"], nf, n, n, I["results"], I["residual"], n, bps, RATE, first, step,
                                        O["out"], slot(), O["out_len"], s)
        elif family == "pack":
            h.pack_frames_device(I["frames"], nf, ch, n, n, I["results"], I["residual"], n, bps, RATE, first, step,
                                 O["out"], slot(), O["out_len"], s)
        elif family == "lengths":
            h.stereo_frame_lengths_device(I["results"], nf, n, bps, RATE, first, step, O["out_len"], s)
        else:
            h.stereo_frame_wire_device(I["results"], nf, n, bps, RATE, first, step, O["wire"], wb(), O["out_len"], s)

    def canon(raw):
        if family == "pack":
            return {"frames": split_frames(raw["out"], raw["out_len"].view(np.uint32), slot())}
        return {k: v.tobytes() for k, v in raw.items()}

    return Case(name, export, family, out_bytes, make, call, canon)


# ---------------------------------------------------------------------------------------------------- the exchange
def offsets_case():
    nt, world, header = 9, 2, 42
    per = (nt + world - 1) // world

    def make(ref, k):
        lens = np.random.default_rng(70 + k).integers(14, 1 << 16, nt).astype(np.uint32) + np.arange(nt, dtype=np.uint32) * 7
        g = np.zeros((world, per), np.uint32)
        for r in range(world):
            g[r, :len(lens[r::world])] = lens[r::world]
        off = (np.cumsum(lens.astype(np.uint64)) - lens + header).astype(np.uint64)
        total = np.array([header + int(lens.sum())], np.uint64)
        return Data({"gathered": g}, {"lengths": lens.tobytes(), "offsets": off.tobytes(), "total": total.tobytes()},
                    lens.tolist())

    def call(h, I, O, s):
        h.stream_offsets_device(I["gathered"], nt, world, header, O["lengths"], O["offsets"], O["total"], s)

    return Case("stream_offsets world 2", "flacenc_hip_stream_offsets_async", "offsets",
                {"lengths": nt * 4, "offsets": nt * 8, "total": 8}, make, call, lambda raw: {k: v.tobytes() for k, v in raw.items()})


def place_case():
    lens = np.array([1, 15, 16, 17, 333, 4096, 7, 1001], np.uint32)   # any byte alignment
    src_off = (np.arange(len(lens), dtype=np.uint64) * 4099 + 3).astype(np.uint64)
    dst_off = (int(lens.sum()) - np.cumsum(lens.astype(np.uint64))).astype(np.uint64)   # frames land in reverse order
    total, src_bytes = int(lens.sum()), int(src_off[-1] + lens[-1]) + 5

    def make(ref, k):
        src = np.random.default_rng(90 + k).integers(0, 256, src_bytes).astype(np.uint8)
        frames = [bytes(src[int(o):int(o) + int(n)]) for o, n in zip(src_off, lens)]
        dst = bytearray(total)
        for fr, o in zip(frames, dst_off):
            dst[int(o):int(o) + len(fr)] = fr
        return Data({"src": src, "src_off": src_off, "lens": lens, "dst_off": dst_off}, {"dst": bytes(dst)}, frames)

    def call(h, I, O, s):
        h.place_frames_device(I["src"], I["src_off"], I["lens"], len(lens), O["dst"], I["dst_off"], s)

    return Case("place_frames", "flacenc_hip_place_frames_async", "place", {"dst": total}, make, call,
                lambda raw: {"dst": raw["dst"].tobytes()})


def allgather_case(records):
    n, rec = 7, 372

    def make(ref, k):
        local = np.random.default_rng(120 + k + 10 * records).integers(0, 256, (n, rec)).astype(np.uint8)
        return Data({"local": local}, {"gathered": local.tobytes()}, [bytes(r) for r in local])

    def call(h, I, O, s):
        if records:
            h.allgather_records_device(I["local"], n, n, rec, O["gathered"], s)
        else:
            h.allgather_device(I["local"], O["gathered"], n * rec, s)

    return Case("allgather_records 1 rank" if records else "allgather 1 rank",
                "flacenc_hip_allgather_records_async" if records else "flacenc_hip_allgather_async", "collective",
                {"gathered": n * rec}, make, call, lambda raw: {"gathered": raw["gathered"].tobytes()},
                capturable=False, comm=True)


# ---------------------------------------------------------------------------------------------------- input side
def fill_case():
    ch, bytes_per, n, nf = 2, 3, 576, 5
    total = nf * n - 123   # a short last block: zero-filled beyond it

    def make(ref, k):
        data = np.random.default_rng(150 + k).integers(0, 256, total * ch * bytes_per).astype(np.uint8)
        rows = ref.fill_le_bytes(data.tobytes(), ch, bytes_per, n)
        if k == 0:   # le_bytes_to_i32s + deinterleave, restated
            b = data.reshape(total, ch, 3).astype(np.int32)
            v = b[..., 0] | (b[..., 1] << 8) | (b[..., 2] << 16)
            v = (v ^ 0x800000) - 0x800000
            want = np.zeros((nf * n, ch), np.int32)
            want[:total] = v
            assert np.array_equal(rows, want.reshape(nf, n, ch).transpose(0, 2, 1))
        return Data({"bytes": data}, {"frames": rows.tobytes()}, [bytes(u8(rows[f])) for f in range(nf)])

    def call(h, I, O, s):
        h.fill_le_bytes_device(I["bytes"], total, ch, bytes_per, nf, n, O["frames"], n, s)

    return Case("fill_le_bytes 24-bit ragged", "flacenc_hip_fill_le_bytes_async", "fill", {"frames": nf * ch * n * 4},
                make, call, lambda raw: {"frames": raw["frames"].tobytes()})


# ---------------------------------------------------------------------------------------------------- the way back
DEC_FRAMES, DEC_MBS = 48, 192


def _decode_launch(k):
    """Launch k of the stereo frames of decode_cases.channel_cases(2) (blocks of 64..192 samples, the four assignments):
    (buffer padded to a common size, offsets, lengths, ground-truth rows)."""
    import decode_cases
    cases = decode_cases.channel_cases(2)
    buf, off, ln, entries = decode_cases.back_to_back(cases[k * DEC_FRAMES:(k + 1) * DEC_FRAMES])
    room = max(sum(len(c.data) for c in cases[j * DEC_FRAMES:(j + 1) * DEC_FRAMES]) for j in range(len(cases) // DEC_FRAMES))
    padded = np.zeros(room, np.uint8)
    padded[:len(buf)] = buf
    return padded, off, ln, decode_cases.expected_rows(entries, 2, DEC_MBS), len(buf)


def decode_case(verify):
    nf = DEC_FRAMES

    def inputs_of(k):
        buf, off, ln, _, _ = _decode_launch(k)
        return dict({"bytes": buf, "offsets": off, "lengths": ln}, **({"expected": _decode_launch(0)[3]} if verify else {}))

    def make(ref, k):
        buf, off, ln, truth, used = _decode_launch(k)
        rows, bs, num, st = ref.decode_frames(buf[:used], off, ln, 2, 16, DEC_MBS)
        assert np.array_equal(rows, truth) and not st.any()   # the blocking form against the frames' own samples
        if not verify:
            return Data({"bytes": buf, "offsets": off, "lengths": ln},
                        {"out": rows.tobytes(), "block_sizes": bs.tobytes(), "numbers": num.tobytes(), "status": st.tobytes()},
                        [bytes(u8(rows[f])) for f in range(nf)])
        x_rows = _decode_launch(0)[3]   # `expected` is always X's: the decoy's frames then MISMATCH, every one
        status = ref.verify_frames(buf[:used], off, ln, 2, 16, DEC_MBS, x_rows)
        want = np.where((rows == x_rows).reshape(nf, -1).all(axis=1), 0, F.DECODE_MISMATCH).astype(np.uint32)
        assert np.array_equal(status, want)
        return Data({"bytes": buf, "offsets": off, "lengths": ln, "expected": x_rows}, {"status": status.tobytes()},
                    status.tolist())

    def call(h, I, O, s):
        if verify:
            h.verify_frames_device(I["bytes"], I["offsets"], I["lengths"], nf, 2, 16, DEC_MBS, I["expected"], DEC_MBS,
                                   O["status"], s)
        else:
            h.decode_frames_device(I["bytes"], I["offsets"], I["lengths"], nf, 2, 16, DEC_MBS, O["out"], DEC_MBS,
                                   O["block_sizes"], O["numbers"], O["status"], s)

    out = {"status": nf * 4} if verify else {"out": nf * 2 * DEC_MBS * 4, "block_sizes": nf * 4, "numbers": nf * 8,
                                             "status": nf * 4}
    return Case("verify_frames stereo" if verify else "decode_frames stereo",
                "flacenc_hip_verify_frames_async" if verify else "flacenc_hip_decode_frames_async", "decode", out, make,
                call, lambda raw: {k: v.tobytes() for k, v in raw.items()}, inputs=inputs_of)


def index_case():
    """Mono 8-bit Verbatim frames of 20 distinct lengths; the decoy holds the same lengths in reverse, so the buffer is as
    long and every frame's (offset, length) differs."""
    sizes = [40 + 37 * i for i in range(20)]
    max_frames, n_bytes = 32, sum(sizes)

    def build(k):
        import decode_cases
        rng = np.random.default_rng(170 + k)
        order = sizes if k == 0 else sizes[::-1]
        frames = [decode_cases.mono8_frame_of_length(t, f, rng)[0] for f, t in enumerate(order)]
        return order, np.frombuffer(b"".join(frames), np.uint8).copy()

    def make(ref, k):
        order, data = build(k)
        lens = np.array(order, np.uint32)
        off = (np.cumsum(lens.astype(np.uint64)) - lens).astype(np.uint64)
        got = ref.index_frames(data, 1, 8, max_frames)
        assert got[2] and np.array_equal(got[0], off) and np.array_equal(got[1], lens)
        return Data({"bytes": data}, {"n": len(order), "offsets": off.tobytes(), "lengths": lens.tobytes()},
                    list(zip(off.tolist(), lens.tolist())))

    def call(h, I, O, s):
        h.index_frames_device(I["bytes"], n_bytes, 1, 8, max_frames, O["offsets"], O["lengths"], O["n_frames"], s)

    def canon(raw):
        n = int(raw["n_frames"].view(np.uint64)[0])
        assert n <= max_frames
        return {"n": n, "offsets": raw["offsets"].view(np.uint64)[:n].tobytes(),
                "lengths": raw["lengths"].view(np.uint32)[:n].tobytes()}

    return Case("index_frames mono", "flacenc_hip_index_frames_async", "index",
                {"offsets": max_frames * 8, "lengths": max_frames * 4, "n_frames": 8}, make, call, canon,
                inputs=lambda k: {"bytes": build(k)[1]})


# ---------------------------------------------------------------------------------------------------- block-size search
def variable_case():
    S, levels, bps, n_sb, first = 4096, 3, 16, 3, 1000
    total = n_sb * S - 777
    cfg = frame_cfg(8)
    cap = lambda: F.variable_bytes_bound(2, S, levels, bps, total)  # noqa: E731
    mf = lambda: F.variable_max_frames(S, levels, total)  # noqa: E731

    def inputs_of(k):
        x = changing(n_sb, 2, S, bps, k)
        x[-1, :, total % S:] = 0
        return {"frames": x}

    def make(ref, k):
        x = inputs_of(k)["frames"]
        v = ref.encode_variable(x, bps, cfg, levels, total_samples=total, sample_rate=RATE, first_sample_number=first)
        assert not v["overflow"]
        frames = [v["data"][int(o):int(o) + int(n)] for o, n in zip(v["offsets"], v["lengths"])]
        if k == 0:
            flat = x.transpose(1, 0, 2).reshape(2, -1)
            for fr in (frames[0], frames[-1]):
                p = flac_parse.parse_frame(fr, stream_bps=bps, stream_rate=RATE)
                at = p["number"] - first
                assert p["variable"] == 1 and np.array_equal(p["channels"], flat[:, at:at + p["block_size"]])
            assert sum(int(b) for b in v["block_sizes"]) == total and len(set(v["block_sizes"].tolist())) > 1
        exp = {"data": v["data"], "offsets": v["offsets"].tobytes(), "lengths": v["lengths"].tobytes(),
               "block_sizes": v["block_sizes"].tobytes(), "masks": v["split_masks"].tobytes(), "frames": v["frames"],
               "bytes": v["bytes"]}
        return Data({"frames": x}, exp, frames)

    def call(h, I, O, s):
        h.encode_variable_device(cfg, I["frames"], total, 2, S, levels, S, bps, RATE, first, O["out"], cap(), O["offsets"],
                                 O["lengths"], O["block_sizes"], mf(), O["masks"], O["totals"], s)

    def canon(raw):
        tot = raw["totals"].view(np.uint64)
        n, nbytes = int(tot[0]), int(tot[1])
        assert n <= mf() and nbytes <= cap()
        return {"data": raw["out"][:nbytes].tobytes(), "offsets": raw["offsets"].view(np.uint64)[:n].tobytes(),
                "lengths": raw["lengths"].view(np.uint32)[:n].tobytes(),
                "block_sizes": raw["block_sizes"].view(np.uint32)[:n].tobytes(), "masks": raw["masks"].tobytes(),
                "frames": n, "bytes": nbytes}

    return Case("encode_variable 4096 x 3 levels ragged", "flacenc_hip_encode_variable_async", "variable",
                lambda: {"out": cap(), "offsets": mf() * 8, "lengths": mf() * 4, "block_sizes": mf() * 4,
                         "masks": n_sb * 4, "totals": 16},
                make, call, canon, inputs=inputs_of)


# ---------------------------------------------------------------------------------------------------- the table
@functools.lru_cache(None)
def all_cases():
    S, W, O = F.FLAG_ORDER_SEARCH, F.FLAG_WINDOW_SEARCH, F.FLAG_WASTED_BITS
    return (
        # encode pipelines
        frames_case("fused 4096 order 8", ENC_S, "fused", 4096, 16, 8, seed=1),
        frames_case("4608 order 12", ENC_S, "fused", 4608, 16, 12, seed=2),
        frames_case("sub-wave 576 marking", ENC_PS, "subwave", 576, 24, 8, nf=8, material="marked", seed=3),
        frames_case("sub-wave 1152 marking", ENC_PS, "subwave", 1152, 24, 8, nf=8, material="marked", seed=4),
        frames_case("big-block 8192 24-bit order 24", ENC_S, "bigblock", 8192, 24, 24, nf=4, seed=5),
        frames_case("ragged 1000", ENC_S, "generic", 1000, 16, 8, seed=6),
        frames_case("1152 unflagged", ENC_S, "subwave", 1152, 16, 8, seed=7),
        frames_case("REFERENCE_SUM_ORDER stereo batch", SQLPC, "fused", 4096, 16, 8, F.FLAG_REFERENCE_SUM_ORDER, seed=8),
        frames_case("NIGHTLY_SUM_ORDER", ENC_S, "fused", 4096, 16, 8, F.FLAG_NIGHTLY_SUM_ORDER, seed=9),
        frames_case("FUSED_PACK", ENC_PS, "fusedpack", 4096, 16, 8, F.FLAG_FUSED_PACK, seed=10),
        frames_case("TWO_STAGE_PACK", ENC_PS, "fused", 4096, 16, 8, F.FLAG_TWO_STAGE_PACK, seed=11),
        frames_case("ORDER_SEARCH order 12", ENC_S, "search", 4096, 16, 12, S, nf=4, seed=12),
        frames_case("WINDOW_SEARCH", ENC_PS, "search", 4096, 16, 8, W, nf=4, seed=13),
        frames_case("ORDER_SEARCH + WINDOW_SEARCH batch", QLPC, "search", 4096, 16, 8, S | W, nf=4, seed=14),
        frames_case("WASTED_BITS", ENC_S, "wasted", 4096, 16, 8, O, material="shifted", syncs=True, seed=15),
        frames_case("direct_mse 2 IRLS steps", QLPC, "direct_mse", 4096, 16, 8, nf=4, want_fp=False,
                    qkw=dict(use_direct_mse=True, mae_optimization_steps=2), seed=16),
        frames_case("3 channels", ENC_C, "channels", 1152, 16, 8, ch=3, nf=5, seed=17),
        frames_case("3 channels encode + pack", ENC_PC, "channels", 1152, 16, 8, ch=3, nf=5, seed=18),
        frames_case("fixed_lpc batch", FIXED, "fixed", 4096, 16, 8, nf=4, seed=19),
        variable_case(),
        # records -> bytes and the exchange
        records_case("pack_stereo_frames", "flacenc_hip_pack_stereo_frames_async", "pack", 4096, 16),
        records_case("pack_frames 3 channels", "flacenc_hip_pack_frames_async", "pack", 1152, 16, ch=3, nf=5),
        records_case("stereo_frame_lengths", "flacenc_hip_stereo_frame_lengths_async", "lengths", 4096, 16),
        records_case("stereo_frame_wire", "flacenc_hip_stereo_frame_wire_async", "wire", 1152, 16),
        offsets_case(), place_case(), allgather_case(False), allgather_case(True),
        # input side and the way back
        fill_case(), decode_case(False), decode_case(True), index_case(),
    )


# two different sequences of six cases, all with handle-free inputs: what the two host threads of
# tests/stream_threads_child.py run, one sequence each
SEQUENCES = (("fused 4096 order 8", "sub-wave 576 marking", "WINDOW_SEARCH", "big-block 8192 24-bit order 24", "3 channels",
              "decode_frames stereo"),
             ("sub-wave 1152 marking", "ORDER_SEARCH order 12", "ragged 1000", "FUSED_PACK",
              "encode_variable 4096 x 3 levels ragged", "index_frames mono"))


def by_name(name):
    return {c.name: c for c in all_cases()}[name]


def names(pred=lambda c: True):
    return [c.name for c in all_cases() if pred(c)]


# ---------------------------------------------------------------------------------------------------- on the device
class Bound:
    """A case on the device: X and D uploaded once, static input buffers, outputs with a canary behind each extent."""

    def __init__(self, case, ref):
        """ref None: X alone, from case.inputs -- nothing of the library runs; resolve(ref) states the references later."""
        import torch
        self.case = case
        up = lambda inputs: {k: torch.from_numpy(u8(v).copy()).cuda() for k, v in inputs.items()}  # noqa: E731
        if ref is None:
            self.cold_inputs = case.inputs(0)
            self.dev, self.expected = {"X": up(self.cold_inputs)}, None
        else:
            self.X, self.D = case.data(ref)
            self.dev = {"X": up(self.X.inputs), "D": up(self.D.inputs)}
            self.expected = {"X": self.X.expected, "D": self.D.expected}
        self.inp = {k: torch.empty_like(t) for k, t in self.dev["X"].items()}
        self.out = {k: torch.empty(n + CANARY, dtype=torch.uint8, device="cuda") for k, n in case.out_bytes.items()}

    def resolve(self, ref):
        """After a cold start: the references, and that what was launched was X."""
        self.X, self.D = self.case.data(ref)
        assert self.X.inputs.keys() == self.cold_inputs.keys()
        assert all(np.array_equal(self.X.inputs[k], v) for k, v in self.cold_inputs.items()), self.case.name
        self.expected = {"X": self.X.expected, "D": self.D.expected}

    def load(self, which):
        """Enqueue, on the current stream, the copy of X or D into the static inputs."""
        for k, t in self.inp.items():
            t.copy_(self.dev[which][k], non_blocking=True)

    def arm(self):
        for t in self.out.values():
            t.fill_(0xAB)

    def launch(self, h, stream_ptr):
        self.case.call(h, {k: t.data_ptr() for k, t in self.inp.items()}, {k: t.data_ptr() for k, t in self.out.items()},
                       stream_ptr)

    def collect(self):
        """The outputs in canonical form; the canary behind every extent must be whole."""
        raw = {}
        for k, t in self.out.items():
            a = t.cpu().numpy()
            assert (a[-CANARY:] == 0xAB).all(), "%s: bytes behind the extent of %s were written" % (self.case.name, k)
            raw[k] = a[:-CANARY]
        return self.case.canon(raw)


def comm_handle(hooks=False):
    """A handle that owns a 1-rank RCCL communicator (what tests/test_gpu_exchange.py runs the collective calls on)."""
    h = F.Handle(0, hooks=hooks)
    h.comm_create(F.Handle.comm_unique_id(), 0, 1)
    return h
