"""flacenc_hip_encode_streams and flacenc_hip_encode_streams_planar on the GPU, on the corpus of
tests/encode_runs_cases.py: batches whose tail runs have the block sizes the kernel families are chosen by (fused 4096 /
4608, both sub-wave forms, big-block, generic), several frames per run, at the call's row stride and in the interior of
the class's buffers; and small batches across LPC orders, use_fixed and flags.  Every frame of every stream is held to
the model of tests/encode_streams_model.py -- the oracle's controller and bit writer, and the project's models of the
flags -- with the frame's own number; no comparison has the library itself as its truth.  tests/test_encode_runs_cpu.py
shows that the corpus reaches the runs it claims.  Every comparison is exact."""
import hashlib

import numpy as np
import pytest

import encode_runs_cases as runs
import encode_streams_cases as cases
import encode_streams_model as model
import planar_encode_model as pem
import stream_seam_cases as seams
from flacenc_rs_amd import _capi

pytestmark = pytest.mark.gpu
FILL = cases.FILL
LEN_SENTINEL, TOTAL_SENTINEL, CLIP_SENTINEL = 0xA5A5A5A5, 0x5A5A5A5A5A5A5A5A, 0x7777777777777777
I32, F32 = _capi.SAMPLE_I32, _capi.SAMPLE_F32


def run_host(h, lay, cfg, block):
    pcm = seams.buffer_of("pageable", lay.pcm.size)
    pcm[:] = lay.pcm
    out = np.full(lay.out_bytes, FILL, np.uint8)
    F = _capi.encode_streams_frames(lay.table, block)
    lens = np.full(F + 8, LEN_SENTINEL, np.uint32)
    totals = np.full((len(lay.table) + 2, 4), TOTAL_SENTINEL, np.uint64)
    _, _, call, _ = h.encode_streams(pcm, lay.table, cfg, block, out, frame_lengths=lens, totals=totals)
    assert np.array_equal(pcm, lay.pcm), "the input was written"
    return out, lens, totals, call


def run_device(h, lay, cfg, block):
    import torch
    F = _capi.encode_streams_frames(lay.table, block)
    d_pcm = torch.from_numpy(lay.pcm).cuda()
    d_out = torch.full((lay.out_bytes,), FILL, dtype=torch.uint8, device="cuda")
    d_lens = torch.from_numpy(np.full(F + 8, LEN_SENTINEL, np.uint32).view(np.int32)).cuda()
    d_totals = torch.from_numpy(np.full((len(lay.table) + 2, 4), TOTAL_SENTINEL, np.uint64).view(np.int64)).cuda()
    torch.cuda.synchronize()
    call, _ = h.encode_streams_device(d_pcm.data_ptr(), lay.pcm.size, lay.table, cfg, block, d_out.data_ptr(),
                                      lay.out_bytes, d_lens.data_ptr(), F, d_totals.data_ptr())
    assert np.array_equal(d_pcm.cpu().numpy(), lay.pcm), "the input was written"
    return d_out.cpu().numpy(), d_lens.cpu().numpy().view(np.uint32), d_totals.cpu().numpy().view(np.uint64), call


def run_planar(h, lay, fmt, cfg, block):
    ns = len(lay.table)
    F = _capi.encode_streams_frames(lay.table, block)
    out = np.full(lay.out_bytes, FILL, np.uint8)
    lens = np.full(F + 8, LEN_SENTINEL, np.uint32)
    totals = np.full((ns + 2, 4), TOTAL_SENTINEL, np.uint64)
    before = lay.samples.copy()
    _, _, call, dig, clip, _ = h.encode_streams_planar(lay.samples, fmt, lay.row_pitch, lay.table, cfg, block, out,
                                                       frame_lengths=lens, totals=totals, max_frames=F)
    assert np.array_equal(lay.samples.view(np.uint32), before.view(np.uint32)), "the input was written"
    return out, lens, totals, call, np.array(dig, copy=True), np.array(clip, copy=True)


def same(got, want, what):
    for a, b, name in zip(got[:3], want[:3], ("out", "frame_lengths", "totals")):
        assert a.shape == b.shape and np.array_equal(a, b), (what, name)
    assert list(got[3]) == list(want[3]), (what, "call_totals")


def check_against_the_model(streams, lay, want, block, out, lens, totals, call):
    """Slots, frame_lengths, totals and call_totals against the model's frames and the cut rule; FILL and the sentinels
    everywhere else."""
    ns = len(streams)
    F = sum(len(w) for w in want)
    assert (lens[F:] == LEN_SENTINEL).all() and (totals[ns:] == TOTAL_SENTINEL).all()
    assert (out[~cases.slot_map(lay.table, lay.out_bytes)] == FILL).all(), "bytes in no slot were written"
    first = frames = nbytes = 0
    for i, s in enumerate(streams):
        wlens = [len(f) for f in want[i]]
        off, cap = int(lay.table[i]["out_offset"]), int(lay.table[i]["out_capacity"])
        j, used = model.cut(wlens, cap)
        assert [int(v) for v in lens[first:first + len(wlens)]] == wlens, s.name
        assert [int(v) for v in totals[i]] == model.totals(wlens, cap, first), (s.name, totals[i])
        got = out[off:off + used].tobytes()
        if got != b"".join(want[i][:j]):
            at = 0
            for k, f in enumerate(want[i][:j]):
                assert got[at:at + len(f)] == f, "%s: frame %d of %d samples differs from the model" % (
                    s.name, k, min(block, s.x.shape[1] - k * block))
                at += len(f)
        assert (out[off + used:off + cap] == FILL).all(), s.name + ": bytes behind the stream's frames were written"
        first += len(wlens)
        frames += j
        nbytes += used
    assert first == F and list(call) == [frames, nbytes]


def planar_layouts(streams, table, fmt):
    """The same samples as rows of int32 or float32 elements (sample * 2^-(bits - 1): exact at these depths), at all four
    residues mod 16, tight and at an odd pitch; slots where the packed call has them."""
    rows = [s.x if fmt == I32 else pem.unscale(s.x, s.bps) for s in streams]
    if fmt == F32:
        for r, s in zip(rows, streams):
            assert np.array_equal(pem.q(r, s.bps)[0], s.x) and not pem.q(r, s.bps)[1].any()
    descs = [(int(d["out_offset"]), int(d["out_capacity"]), s.bps, s.width, s.rate) for d, s in zip(table, streams)]
    pitch = (max(s.x.shape[1] for s in streams) + 3) | 1
    for p in (0, pitch):
        lay = pem.layout(rows, descs, p, dtype=np.int32 if fmt == I32 else np.float32)
        assert {int(o) % 16 for o in lay.table["offset"]} == {0, 4, 8, 12}
        yield lay


@pytest.mark.parametrize("case", runs.CASES, ids=lambda c: c.name)
def test_a_batch_equals_the_model_on_every_frame(hooks_handle, case):
    h = hooks_handle
    block = case.block
    cfg, mod = model.run_configs(case.order, case.use_fixed, case.flags)
    assert mod is not None
    streams = runs.streams(case)
    want = [model.frames(mod, s, block) for s in streams]
    capacities = None
    if case.short:   # one slot a byte short of its last (tail) frame
        cut = next(i for i, s in enumerate(streams) if s.x.shape[1] == block + case.short)
        capacities = [None] * len(streams)
        capacities[cut] = sum(len(f) for f in want[cut]) - 1
    lay = cases.layout(streams, block, capacities=capacities, seed=len(case.name) + block)
    h.debug_set_encode_streams_chunk(case.chunk)
    try:
        got = run_host(h, lay, cfg, block)
        plan = h.debug_last_encode_streams_plan()
    finally:
        h.debug_set_encode_streams_chunk(0)
    check_against_the_model(streams, lay, want, block, *got)
    out, lens, totals, call = got
    if case.short:
        assert [int(v) for v in totals[cut]][0::3] == [len(want[cut]) - 1, _capi.ENCODE_NO_ROOM] and len(want[cut]) == 2
        assert sum(int(t[3]) != 0 for t in totals[:len(streams)]) == 1
    else:
        assert (totals[:len(streams), 3] == 0).all() and call[0] == sum(len(w) for w in want)

    # the plan is the brute-force one: the runs the CPU test reasons about are the runs that ran
    brute = runs.brute_plan(case)
    assert plan["classes"] == len(brute["classes"]) and plan["full_runs"] == brute["full_runs"]
    assert plan["tail_runs"] == brute["tail_runs"] and plan["calls"] == len(brute["runs"])
    assert plan["syncs"] == 2 and plan["transfers"] == 4

    if case.name in runs.DEVICE_TOO:
        same(run_device(h, lay, cfg, block), got, "device memory")
        dplan = h.debug_last_encode_streams_plan()
        assert dplan["syncs"] == 1 and dplan["transfers"] == 2 and dplan["calls"] == plan["calls"]

    if case.name in runs.PLANAR_TOO:
        digests = [hashlib.md5(cases.pack(s.x, s.width).tobytes()).digest() for s in streams]
        for fmt in (I32, F32):
            for play in planar_layouts(streams, lay.table, fmt):
                assert play.out_bytes == lay.out_bytes
                p = run_planar(h, play, fmt, cfg, block)
                same(p, got, ("planar", fmt, play.row_pitch))
                assert [d.tobytes() for d in p[4]] == digests, (fmt, play.row_pitch)
                assert not p[5].any(), "clip counts"
                pplan = h.debug_last_encode_streams_planar_plan()
                for k in ("classes", "full_runs", "tail_runs", "calls", "syncs", "transfers"):
                    assert pplan[k] == plan[k], k
