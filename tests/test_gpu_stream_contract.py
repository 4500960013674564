"""The four promises include/flacenc_hip.h makes about the `*_async` exports, held on a stream that is not the NULL stream
(DESIGN.md section 4.12).  The cases are those of tests/stream_cases.py: every async export, each reference the blocking
host-pointer form of the same call on a separate handle, every comparison exact.

  1. stream-ordered: behind a sleep kernel on a stream s the test queues the copy of the real input X over a decoy D and
     then the library call.  The call returns while s is still inside the sleep (no synchronise; WASTED_BITS, whose one
     synchronise the header documents, must instead return only once s has drained), the outputs after s.synchronize() --
     no device-wide synchronise -- are X's, and the canary behind every output is whole.  A launch, memset or copy on
     another stream would have run during the sleep, on D.  The CONTROL of every case shows that the method sees this:
     the same sequence with the library call placed on a second stream by the test itself must give D's outputs.
  2. one handle, one stream at a time, or ordered by events: a marking sub-wave call on s1, an event, the fused kernel
     and the sub-wave call again on s2; two handles on two streams from two host threads in a fresh process
     (tests/stream_threads_child.py: every kernel's first use in the process is concurrent), then interleaved from one.
  3. the host may run ahead: 28 launches of the certified shape queued behind one sleep with the order mode switched
     on -- hard, easy, hard material -- against the same launches with a synchronise between them.
  4. capturable: tests/stream_capture_child.py captures every capturable case into a graph and replays it on X, D, X.

The sleep is ten times the event-timed duration of the case's warm blocking form on the reference handle (which stages
through host memory, so it bounds the device form from above); the control failing means that margin is too small.
"Still inside the sleep" is asked of an event recorded on s behind the copy of X, not of s.query(): a call that
synchronised half-way and then enqueued more would leave s busy all the same.
A floor of 5 ms covers the test's own enqueueing where the call is a few microseconds long.
Measured on an MI355X: _sleep runs 2.39e6 cycles per ms; blocking form -> sleep in ms, per case (* no blocking form: the
device form on the NULL stream and a synchronise were timed):
    fused 4096 order 8                          0.138 ->  5.00
    4608 order 12                               0.136 ->  5.00
    sub-wave 576 marking                        0.775 ->  7.75
    sub-wave 1152 marking                       0.832 ->  8.32
    big-block 8192 24-bit order 24              0.268 ->  5.00
    ragged 1000                                 0.173 ->  5.00
    1152 unflagged                              0.134 ->  5.00
    REFERENCE_SUM_ORDER stereo batch            0.156 ->  5.00
    NIGHTLY_SUM_ORDER                           0.290 ->  5.00
    FUSED_PACK                                  0.233 ->  5.00
    TWO_STAGE_PACK                              0.234 ->  5.00
    ORDER_SEARCH order 12                       0.605 ->  6.05
    WINDOW_SEARCH                               0.668 ->  6.68
    ORDER_SEARCH + WINDOW_SEARCH batch          1.989 -> 19.89
    WASTED_BITS                                 0.243 ->  5.00
    direct_mse 2 IRLS steps                     0.545 ->  5.45
    3 channels                                  0.146 ->  5.00
    3 channels encode + pack                    0.249 ->  5.00
    fixed_lpc batch                             0.126 ->  5.00
    encode_variable 4096 x 3 levels ragged      0.648 ->  6.48
    pack_stereo_frames                          0.255 ->  5.00
    pack_frames 3 channels                      0.245 ->  5.00
    stereo_frame_lengths                        0.228 ->  5.00
    stereo_frame_wire                           0.250 ->  5.00
    stream_offsets world 2 *                    0.018 ->  5.00
    place_frames *                              0.019 ->  5.00
    allgather 1 rank *                          0.011 ->  5.00
    allgather_records 1 rank *                  0.014 ->  5.00
    fill_le_bytes 24-bit ragged                 0.045 ->  5.00
    decode_frames stereo                        0.944 ->  9.44
    verify_frames stereo                        1.850 -> 18.50
    index_frames mono                           0.216 ->  5.00
All 32 controls pass with these; the file (97 tests) runs in 11.18 s, its longest test (test_call_is_ordered_on_the_callers_stream[decode_frames) in 0.39 s."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import stream_cases as sc
from flacenc_rs_amd import _capi

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ALL = sc.names()
SLEEP_FACTOR = 10
# The margin of ten covers the host time the library spends enqueueing, which scales with the call; the host time of the
# test's own enqueueing (the copies of X, the stream switch) does not shrink with the kernel, so calls of a few
# microseconds (lengths, offsets, place) get this much at least.
SLEEP_FLOOR_MS = 5.0


def sleep_ms(blocking_ms):
    return max(SLEEP_FACTOR * blocking_ms, SLEEP_FLOOR_MS)


@pytest.fixture(scope="module")
def ref():
    """The reference handle: only blocking forms run on it (and, for the few exports that have none, the device form on
    the NULL stream with a synchronise behind it, to be timed)."""
    h = sc.comm_handle()
    yield h
    h.close()


@pytest.fixture(scope="module")
def dut():
    """The handle under test: one for every case, so that each call meets the scratch the others left; it owns the 1-rank
    communicator of the two collective calls."""
    h = sc.comm_handle()
    yield h
    h.close()


@pytest.fixture(scope="module")
def cycles_per_ms():
    """torch.cuda._sleep spins for a number of device clock cycles: two events around one calibrate it."""
    import torch
    torch.cuda._sleep(1000)
    torch.cuda.synchronize()
    cycles = 50_000_000
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    torch.cuda._sleep(cycles)
    e1.record()
    e1.synchronize()
    rate = cycles / e0.elapsed_time(e1)
    print("stream contract: _sleep runs %.0f cycles per ms" % rate)
    assert rate > 1000
    return rate


class Timed:
    """The reference handle with every call timed between two events (the blocking forms return when their results are
    on the host, so this is their whole duration)."""

    def __init__(self, h):
        self.h, self.ms = h, 0.0

    def __getattr__(self, name):
        import torch
        f = getattr(self.h, name)

        def call(*a, **k):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = f(*a, **k)
            e1.record()
            e1.synchronize()
            self.ms += e0.elapsed_time(e1)
            return out
        return call


_bound, _sleep = {}, {}


def bound(name, ref):
    if name not in _bound:
        _bound[name] = sc.Bound(sc.by_name(name), ref)
    return _bound[name]


def sleep_cycles(name, ref, cycles_per_ms):
    """Ten times the warm blocking form's duration, in _sleep cycles."""
    if name not in _sleep:
        bound(name, ref)   # (the first run of the blocking form: now it is warm)
        t = Timed(ref)
        sc.by_name(name).make(t, 0)
        if t.ms == 0:   # no blocking form (offsets, place, the collective): the device form and a synchronise
            import torch
            b = bound(name, ref)
            warm(b, ref)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            b.launch(ref, torch.cuda.current_stream().cuda_stream)
            e1.record()
            e1.synchronize()
            t.ms = e0.elapsed_time(e1)
        assert t.ms > 0
        _sleep[name] = t.ms
        print("stream contract: %-40s blocking form %8.3f ms, sleep %8.2f ms" % (name, t.ms, sleep_ms(t.ms)))
    return int(sleep_ms(_sleep[name]) * cycles_per_ms)


def warm(b, h):
    import torch
    b.load("D")
    b.arm()
    b.launch(h, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()


def behind_sleep(b, h, cycles, call_on_second_stream=False):
    """D in the inputs, the canary in the outputs; on s: sleep, copy X in, the call (or the call on a stream of its own).
    -> (what was queued on s before the call was still pending when the call returned, the outputs after the streams --
    and nothing else -- were synchronised)."""
    import torch
    s, s2, queued = torch.cuda.Stream(), torch.cuda.Stream(), torch.cuda.Event()
    b.load("D")
    b.arm()
    torch.cuda.current_stream().synchronize()
    with torch.cuda.stream(s):
        torch.cuda._sleep(cycles)
        b.load("X")
        queued.record(s)
    b.launch(h, (s2 if call_on_second_stream else s).cuda_stream)
    busy = not queued.query()
    s2.synchronize()
    s.synchronize()
    return busy, b.collect()


@pytest.mark.parametrize("name", ALL)
def test_call_is_ordered_on_the_callers_stream(name, ref, dut, cycles_per_ms):
    """WASTED_BITS "SYNCHRONISES the stream once ... cannot be captured into a graph": it is not captured, and the other
    half is asked here -- behind a sleep the call returns only after the stream has drained of what it held.  (The
    synchronise sits between the scan and the pipeline, which the call enqueues after it -- "the *_async forms block the
    host for that long" -- so the stream is busy again on return: the event behind the copy of X is what is asked.)"""
    b = bound(name, ref)
    cycles = sleep_cycles(name, ref, cycles_per_ms)
    warm(b, dut)
    busy, got = behind_sleep(b, dut, cycles)
    if b.case.syncs:
        assert not busy, "the header's one synchronise: the call returns after what the stream held before it has run"
    else:
        assert busy, "the call returned after the sleep on its stream had ended: it synchronised, or the sleep is too short"
    assert sc.same(got, b.expected["X"]), "differs from the blocking form on X in %s%s" % (
        sc.first_difference(got, b.expected["X"]), " (and equals D's: read before its turn on the stream)"
        if sc.same(got, b.expected["D"]) else "")


@pytest.mark.parametrize("name", ALL)
def test_control_call_on_another_stream_sees_the_decoy(name, ref, dut, cycles_per_ms):
    """The method's own check: with the call on a second stream the copy of X is still behind the sleep, so the outputs
    must be D's.  Every buffer is valid memory throughout."""
    b = bound(name, ref)
    cycles = sleep_cycles(name, ref, cycles_per_ms)
    warm(b, dut)
    busy, got = behind_sleep(b, dut, cycles, call_on_second_stream=True)
    assert busy or b.case.syncs
    assert sc.same(got, b.expected["D"]), "the sleep did not cover the call: margin too small (differs in %s)" % \
        sc.first_difference(got, b.expected["D"])


# ---- one handle across two streams, two handles at once ----------------------------------------------------------------
def fresh(name, ref, which="X"):
    """A case's buffers of their own, the input in place and the canary set."""
    b = sc.Bound(sc.by_name(name), ref)
    b.load(which)
    b.arm()
    return b


def test_one_handle_handed_from_stream_to_stream_by_an_event(ref, dut, cycles_per_ms):
    """"Ordered on one stream (or by events)": the marking sub-wave call on s1 behind a sleep, an event, then on s2 the
    fused 4096 kernel and the sub-wave call again -- scratch reuse and both parities of the marked-subframe counters,
    with no host synchronise between the three."""
    import torch
    A, B = "sub-wave 576 marking", "fused 4096 order 8"
    a1, bb, a2 = fresh(A, ref, "D"), fresh(B, ref), fresh(A, ref)
    for x in (a1, bb):
        warm(x, dut)
    a1.load("D")
    bb.load("X")
    for x in (a1, bb, a2):
        x.arm()
    cycles = sleep_cycles(A, ref, cycles_per_ms)
    torch.cuda.current_stream().synchronize()
    s1, s2, ev, slept = torch.cuda.Stream(), torch.cuda.Stream(), torch.cuda.Event(), torch.cuda.Event()
    with torch.cuda.stream(s1):
        torch.cuda._sleep(cycles)
        slept.record(s1)
        a1.load("X")
    a1.launch(dut, s1.cuda_stream)
    ev.record(s1)
    s2.wait_event(ev)
    bb.launch(dut, s2.cuda_stream)
    a2.launch(dut, s2.cuda_stream)
    assert not slept.query(), "the sleep was to be running still when the third call had been queued"
    s2.synchronize()
    s1.synchronize()
    for x in (a1, bb, a2):
        got = x.collect()
        assert sc.same(got, x.expected["X"]), (x.case.name, sc.first_difference(got, x.expected["X"]))


@pytest.fixture(scope="module")
def threads_report(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("threads") / "report.json")
    run = subprocess.run([sys.executable, os.path.join(HERE, "stream_threads_child.py"), path], capture_output=True,
                         text=True, timeout=300)
    report = json.load(open(path)) if os.path.exists(path) else {"error": "no report", "threads": {}, "interleaved": {}}
    report["tail"] = (run.stdout + run.stderr)[-1500:]
    report["returncode"] = run.returncode
    return report


def test_two_handles_on_two_streams_from_two_threads(threads_report):
    """Two fresh handles, each with its own stream and host thread, each running its own six cases
    (stream_cases.SEQUENCES) with no synchronise between them, in a child process in which no handle existed and no
    kernel of the library had been launched before the threads started: the process-wide first use of every kernel
    (lds_opt_in.h's bookkeeping, shared by all handles) and every handle's first use of its scratch, window cache and
    marked-subframe counters happen while the other thread is inside the library.  The blocking references run after the
    join.  Then both sequences interleaved from one thread.  tests/stream_threads_child.py."""
    r = threads_report
    assert r["error"] is None and r["returncode"] == 0, (r["error"], r["returncode"], r["tail"])
    names = [n for seq in sc.SEQUENCES for n in seq]
    assert len(names) == 12 and len(set(names)) == 12
    for phase in ("threads", "interleaved"):
        assert sorted(r[phase]) == sorted(names), (phase, "cases that did not run", sorted(set(names) - set(r[phase])))
        wrong = {n: d for n, d in r[phase].items() if d is not None}
        assert not wrong, (phase, "differ from the blocking forms in", wrong)


# ---- the host running ahead of the device ------------------------------------------------------------------------------
def test_order_mode_decides_the_same_with_the_host_far_ahead(ref, cycles_per_ms):
    """launch_adaptive (api_candidates.cpp) picks the certified or the two-pass form from verdicts the device writes late
    into a pinned word; "the host may run many launches ahead of the device".  28 launches of 160 frames (640 subframes)
    at order 8 -- 12 of near-pure tones, 4 of noisy sines, 12 of tones again -- are queued behind one sleep, each into its
    own buffers: nothing has run when the last is queued, so no verdict can have been seen and the state is still "easy".
    Then the 12 hard launches with a synchronise between them, where the state machine does see its verdicts (and takes the
    two-pass form: span 8).  A choice of speed, never of result: every launch equals the blocking reference."""
    import torch

    import test_gpu_certified_order as corp
    n, nf, order, bps = 4096, 160, 8, 16
    pick = np.random.default_rng(order).integers(0, 24, size=(nf, 2))
    hl, hr = corp.near_pure_sines(24, n, seed0=700 + order), corp.near_pure_sines(24, n, seed0=800 + order)
    el, er = corp.noisy_sines(24, n, seed0=900), corp.noisy_sines(24, n, seed0=950)
    hard = np.ascontiguousarray(np.stack([hl[pick[:, 0]], hr[pick[:, 1]]], axis=1))
    easy = np.ascontiguousarray(np.stack([el[pick[:, 0]], er[pick[:, 1]]], axis=1))
    fc = sc.frame_cfg(order)
    ref.encode_stereo_frames(hard, bps, fc)   # warm
    t = Timed(ref)
    want = {"hard": t.encode_stereo_frames(hard, bps, fc), "easy": ref.encode_stereo_frames(easy, bps, fc)}
    assert want["hard"][0].tobytes() != want["easy"][0].tobytes()
    dev = {"hard": torch.from_numpy(hard).cuda(), "easy": torch.from_numpy(easy).cuda()}
    plan = ["hard"] * 12 + ["easy"] * 4 + ["hard"] * 12
    outs = [(torch.full((nf * sc.RES,), 0xAB, dtype=torch.uint8, device="cuda"),
             torch.full((nf * 2 * n,), -1, dtype=torch.int32, device="cuda")) for _ in plan]

    def launch(h, kind, out, stream):
        h.encode_stereo_frames_device(fc, dev[kind].data_ptr(), nf, n, n, bps, out[0].data_ptr(), out[1].data_ptr(), n,
                                      stream)

    def check(kind, out, label):
        res, resid = want[kind]
        assert out[0].cpu().numpy().tobytes() == res.tobytes(), (label, "records")
        assert np.array_equal(out[1].cpu().numpy().reshape(resid.shape), resid), (label, "rows")

    with _capi.Handle(0, hooks=True) as h:
        warm_out = (torch.empty_like(outs[0][0]), torch.empty_like(outs[0][1]))
        launch(h, "easy", warm_out, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        h.debug_set_adaptive_order(True)   # (also resets the state the warm-up left)
        s, slept = torch.cuda.Stream(), torch.cuda.Event()
        with torch.cuda.stream(s):
            torch.cuda._sleep(int(sleep_ms(t.ms) * cycles_per_ms))
            slept.record(s)
        for kind, out in zip(plan, outs):
            launch(h, kind, out, s.cuda_stream)
        assert not slept.query(), "the sleep was to be running still when the 28th launch had been queued"
        assert h.debug_adaptive_state() == (0, 0), "a verdict was concluded from launches that have not run"
        s.synchronize()
        for i, (kind, out) in enumerate(zip(plan, outs)):
            check(kind, out, "launch %d (%s), host ahead" % (i, kind))
        # the same hard launches with the verdicts in sight
        h.debug_set_adaptive_order(True)
        spans = []
        for i in range(12):
            out = outs[i]
            out[0].fill_(0xAB)
            out[1].fill_(-1)
            torch.cuda.current_stream().synchronize()
            launch(h, "hard", out, s.cuda_stream)
            s.synchronize()
            spans.append(h.debug_adaptive_state()[0])
            check("hard", out, "launch %d, synchronised" % i)
        assert 8 in spans, spans


# ---- capture and replay -------------------------------------------------------------------------------------------------
CAPTURABLE = sc.names(lambda c: c.capturable)


@pytest.fixture(scope="module")
def capture_report(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("capture") / "report.json")
    run = subprocess.run([sys.executable, os.path.join(HERE, "stream_capture_child.py"), path], capture_output=True,
                         text=True, timeout=600)
    report = json.load(open(path)) if os.path.exists(path) else {"cases": {}, "stopped_at": "before the first case"}
    report["tail"] = (run.stdout + run.stderr)[-1500:]
    report["returncode"] = run.returncode
    return report


@pytest.mark.parametrize("name", CAPTURABLE)
def test_captured_call_replays_on_new_inputs(name, capture_report):
    entry = capture_report["cases"].get(name)
    assert entry is not None, "did not run: the child stopped at %r (exit %s)\n%s" % (
        capture_report["stopped_at"], capture_report["returncode"], capture_report["tail"])
    assert entry["error"] is None, entry["error"]
    assert entry["replays"] == [True, True, True], "replays on X, D, X against their references: %s, first difference in %s" % (
        entry["replays"], entry["differs"])
