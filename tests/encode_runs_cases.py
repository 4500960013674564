"""The corpus of tests/test_gpu_encode_runs.py and tests/test_encode_runs_cpu.py: batches for flacenc_hip_encode_streams
whose *tail runs* -- the frame-level launch that holds the last, shorter block of every stream of one class that ends on
one tail length -- have the block sizes the kernel families are chosen by, several frames each, at the row stride of the
call's block size and in the interior of the class's buffers; and small batches across LPC orders, use_fixed and flags.

A case is a table: per class and tail length how many streams end on it, each with 0, 1 or 2 full blocks in front.
route() restates csrc/qlpc_dispatch.cpp's shape rule, so that the CPU test can say which kernel family every run of the
brute-force plan takes.  Streams, material, layout and packing are tests/encode_streams_cases.py's."""
import collections
import functools

import numpy as np

import encode_streams_cases as cases
from flacenc_rs_amd import _capi

Stream, material, layout, pack, slot_map = cases.Stream, cases.material, cases.layout, cases.pack, cases.slot_map

ROUTES = ("fused4096", "fused4608", "subwave64", "subwave72", "bigblock", "generic")
SUBWAVE = (256, 288, 512, 576, 1024, 1152, 2048, 2304)


def route(block, order):
    """The kernel family a frame-level launch of `block` samples at LPC order `order` takes, by its shape alone (aligned
    rows, no flag that forces the general path): wave_kernel_eligible, subwave_*_eligible and bigblock_eligible of
    csrc/qlpc_dispatch.cpp.  The fused and the sub-wave kernels stop at order 12."""
    if block < 64:
        return "generic"
    if block in (8192, 16384) or (block == 4096 and order >= 13):
        return "bigblock"
    if order <= 12:
        if block == 4096:
            return "fused4096"
        if block == 4608:
            return "fused4608"
        if block in SUBWAVE:
            return "subwave72" if block % 72 == 0 else "subwave64"     # spl of launch_qlpc
    return "generic"


# classes: (channels, bits, bytes per sample, rate)
MONO, STEREO = (1, 16, 2, 44100), (2, 16, 2, 44100)
STEREO24, THREE = (2, 24, 3, 48000), (3, 16, 4, 12345)
MONO24 = (1, 24, 3, 48000)
FULLS = {1: (0,), 3: (0, 1, 0), 5: (0, 1, 0, 2, 0)}     # full blocks in front of the tails of a run of 1, 3, 5 streams

Case = collections.namedtuple("Case", "name block order use_fixed flags groups chunk short material full_route")
Case.__new__.__defaults__ = (0, None, "plain", None)


def _route_case(name, block, order, groups, full_route, two_full=MONO, **kw):
    """groups: (tail, class, streams) in table order; a stream of exactly two full blocks of class `two_full` ends it."""
    return Case(name, block, order, True, 0, tuple(groups) + ((0, two_full, 0),), full_route=full_route, **kw)


A = (4096, STEREO, 3), (4096, MONO, 1), (2304, STEREO, 3), (1152, MONO, 5), (576, STEREO24, 3), (288, MONO, 3), \
    (4607, STEREO24, 3)
B = (2048, STEREO, 3), (1152, MONO, 3), (1024, MONO, 3), (576, STEREO, 3), (512, THREE, 3), (288, THREE, 3), \
    (256, STEREO, 5), (257, THREE, 3), (255, MONO, 3), (512, MONO, 1), (288, STEREO, 1)
C = (4608, STEREO, 3), (4608, MONO, 1), (4096, MONO, 3), (2048, STEREO24, 3), (1024, STEREO, 3), (8191, MONO, 3)
D = (4096, STEREO24, 3), (2304, STEREO24, 3), (8191, MONO24, 3), (4096, STEREO, 1), (2304, MONO, 3)
E = (2048, STEREO, 3), (4095, MONO, 3), (2048, THREE, 3), (4095, STEREO, 1)
F = (8192, STEREO, 3), (4096, MONO, 1)        # five streams: 4096 is a run of one frame here (A and C hold three)
G = (255, MONO, 3), (64, STEREO, 3), (63, STEREO24, 3), (64, MONO, 1), (63, STEREO, 1)

ROUTE_CASES = (
    _route_case("A", 4608, 8, A, "fused4608"),
    _route_case("A-chunk2", 4608, 8, A, "fused4608", chunk=2),
    # FLACENC_HIP_FLAG_FUSED_PACK: the stereo tail run of 4096 samples is written by the fused kernel's own bit writer
    # (it exists for 4096 alone), into pack slots as wide as a frame of 4608 samples needs
    _route_case("A-fused", 4608, 8, A, "fused4608")._replace(flags=_capi.FLAG_FUSED_PACK),
    _route_case("B", 2304, 10, B, "subwave72"),
    _route_case("B-short", 2304, 10, B, "subwave72", short=1152),
    _route_case("C", 8192, 12, C, "bigblock", two_full=STEREO),
    _route_case("D", 8192, 24, D, "bigblock", two_full=STEREO),
    _route_case("E", 4096, 13, E, "bigblock"),
    _route_case("F", 16384, 10, F, "bigblock"),
    _route_case("G", 256, 12, G, "subwave64"),
)

# ---- configs: block 576, tails 288 (sub-wave), 256 (sub-wave, the other form), 100 and 17 (generic, too short)
SMALL = (288, STEREO, 3), (256, MONO, 3), (100, THREE, 1), (17, THREE, 1), (100, STEREO, 1), (17, MONO, 1), (288, THREE, 3)
# under the flags whose model writes with tests/flac_write.py the rate is 44100 in every class
SMALL_44100 = tuple((t, STEREO24[:3] + (44100,) if k == THREE else k, n) for t, k, n in SMALL)
_F = _capi
FLAG_CASES = (("WASTED_BITS", _F.FLAG_WASTED_BITS), ("ORDER_SEARCH", _F.FLAG_ORDER_SEARCH),
              ("WINDOW_SEARCH", _F.FLAG_WINDOW_SEARCH), ("ORDER_GUESS", _F.FLAG_ORDER_GUESS),
              ("PRECISION_SEARCH", _F.FLAG_PRECISION_SEARCH), ("RICE_ESCAPE", _F.FLAG_RICE_ESCAPE),
              ("REFERENCE_SUM_ORDER", _F.FLAG_REFERENCE_SUM_ORDER), ("GENERIC_KERNEL", _F.FLAG_GENERIC_KERNEL),
              ("WASTED_BITS+ORDER_GUESS+WINDOW_SEARCH", _F.FLAG_WASTED_BITS | _F.FLAG_ORDER_GUESS | _F.FLAG_WINDOW_SEARCH),
              ("ORDER_SEARCH+WINDOW_SEARCH", _F.FLAG_ORDER_SEARCH | _F.FLAG_WINDOW_SEARCH),
              ("PRECISION_SEARCH+RICE_ESCAPE", _F.FLAG_PRECISION_SEARCH | _F.FLAG_RICE_ESCAPE))
CONFIG_CASES = tuple(
    Case("order%d-%s" % (order, "fixed" if use_fixed else "lpc"), 576, order, use_fixed,
         _F.FLAG_ALLOW_ORDER_32 if order == 32 else 0, SMALL + ((0, MONO, 0),), full_route=route(576, order))
    for order in (1, 10, 12, 16, 32) for use_fixed in (True, False)) + tuple(
    Case(name, 576, 8, True, flags, SMALL_44100 + ((0, MONO, 0),), material="flagged") for name, flags in FLAG_CASES)

CASES = ROUTE_CASES + CONFIG_CASES
BY_NAME = {c.name: c for c in CASES}
DEVICE_TOO = ("A", "C", "E", "WASTED_BITS", "PRECISION_SEARCH+RICE_ESCAPE")      # the same call in device memory
PLANAR_TOO = ("A", "B", "D", "ORDER_SEARCH", "WASTED_BITS+ORDER_GUESS+WINDOW_SEARCH")   # encode_streams_planar, both formats


@functools.lru_cache(None)
def _streams(block, groups, kind):
    out = []
    for g, (tail, (channels, bps, width, rate), count) in enumerate(groups):
        for k, full in enumerate(FULLS[count] if count else (2,)):
            total = full * block + tail
            name = "%dch%d in %d, %d blocks + %d, #%d" % (channels, bps, width, full, tail, k)
            # the material depends on what the stream is, not on the case: cases that share a stream share its frames
            seed = (tail * 7 + channels * 131 + bps * 17 + full * 3 + k) % 9973
            x = material(total, channels, bps, seed)
            if kind == "flagged" and len(out) % 3 == 1:        # low bits all zero in every channel
                x = np.ascontiguousarray((x >> 4) << 4)
            if kind == "flagged" and len(out) % 3 == 2:        # digital silence in the middle of the last block
                x[:, full * block + tail // 4:full * block + (3 * tail) // 4] = 0
            out.append(Stream(name, x, channels, bps, width, rate))
    return tuple(out)


def streams(case):
    """The case's streams in table order (stated once per table: the chunked and the cut variant share them)."""
    return _streams(case.block, case.groups, case.material)


def brute_plan(case):
    """The plan from the case's table, frame by frame: classes in order of first appearance; per class its full frames in
    one stretch, then its tails sorted by (length, stream); runs are maximal stretches of one class and one length, cut
    every `chunk` frames (0: the rule's chunk, which no case reaches).
    -> dict(classes, runs: [(class, block size of the run, frames, is tail)], full_runs, tail_runs, frames)."""
    ss = streams(case)
    key_of = lambda s: (s.channels, s.bps, s.width, s.rate)
    classes = []
    for s in ss:
        if key_of(s) not in classes:
            classes.append(key_of(s))
    chunk = case.chunk or 768
    runs = []
    for k in classes:
        mine = [s for s in ss if key_of(s) == k]
        full = sum(s.x.shape[1] // case.block for s in mine)
        for f in range(0, full, chunk):
            runs.append((k, case.block, min(chunk, full - f), False))
        tails = sorted(s.x.shape[1] % case.block for s in mine if s.x.shape[1] % case.block)
        for t in sorted(set(tails)):
            n = tails.count(t)
            for f in range(0, n, chunk):
                runs.append((k, t, min(chunk, n - f), True))
    frames = sum(cases.n_frames(s, case.block) for s in ss)
    assert frames == sum(r[2] for r in runs)
    tail_runs = sum(1 for r in runs if r[3])
    return dict(classes=classes, runs=runs, full_runs=len(runs) - tail_runs, tail_runs=tail_runs, frames=frames)
