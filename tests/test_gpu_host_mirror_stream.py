"""The C++ host mirror's streams (flacenc_rs_amd/host/flacenc.hpp: encode_with_fixed_block_size in its one-handle and
several-handle forms, Stream::to_bytes, StreamInfo, the HipContext search setters) held to the CPU oracle byte for byte,
and the mirror's way back (decode_frames, decode_pcm, decode_streams, decode_streams_md5, md5_spans) to the input.

tests/host/mirror_stream_tool.cpp runs every case of CASES in ONE process; a module-scoped fixture builds it, writes the
cases, runs it once under a timeout of its own and the parametrized tests read what it wrote -- they do no GPU work.  If
the driver dies or times out every test of the module fails on the fixture; nothing retries.

Expected bytes come from the CPU alone: a frame is stated by tests/stream_seam_cases.py's Model (the oracle's controller
and bit writer in the summation order the mirror's SumOrder chooses) or, with a search setter, by order_model,
window_model, guess_model or precision_model with the K, floor and windows the case sets; STREAMINFO's 34 bytes are
restated here from bitrepr.rs:246-263, datatype.rs:476-523 and coding.rs:676-693 over the EXPECTED frames, the MD5 field
all zero (the mirror documents one stream's MD5 as host work).  The one exception is `nightly_order8`: the oracle models
no frame in the simd-nightly summation order, so that case is differential -- its frames come from the Python binding's
encode_pack_* with FLACENC_HIP_FLAG_NIGHTLY_SUM_ORDER, the same library through another host path.

Everything compared is integers and bytes: every comparison is exact.

DRIVER_TIMEOUT: the driver's one run (a cold process, its first handle included) took 0.80 s of wall time on an MI355X,
0.59 s by its own clock; five times that is below the floor of 60 s, so the floor it is."""
import functools
import hashlib
import os
import subprocess

import numpy as np
import pytest

import flac_parse
import guess_model as gm
import order_model as om
import precision_model as pm
import stream_seam_cases as seam
import util
import window_model as wm
from oracle import oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER_TIMEOUT = 60
CANONICAL, STABLE, NIGHTLY = 0, 1, 2   # HipContext::SumOrder
CONFIG = "EncodeError::Config"
NO_ROOM = 256                          # FLACENC_HIP_DECODE_NO_ROOM
DEFAULTS = dict(channels=2, bits=16, rate=44100, block_size=4096, handles=1, wayback=0,
                use_constant=1, use_fixed=1, use_lpc=1, fixed_max_order=4, fixed_order_sel=1, fixed_partitions=16,
                lpc_order=10, quant_precision=15, window_type=1, tukey_alpha=0.4, max_parameter=30,
                use_leftside=1, use_rightside=1, use_midside=1, sum_order=CANONICAL,
                order_search=0, window_search=0, order_guess=0, precision_search=0, order_guesses=1,
                precision_floor=pm.DEFAULT_FLOOR)
SEARCHES = ("order_search", "window_search", "order_guess", "precision_search")
KINDS = ("constant", "verbatim", "fixed", "lpc")   # the sidecar's kind numbers = component::SubFrame's alternatives
TAG_OF_ASSIGNMENT = {1: 8, 2: 9, 3: 10}            # component::ChannelAssignment -> the frame header's channel tag


def build_tool():
    """Built like host_mirror_test (tests/test_host_mirror_gpu.py: build_host_test)."""
    out = os.path.join(ROOT, "tests", "host", "mirror_stream_tool")
    cmd = ["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"),
           "-I", os.path.join(ROOT, "flacenc_rs_amd", "host"),
           os.path.join(ROOT, "tests", "host", "mirror_stream_tool.cpp"),
           "-L", os.path.join(ROOT, "flacenc_rs_amd"), "-lflacenc_hip",
           "-Wl,-rpath," + os.path.join(ROOT, "flacenc_rs_amd"), "-Wl,-rpath,/opt/rocm/lib",
           "-L/opt/rocm/lib", "-lamdhip64", "-pthread", "-o", out]
    subprocess.check_call(cmd)
    return out


# ---------------------------------------------------------------------------------------------------- material ----
def tone(n, bits, seed, C=2, namp=0.03):
    """int32 [n, C] interleaved: tone + noise, every channel its own period, phase and noise."""
    return np.stack([util.sine_noise(n, bits, 57.0 + 13 * c + seed % 11, 0.35, namp, 4000 + 17 * seed + c, phase=0.7 * c)
                     for c in range(C)], axis=1)


def full_noise(n, bits, seed, C=2):
    lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
    return np.random.default_rng(0xF00 + seed).integers(lo, hi + 1, (n, C)).astype(np.int32)


def slow_ramp(n, C=2):
    """x[t] = 3t - 1000 (tests/escape_cases.py: ramp) and its mirror image: the fixed predictor's material."""
    t = np.arange(n, dtype=np.int64)
    return np.stack([(3 * t - 1000) * (1 if c % 2 == 0 else -1) + 5 * c for c in range(C)], axis=1).astype(np.int32)


def four_assignments(n, seed=0):
    """int32 [4 n, 2]: one block for each stereo assignment.  Independent: a tone and an unrelated loud noise.
    LeftSide: the left channel a clean tone, the right one that tone plus noise (the side is the noise alone, and the left is cheaper than the mid).
    RightSide: the same with the channels swapped.  MidSide: the clean tone plus a noise in one channel and minus the same
    noise in the other: the mid is the clean tone, the side twice the noise."""
    rng = np.random.default_rng(0xA55 + seed)
    clean = util.sine_noise(n, 16, 83.0, 0.3, 0.0, 1).astype(np.int64)
    rough = clean + rng.integers(-300, 301, n)
    apart = rng.integers(-300, 301, n)
    blocks = [np.stack([util.sine_noise(n, 16, 61.0, 0.3, 0.01, 2).astype(np.int64), rng.integers(-9000, 9001, n)], axis=1),
              np.stack([clean, rough], axis=1),
              np.stack([rough, clean], axis=1),
              np.stack([clean + apart, clean - apart], axis=1)]
    return np.concatenate(blocks).astype(np.int32)


def four_kinds(n):
    """int32 [4 n, 2]: silence, full-scale noise, a slow ramp, tone + noise -- Constant, Verbatim, FixedLpc and Lpc."""
    return np.concatenate([np.zeros((n, 2), np.int32), full_noise(n, 16, 1), slow_ramp(n), tone(n, 16, 5)])


# ------------------------------------------------------------------------------------------------------- cases ----
class Case:
    def __init__(self, name, pcm, expect="stream", differential=False, windows=wm.DEFAULT, kinds=(), assignments=(),
                 tail=None, frames=None, differs_from=None, **settings):
        unknown = set(settings) - set(DEFAULTS)
        assert not unknown, unknown
        self.name, self.expect, self.differential, self.windows = name, expect, differential, tuple(windows)
        self.s = dict(DEFAULTS, **settings)
        C = self.s["channels"]
        self.pcm = np.ascontiguousarray(pcm, np.int32).reshape(-1, C)
        # what the CPU test holds the case to: the subframe kinds and assignments its model must choose, its last
        # block's size, its frame count, and the case (same material, no search) its model bytes must differ from
        self.kinds, self.assignments, self.tail, self.n_frames, self.differs_from = kinds, assignments, tail, frames, differs_from

    @property
    def search(self):
        return any(self.s[k] for k in SEARCHES)

    def blocks(self):
        n = self.s["block_size"]
        return [np.ascontiguousarray(self.pcm[t:t + n].T) for t in range(0, len(self.pcm), n)]


def _cases():
    out = []
    add = lambda *a, **k: out.append(Case(*a, **k))  # noqa: E731
    n = 4096
    # the fused stereo path and its tail batch
    add("stereo_defaults", tone(2 * n, 16, 0), frames=2, kinds=("lpc",))
    add("stereo_order8_nofixed", tone(2 * n, 16, 1), frames=2, lpc_order=8, use_fixed=0)
    add("stereo_tail1000", tone(3 * n + 1000, 16, 2), frames=4, tail=1000, wayback=1)
    for rate in (48000, 16000, 12345):   # (12345: the header's 16-bit rate field; 44100 is every other case's)
        add("stereo_rate%d" % rate, tone(2 * n, 16, 0), frames=2, rate=rate)
    # other kernel families
    add("stereo_1152", tone(2 * 1152 + 300, 16, 3), frames=3, tail=300, block_size=1152)
    add("stereo_8192x24_order12", tone(2 * 8192, 24, 4), frames=2, block_size=8192, bits=24, lpc_order=12)
    add("stereo_256", tone(3 * 256, 16, 5), frames=3, block_size=256)
    # independent channels, each with a ragged tail
    add("mono_4096", tone(2 * n + 777, 16, 6, C=1), frames=3, tail=777, channels=1, wayback=1)
    add("three_1000x24", tone(2 * 1000 + 333, 24, 7, C=3), frames=3, tail=333, channels=3, block_size=1000, bits=24, wayback=1)
    add("eight_256", tone(2 * 256 + 100, 16, 8, C=8), frames=3, tail=100, channels=8, block_size=256)
    # what used to be the host-controller branch: blocks below 64 samples, configs without predictors
    add("stereo_tail17", tone(2 * n + 17, 16, 9), frames=3, tail=17, kinds=("verbatim",))
    add("mono_tail17", tone(2 * 1000 + 17, 16, 10, C=1), frames=3, tail=17, channels=1, block_size=1000, kinds=("verbatim",))
    add("stereo_40_samples", tone(40, 16, 11), frames=1, tail=40, kinds=("verbatim",))
    add("stereo_tail63", tone(2 * 256 + 63, 16, 12), frames=3, tail=63, block_size=256, kinds=("verbatim",))
    add("stereo_tail64", tone(2 * 256 + 64, 16, 12), frames=3, tail=64, block_size=256)
    silent_then_tone = np.concatenate([np.full((256, 2), -7, np.int32), tone(256, 16, 13)])
    add("no_predictors_constant_on", silent_then_tone, frames=2, block_size=256, use_lpc=0, use_fixed=0,
        kinds=("constant", "verbatim"))
    add("no_predictors_constant_off", silent_then_tone, frames=2, block_size=256, use_lpc=0, use_fixed=0, use_constant=0,
        kinds=("verbatim",))
    add("mono_no_predictors", tone(2 * 256 + 17, 16, 14, C=1), frames=3, tail=17, channels=1, block_size=256, use_lpc=0,
        use_fixed=0, kinds=("verbatim",))
    # STREAMINFO edges
    add("one_frame_3000", tone(3000, 16, 15), frames=1, tail=3000)
    add("empty_source", np.zeros((0, 2), np.int32), frames=0)
    add("all_one_constant", np.full((3 * 256, 2), 1234, np.int32), frames=3, block_size=256, kinds=("constant",))
    # stereo toggles
    four = four_assignments(1152)
    add("stereo_all_assignments", four, frames=4, block_size=1152, assignments=(0, 1, 2, 3))
    add("stereo_left_only", four, frames=4, block_size=1152, use_rightside=0, use_midside=0, assignments=(0, 1))
    add("stereo_right_only", four, frames=4, block_size=1152, use_leftside=0, use_midside=0, assignments=(0, 2))
    add("stereo_mid_only", four, frames=4, block_size=1152, use_leftside=0, use_rightside=0, assignments=(0, 3))
    add("stereo_no_toggles", four, frames=4, block_size=1152, use_leftside=0, use_rightside=0, use_midside=0, assignments=(0,))
    # subframe kinds
    add("stereo_all_kinds", four_kinds(n), frames=4, kinds=KINDS)
    add("three_all_kinds", np.concatenate([four_kinds(1000), four_kinds(1000)[:, :1]], axis=1), frames=4, channels=3,
        block_size=1000, kinds=KINDS)
    # sum orders (Canonical: every other case)
    add("stable_order", tone(2 * n + 500, 16, 16), frames=3, tail=500, sum_order=STABLE)
    add("stable_order_mono_1000", tone(2 * 1000, 16, 17, C=1), frames=2, channels=1, block_size=1000, sum_order=STABLE)
    add("nightly_order8", tone(2 * n + 500, 16, 18), frames=3, tail=500, sum_order=NIGHTLY, lpc_order=8, differential=True)
    add("nightly_order16_is_canonical", tone(2 * n, 16, 19), frames=2, sum_order=NIGHTLY, lpc_order=16)
    # the searches, each on 2 x 1000 x 16 and 2 x 4096 x 16 at order 8
    two_windows = ((wm.PARTIAL_TUKEY, 0.5, 0, 32768), (wm.PUNCHOUT_TUKEY, 0.1, 16384, 49152))
    searches = [("order", dict(order_search=1), wm.DEFAULT),
                ("window", dict(window_search=1), wm.DEFAULT),
                ("guess", dict(order_guess=1), wm.DEFAULT),
                ("precision", dict(precision_search=1), wm.DEFAULT),
                ("order_window", dict(order_search=1, window_search=1), wm.DEFAULT),
                ("guess2_window", dict(order_guess=1, window_search=1, order_guesses=2), wm.DEFAULT),
                ("precision_floor8", dict(precision_search=1, precision_floor=8), wm.DEFAULT),
                ("precision_order", dict(precision_search=1, order_search=1), wm.DEFAULT),
                ("two_windows", dict(window_search=1), two_windows)]
    for block in (1000, 4096):
        x = tone(2 * block, 16, 20 + block % 7, namp=0.3)
        add("unflagged_%d" % block, x, frames=2, block_size=block, lpc_order=8)
        for label, flags, windows in searches:
            add("search_%s_%d" % (label, block), x, frames=2, block_size=block, lpc_order=8, windows=windows,
                differs_from="unflagged_%d" % block, **flags)
        # the same context with the searches switched off again: the unflagged bytes
        add("after_searches_%d" % block, x, frames=2, block_size=block, lpc_order=8)
    add("search_conflict", tone(2 * 1000, 16, 21), expect=CONFIG, block_size=1000, lpc_order=8, order_search=1, order_guess=1)
    # several handles: frames that do not divide by G, the short tail on a rank other than 0
    for G in (2, 3):
        add("handles%d_stereo" % G, tone(4 * n + 17, 16, 22), frames=5, tail=17, handles=G)
        add("handles%d_three" % G, tone(4 * 1000 + 17, 16, 23, C=3), frames=5, tail=17, channels=3, block_size=1000, handles=G)
    add("handles2_worker_config_error", tone(4 * 1000, 16, 24), expect=CONFIG, block_size=1000, lpc_order=8, handles=2,
        order_search=1, order_guess=1)
    # errors: nothing is written for any of them
    loud = tone(2 * n, 16, 25)
    loud[n + 5, 1] = 32768
    add("sample_out_of_range", loud, expect=CONFIG)
    add("lpc_order_25", tone(n, 16, 26), expect=CONFIG, lpc_order=25)
    add("fixed_max_order_5", tone(n, 16, 26), expect=CONFIG, fixed_max_order=5)
    add("nine_channels", tone(256, 16, 27, C=9), expect=CONFIG, channels=9, block_size=256)
    add("bits_3", np.zeros((256, 2), np.int32), expect=CONFIG, bits=3, block_size=256)
    add("bits_25", np.zeros((256, 2), np.int32), expect=CONFIG, bits=25, block_size=256)
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
STREAMS = [c.name for c in CASES if c.expect == "stream"]
ERRORS = [c.name for c in CASES if c.expect != "stream"]
WAYBACK = [c.name for c in CASES if c.s["wayback"]]
CPU_STATED = [c.name for c in CASES if c.expect == "stream" and not c.differential]


# ------------------------------------------------------------------------------------------ the CPU's statement ----
def frame_writer(c):
    """-> f(x int32 [C, n], number) -> the frame's bytes, from the models alone."""
    s = c.s
    window = ("tukey", s["tukey_alpha"]) if s["window_type"] else "rectangle"
    if c.search:
        assert s["sum_order"] == CANONICAL
        acorr, sums = orc.ACORR_REFERENCE, orc.SUMABS_STABLE            # (as stream_seam_cases.configs states a search)
    elif s["sum_order"] == STABLE:
        acorr, sums = seam.ORACLE_FLAGS[seam._capi.FLAG_REFERENCE_SUM_ORDER]
    else:   # Canonical, and SimdNightly above order 15 (HipContext::sum_order_flags)
        assert s["sum_order"] == CANONICAL or s["lpc_order"] > 15
        acorr, sums = seam.ORACLE_FLAGS[0]
    qlpc = orc.make_config(lpc_order=s["lpc_order"], quant_precision=s["quant_precision"], window=window,
                           max_rice_parameter=s["max_parameter"], acorr=acorr)
    fixed = orc.make_fixed_config(max_order=s["fixed_max_order"], order_sel=s["fixed_order_sel"],
                                  partitions=s["fixed_partitions"], sum_mode=sums)
    ofc = orc.make_frame_config(qlpc, use_constant=s["use_constant"], use_fixed=s["use_fixed"], use_lpc=s["use_lpc"],
                                use_leftside=s["use_leftside"], use_rightside=s["use_rightside"],
                                use_midside=s["use_midside"], fixed=fixed)
    bps, rate = s["bits"], s["rate"]
    if not c.search:
        model = seam.Model(0, False, ofc)
        return lambda x, number: model.frame(x, bps, rate, number)
    extras = c.windows if s["window_search"] else ()
    if s["precision_search"]:
        model = pm.Model(s["precision_floor"], extras, bool(s["order_search"]), s["order_guesses"] if s["order_guess"] else 0)
    elif s["order_guess"]:
        model = gm.Model(s["order_guesses"], extras)
    elif s["window_search"]:
        model = wm.Model(extras, bool(s["order_search"]))
    else:
        model = om

    def write(x, number):
        if x.shape[0] == 2:
            return model.stereo_frame_bytes(x[0], x[1], bps, ofc, number=number, sample_rate=rate)
        return model.channel_frame_bytes(list(x), bps, ofc, number=number, sample_rate=rate)
    return write


def stream_info(rate, channels, bits, total_samples, frames):
    """STREAMINFO's 34 bytes.  `frames`: [(block size, bytes)].  StreamInfo::new (datatype.rs:476-479) starts at
    min_block u16::MAX, max_block 0, min_frame u32::MAX, max_frame 0; update_frame_info (:514-523) takes min / max over
    the frames; the fixed-block encoder then writes the largest block twice if there is a frame (coding.rs:681-687);
    write (bitrepr.rs:246-263): u16, u16, 24 bits, 24 bits (the low bits of u32::MAX), 20 + 3 + 5 + 36 bits, the MD5."""
    min_block, max_block, min_frame, max_frame = 0xFFFF, 0, 0xFFFFFFFF, 0
    for block, size in frames:
        min_block, max_block = min(min_block, block), max(max_block, block)
        min_frame, max_frame = min(min_frame, size), max(max_frame, size)
    if frames:
        min_block = max_block
    packed = (rate << 44) | ((channels - 1) << 41) | ((bits - 1) << 36) | total_samples
    return (min_block.to_bytes(2, "big") + max_block.to_bytes(2, "big") + (min_frame & 0xFFFFFF).to_bytes(3, "big")
            + (max_frame & 0xFFFFFF).to_bytes(3, "big") + packed.to_bytes(8, "big") + bytes(16))


def stream_bytes(c, frames):
    s = c.s
    info = stream_info(s["rate"], s["channels"], s["bits"], len(c.pcm), [(b.shape[1], len(f)) for b, f in zip(c.blocks(), frames)])
    return b"fLaC" + bytes([0x80, 0, 0, 34]) + info + b"".join(frames)


@functools.lru_cache(None)
def model_frames(name):
    return frames_of(BY_NAME[name])


def frames_of(c):
    assert not c.differential
    write = frame_writer(c)
    return tuple(write(x, number) for number, x in enumerate(c.blocks()))


@functools.lru_cache(None)
def parsed(frame, bits, rate):
    p = flac_parse.parse_frame(frame, stream_bps=bits, stream_rate=rate)
    assert p["length"] == len(frame)
    return p


def pack_le(x, bits):
    """int32 [T, C] -> interleaved little-endian bytes at ceil(bits / 8) per sample: what the STREAMINFO MD5 covers."""
    flat = np.ascontiguousarray(x, "<i4").reshape(-1)
    return np.ascontiguousarray(flat.view(np.uint8).reshape(-1, 4)[:, :(bits + 7) // 8]).tobytes()


def test_the_models_state_every_case_and_what_it_claims():
    """CPU: every case has an expectation built from the models alone, and the material does what the case says it does:
    the tail sizes and frame counts are as listed, each subframe kind and each channel assignment is really chosen, and
    every search case's model bytes differ from the unflagged model's on the same material (a setter that is silently
    ignored cannot pass).  nightly_order8 is the one case without a CPU statement (see the module's docstring)."""
    assert [c.name for c in CASES if c.differential] == ["nightly_order8"]
    for c in CASES:
        if c.expect != "stream":
            assert c.expect == CONFIG
            continue
        blocks = c.blocks()
        assert len(blocks) == c.n_frames, c.name
        if c.tail is not None:
            assert blocks[-1].shape[1] == c.tail and c.tail <= c.s["block_size"], c.name
        if c.differential:
            continue
        frames = model_frames(c.name)
        assert len(frames) == len(blocks) and all(frames), c.name
        kinds, tags = set(), set()
        for number, (f, x) in enumerate(zip(frames, blocks)):
            p = parsed(f, c.s["bits"], c.s["rate"])
            assert p["number"] == number and p["block_size"] == x.shape[1] and np.array_equal(p["channels"], x), (c.name, number)
            kinds |= set(p["kinds"])
            tags.add(p["channel_tag"])
        assert set(c.kinds) <= kinds, (c.name, kinds)
        if c.assignments:
            assert tags == {TAG_OF_ASSIGNMENT.get(a, 1) for a in c.assignments}, (c.name, tags)
        if c.differs_from:
            base = BY_NAME[c.differs_from]
            assert np.array_equal(base.pcm, c.pcm) and not base.search and c.search
            assert frames != model_frames(base.name), c.name
        assert len(stream_bytes(c, frames)) == 42 + sum(map(len, frames))
    # the case that follows the searches on the same context is the unflagged one again
    # ... and the handle's own settings count: two guesses are not one, a floor of 8 is not the default floor, the two
    # custom windows are not the default list
    for block in (1000, 4096):
        assert model_frames("after_searches_%d" % block) == model_frames("unflagged_%d" % block)
        of = lambda label: model_frames("search_%s_%d" % (label, block))  # noqa: E731
        one_guess = Case("one_guess", BY_NAME["unflagged_%d" % block].pcm, block_size=block, lpc_order=8, order_guess=1,
                         window_search=1)
        assert of("guess2_window") != frames_of(one_guess)
        assert of("precision_floor8") != of("precision") and of("two_windows") != of("window")
    every = lambda key: {v for c in CASES if c.expect == "stream" and not c.differential  # noqa: E731
                         for f in model_frames(c.name) for v in parsed(f, c.s["bits"], c.s["rate"])[key]}
    assert every("kinds") == set(KINDS)
    assert {c.tail for c in CASES} >= {17, 40, 63, 64, 1000, 3000}
    # the empty source keeps StreamInfo::new's values; a stream below one block says its own size twice
    assert stream_info(44100, 2, 16, 0, [])[:10] == bytes.fromhex("ffff0000ffffff000000")
    assert stream_info(44100, 2, 16, 3000, [(3000, 77)])[:10] == bytes.fromhex("0bb80bb800004d00004d")


def test_the_driver_compiles():
    """CPU: the driver compiles and links against the header-only mirror and the C ABI."""
    assert os.path.exists(build_tool())


# --------------------------------------------------------------------------------------------------- the one run ----
MD5_SPANS = ((1, 0), (3, 55), (61, 56), (121, 64), (301, 1000))   # (offset, length): odd offsets, the padding's edges
MD5_BLOB = np.random.default_rng(0x3D5).integers(0, 256, 1400, dtype=np.uint8).tobytes()


def write_cases(d):
    lines = []
    for c in CASES:
        lines.append("case %s" % c.name)
        lines += ["%s %s" % kv for kv in c.s.items()]
        lines += ["win %d %r %d %d" % w for w in c.windows]
        lines.append("end")
        c.pcm.tofile(os.path.join(d, c.name + ".pcm"))
    with open(os.path.join(d, "cases.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    with open(os.path.join(d, "md5.bin"), "wb") as f:
        f.write(MD5_BLOB)
    with open(os.path.join(d, "md5_spans.txt"), "w") as f:
        f.write("".join("%d %d\n" % s for s in MD5_SPANS))


class Run:
    def __init__(self, d, nightly):
        self.d, self.nightly = d, nightly
        with open(self.path("wayback.txt")) as f:
            self.wayback = [line.split() for line in f]

    def path(self, name):
        return os.path.join(self.d, name)

    def read(self, name):
        with open(self.path(name), "rb") as f:
            return f.read()

    def rows(self, key, name=None):
        return [r[1:] for r in self.wayback if r[0] == key and (name is None or r[1] == name)]

    def expected_frames(self, name):
        return self.nightly if BY_NAME[name].differential else model_frames(name)

    def side(self, name):
        """-> (info fields, [(frame fields, [subframe fields])], round trip)."""
        info, frames, trip = None, [], None
        for row in self.read(name + ".side").decode().splitlines():
            w = row.split()
            if w[0] == "info":
                info = [int(v) for v in w[1:9]] + [w[9]]
            elif w[0] == "frame":
                frames.append(([int(v) for v in w[1:]], []))
            elif w[0] == "sub":
                frames[-1][1].append([int(v) for v in w[1:]])
            elif w[0] == "roundtrip":
                trip = int(w[1])
        return info, frames, trip

    def got_frames(self, name):
        """The frames of the stream the mirror wrote, cut at the lengths its sidecar states."""
        data, at, out = self.read(name + ".flac"), 42, []
        for fields, _ in self.side(name)[1]:
            out.append(data[at:at + fields[3]])
            at += fields[3]
        assert at == len(data)
        return out


def nightly_frames():
    """nightly_order8's frames through the Python binding: one encode_pack_* launch over the full blocks and one over
    the tail, FLACENC_HIP_FLAG_NIGHTLY_SUM_ORDER in the config."""
    from flacenc_rs_amd import _capi
    c = BY_NAME["nightly_order8"]
    cfg = _capi.make_frame_config(_capi.make_config(lpc_order=c.s["lpc_order"], flags=_capi.FLAG_NIGHTLY_SUM_ORDER), use_fixed=True)
    blocks, frames = c.blocks(), []
    with _capi.Handle(0) as h:
        for number, x in enumerate(blocks):
            data, lens = seam.one_call(h, x[None], c.s["bits"], cfg, c.s["rate"], number, 1)
            assert len(data) == int(lens[0])
            frames.append(data)
    return tuple(frames)


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    exe = build_tool()
    d = str(tmp_path_factory.mktemp("mirror_stream"))
    write_cases(d)
    res = subprocess.run([exe, d], capture_output=True, text=True, timeout=DRIVER_TIMEOUT)
    print(res.stdout[-6000:], res.stderr[-3000:])
    assert res.returncode == 0, (res.returncode, res.stdout[-2000:], res.stderr[-2000:])
    assert os.path.exists(os.path.join(d, "done.txt"))
    return Run(d, nightly_frames())


# ------------------------------------------------------------------------------------------------------ streams ----
@pytest.mark.gpu
@pytest.mark.parametrize("name", STREAMS)
def test_stream_bytes(run, name):
    """fLaC, the expected STREAMINFO, the expected frames -- and every StreamInfo field of the sidecar says the same."""
    c = BY_NAME[name]
    assert not os.path.exists(run.path(name + ".err")), run.read(name + ".err")
    want_frames = run.expected_frames(name)
    want, got = stream_bytes(c, want_frames), run.read(name + ".flac")
    assert got[:8] == want[:8]
    assert got[8:42].hex() == want[8:42].hex(), "STREAMINFO"
    at = 42
    for number, f in enumerate(want_frames):
        assert got[at:at + len(f)] == f, "frame %d" % number
        at += len(f)
    assert got == want
    info = run.side(name)[0]
    sizes = [len(f) for f in want_frames]
    largest = max([x.shape[1] for x in c.blocks()], default=None)
    assert info == [c.s["rate"], c.s["channels"], c.s["bits"], largest or 0xFFFF, largest or 0,
                    min(sizes, default=0xFFFFFFFF), max(sizes, default=0), len(c.pcm), "00" * 16]


@pytest.mark.gpu
@pytest.mark.parametrize("name", STREAMS)
def test_frames_parse(run, name):
    """Every frame the mirror wrote parses (sync, both CRCs, every field) to its number, block size, rate and samples."""
    c = BY_NAME[name]
    blocks, frames = c.blocks(), run.got_frames(name)
    assert len(frames) == len(blocks)
    for number, (f, x) in enumerate(zip(frames, blocks)):
        assert f, "frame %d has no bytes" % number
        p = parsed(f, c.s["bits"], c.s["rate"])
        assert (p["number"], p["block_size"], p["sample_rate"], p["bps"]) == (number, x.shape[1], c.s["rate"], c.s["bits"])
        assert np.array_equal(p["channels"], x), number


@pytest.mark.gpu
@pytest.mark.parametrize("name", STREAMS)
def test_components_describe_the_bytes(run, name):
    """The Frame / SubFrame components of the sidecar are the model's choice, field by field, and count the frame's bits."""
    c = BY_NAME[name]
    want_frames = run.expected_frames(name)
    frames = run.side(name)[1]
    assert len(frames) == len(want_frames)
    for number, ((fields, subs), want) in enumerate(zip(frames, want_frames)):
        p = parsed(want, c.s["bits"], c.s["rate"])
        f_number, block, assignment, size = fields
        assert (f_number, block) == (number, p["block_size"])
        assert TAG_OF_ASSIGNMENT.get(assignment, c.s["channels"] - 1) == p["channel_tag"], number
        assert len(subs) == c.s["channels"]
        for k, sub in enumerate(subs):
            kind, bits, order, precision, shift, porder, count_bits, n_params = sub[:8]
            stated = (KINDS[kind], bits, order, precision, shift, porder, sub[8:])
            model = (p["kinds"][k], p["sub_bps"][k], p["orders"][k], p["precisions"][k], p["shifts"][k],
                     p["partition_orders"][k], p["rice_params"][k])
            assert stated == model, (number, k)
            assert n_params == len(sub[8:]) and count_bits == p["subframe_bits"][k], (number, k)
        # Frame::count_bits: the header, the subframes, the padding to a byte, the CRC-16
        total = p["header_bits"] + sum(sub[6] for sub in subs)
        assert (total + 7) // 8 * 8 + 16 == 8 * size, number


@pytest.mark.gpu
@pytest.mark.parametrize("name", STREAMS)
def test_round_trip(run, name):
    """Frame::decode_channels() of every frame gave the input (the driver compares; the sidecar says so)."""
    assert run.side(name)[2] == 1


@pytest.mark.gpu
@pytest.mark.parametrize("name", ERRORS)
def test_errors(run, name):
    """The exception's kind is the reference's -- EncodeError::Config -- and nothing was written."""
    assert not os.path.exists(run.path(name + ".flac")) and not os.path.exists(run.path(name + ".side"))
    kind, text = run.read(name + ".err").decode().split("\n", 1)
    assert kind == BY_NAME[name].expect, (kind, text)


# ------------------------------------------------------------------------------------------------- the way back ----
@pytest.mark.gpu
@pytest.mark.parametrize("name", WAYBACK)
def test_decode_frames(run, name):
    c = BY_NAME[name]
    rows, blocks = run.rows("df", name), c.blocks()
    assert [[int(v) for v in r[1:]] for r in rows] == [[0, number, x.shape[1]] for number, x in enumerate(blocks)]
    assert np.array_equal(np.fromfile(run.path(name + ".df.bin"), np.int32).reshape(-1, c.s["channels"]), c.pcm)


@pytest.mark.gpu
@pytest.mark.parametrize("name", WAYBACK)
def test_decode_pcm(run, name):
    c = BY_NAME[name]
    want, n_bytes = pack_le(c.pcm, c.s["bits"]), len(run.read(name + ".flac")) - 42
    (row,) = run.rows("dp", name)
    assert [int(v) for v in row[1:]] == [len(c.blocks()), len(c.pcm), n_bytes, 0]
    assert run.read(name + ".dp.bin") == want + b"\xcd" * 64


@pytest.mark.gpu
@pytest.mark.parametrize("name", WAYBACK)
def test_decode_pcm_without_room(run, name):
    """Room for 1.5 frames: one frame, FLACENC_HIP_DECODE_NO_ROOM, nothing written behind it; a second call finishes."""
    c = BY_NAME[name]
    block, per = c.s["block_size"], c.s["channels"] * ((c.s["bits"] + 7) // 8)
    want, lens = pack_le(c.pcm, c.s["bits"]), [len(f) for f in run.got_frames(name)]
    (r1,), (r2,) = run.rows("dp1", name), run.rows("dp2", name)
    assert int(r1[5]) == block * 3 // 2 * per
    assert [int(v) for v in r1[1:5]] == [1, block, lens[0], NO_ROOM]
    got = run.read(name + ".dp1.bin")
    assert got[:block * per] == want[:block * per] and got[block * per:] == b"\xcd" * (len(got) - block * per)
    assert [int(v) for v in r2[1:]] == [len(lens) - 1, len(c.pcm) - block, sum(lens[1:]), 0]
    rest = want[block * per:]
    assert run.read(name + ".dp2.bin") == rest + b"\xcd" * (len(want) - len(rest) + 64)


@pytest.mark.gpu
@pytest.mark.parametrize("key, blob", [("ds", "streams.bin"), ("dsmd5", "streams_md5.bin")])
def test_decode_streams(run, key, blob):
    """The three streams in one buffer: totals and bytes are decode_pcm's per stream, the digests hashlib's."""
    rows = run.rows(key)
    assert [r[0] for r in rows] == WAYBACK
    want = b""
    for r in rows:
        c = BY_NAME[r[0]]
        (single,) = run.rows("dp", c.name)
        assert r[1:5] == single[1:5]
        pcm = pack_le(c.pcm, c.s["bits"])
        if key == "dsmd5":
            assert r[5] == hashlib.md5(pcm).hexdigest(), c.name
        want += pcm
    assert run.read(blob) == want + b"\xcd" * 64


@pytest.mark.gpu
def test_decode_streams_limits(run):
    """max_frames one too small throws; an empty stream list returns empty."""
    for key in ("ds_small", "dsmd5_small"):
        (row,) = run.rows(key)
        assert row[:2] == ["threw", "Device"], row
    assert run.rows("ds_empty") == [["returned", "0"]]
    assert run.rows("dsmd5_empty") == [["returned", "0", "0"]]


@pytest.mark.gpu
def test_md5_spans(run):
    (row,) = run.rows("md5")
    assert row[:2] == ["returned", str(len(MD5_SPANS))]
    assert row[2:] == [hashlib.md5(MD5_BLOB[o:o + n]).hexdigest() for o, n in MD5_SPANS]
    assert run.rows("md5_empty") == [["returned", "0"]]
    (row,) = run.rows("md5_sizes")
    assert row[0] == "threw", row
