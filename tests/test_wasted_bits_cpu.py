"""FLACENC_HIP_FLAG_WASTED_BITS without a GPU: the model (tests/wasted_model.py) on the golden fixtures, its frames read
back by the decoder's CPU build, and the flag / record layout as every binding states it."""
import os
import re

import numpy as np
import pytest

import util
import wasted_model as wm
from flacenc_rs_amd import _capi, decode_cpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def golden_frames():
    """4 stereo frames of 4096: sus109 and ras22, two each."""
    for name in ("sus109", "ras22"):
        l, r = util.test_signal(name, 0), util.test_signal(name, 1)
        for f in range(2):
            yield l[f * 4096:(f + 1) * 4096], r[f * 4096:(f + 1) * 4096]


@pytest.mark.parametrize("shift,bps,today,wasted", [(0, 16, 42196, 42196), (8, 24, 74982, 42301), (4, 20, 58584, 42297)])
def test_model_reproduces_the_size_table(shift, bps, today, wasted):
    fc = wm.frame_config(order=8)
    frames = list(golden_frames())
    assert sum(wm.stereo_bits(l << shift, r << shift, bps, fc, wasted=False) for l, r in frames) // 8 == today
    assert sum(wm.stereo_bits(l << shift, r << shift, bps, fc) for l, r in frames) // 8 == wasted


def test_wasted_of_follows_the_semantics():
    fc = wm.frame_config()
    assert wm.wasted_of(np.array([4, 8, -12]), fc) == 2
    assert wm.wasted_of(np.zeros(16, np.int32), fc) == 0               # OR 0
    assert wm.wasted_of(np.full(16, 8), fc) == 0                       # constant with use_constant: Constant, k = 0
    assert wm.wasted_of(np.full(16, 8), wm.frame_config(use_constant=False)) == 3
    assert wm.wasted_of(np.array([-(1 << 23), 0]), fc) == 23           # k = w - 1


@pytest.fixture(scope="module")
def dec():
    return decode_cpu.DecoderCpu(decode_cpu.build())


def _decode(dec, frames, channels, bps, n):
    data = b"".join(frames)
    lens = [len(f) for f in frames]
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
    out, bs, _, st = dec.decode_frames(data, offs, lens, channels, bps, n)
    assert list(st) == [0] * len(frames)
    assert list(bs) == [n] * len(frames)
    return out


@pytest.mark.parametrize("use_fixed", [False, True])
def test_model_stereo_frames_decode_to_the_input(dec, use_fixed):
    fc = wm.frame_config(order=8, use_fixed=use_fixed)
    n = 1152
    l0, r0 = util.test_signal("sus109", 0)[:n], util.test_signal("sus109", 1)[:n]
    cases = [
        (l0 << 8, r0 << 8, 24),                    # 16-bit content at 24 bits
        (l0 << 4, r0 << 4, 20),
        (l0 << 1, r0 << 1, 16),
        (l0 << 3, (r0 << 3) | 1, 24),               # L wasted, R not
        (l0 << 2, r0 << 5, 24),                    # different k
        ((l0 << 1) | 1, (l0 << 1) | 1, 16),         # S = 0 (silence), L / R odd
        (np.full(n, -(1 << 23)), np.zeros(n, np.int64), 24),  # k = w - 1
    ]
    for i, (l, r, bps) in enumerate(cases):
        b = wm.stereo_frame_bytes(l, r, bps, fc, number=i)
        out = _decode(dec, [b], 2, bps, n)
        assert np.array_equal(out[0, 0], l) and np.array_equal(out[0, 1], r), i


def test_model_wasted_frames_are_shorter_and_carry_the_flag():
    fc = wm.frame_config(order=8)
    l, r = util.test_signal("ras22", 0)[:4096], util.test_signal("ras22", 1)[:4096]
    a, subs = wm.stereo_decision(l << 8, r << 8, 24, fc)
    assert [subs[i]["k"] for i in wm.STEREO_ROLES[a]] == [8, 8]
    plain = wm.stereo_frame_bytes(l, r, 16, wm.frame_config(order=8))
    assert len(wm.stereo_frame_bytes(l << 8, r << 8, 24, fc)) - len(plain) in (2, 3)


def test_model_independent_frames_decode_to_the_input(dec):
    fc = wm.frame_config(order=8, stereo=False)
    n = 576
    xs = [util.test_signal("ras103", c % 2)[:n] << (c + 1) for c in range(3)]
    b = wm.channel_frame_bytes(xs, 20, fc)
    out = _decode(dec, [b], 3, 20, n)
    for c in range(3):
        assert np.array_equal(out[0, c], xs[c])


def _read(path):
    with open(os.path.join(ROOT, path)) as f:
        return f.read()


def test_flag_constant_agrees_across_bindings():
    assert _capi.FLAG_WASTED_BITS == 512
    assert re.search(r"#define FLACENC_HIP_FLAG_WASTED_BITS 512u\b", _read("include/flacenc_hip.h"))
    assert re.search(r"pub const FLAG_WASTED_BITS: u32 = 512;", _read("rust/flacenc_hip.rs"))
    flags = [v for k, v in vars(_capi).items() if k.startswith("FLAG_")]
    assert len(flags) == len(set(flags))  # (no other flag took the bit)


def test_records_keep_their_layout():
    assert _capi.ABI_VERSION == 6
    assert _capi.FRAME_RESULT_DTYPE.itemsize == 752
    assert _capi.CHANNEL_RESULT_DTYPE.itemsize == 368
    assert _capi.FRAME_RESULT_DTYPE.fields["pad"][1] == 6
    assert _capi.CHANNEL_RESULT_DTYPE.fields["pad"][1] == 2
    fr = np.zeros(3, _capi.FRAME_RESULT_DTYPE)
    fr["pad"][1] = (8, 7)
    assert _capi.wasted_bits(fr).tolist() == [[0, 0], [8, 7], [0, 0]]
    cr = np.zeros(2, _capi.CHANNEL_RESULT_DTYPE)
    cr["pad"][1, 0] = 4
    assert _capi.wasted_bits(cr).tolist() == [0, 4]
