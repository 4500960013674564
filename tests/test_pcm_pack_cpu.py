"""flacenc_hip_pack_le_bytes without a GPU: the numpy model (tests/pcm_pack_model.py) against the oracle's restatement
of fill_le_bytes in both directions, the host build of csrc/pcm_pack_core.h -- the device kernel's own index arithmetic,
walked frame by frame, slice by slice and lane by lane -- against the model on the shapes the GPU tests use, the new
symbols in the header and the binding, and the calls' answer to a NULL handle."""
import os
import re
import subprocess

import numpy as np
import pytest

import pcm_pack_model as model
from flacenc_rs_amd import _capi, pcm_pack_cpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def core():
    return pcm_pack_cpu.PackCore()


@pytest.mark.parametrize("bytes_per", model.BYTES)
@pytest.mark.parametrize("channels", model.CHANNELS)
def test_model_inverts_the_oracles_fill_le_bytes(bytes_per, channels):
    n, nf = 37, 5
    rng = np.random.default_rng(bytes_per * 10 + channels)
    # pack(fill(b)) == b for any bytes
    data = rng.integers(0, 256, nf * n * channels * bytes_per).astype(np.uint8)
    filled = model.fill_le_bytes(data, channels, bytes_per, n)
    out, off, total = model.pack_le_bytes(filled, [n] * nf, bytes_per)
    assert np.array_equal(out, data) and total == nf * n and off.tolist() == [f * n for f in range(nf + 1)]
    # fill(pack(x)) == x for every x that fits the width, the extremes included
    x = model.rows([n] * nf, channels, n, bytes_per, seed=channels)
    bits = 8 * bytes_per
    x = np.clip(x.astype(np.int64), -(1 << (bits - 1)), (1 << (bits - 1)) - 1).astype(np.int32)
    x[0, 0, :4] = [-(1 << (bits - 1)), (1 << (bits - 1)) - 1, -1, 0]
    packed, _, _ = model.pack_le_bytes(x, [n] * nf, bytes_per)
    assert np.array_equal(model.fill_le_bytes(packed, channels, bytes_per, n), x)


def test_model_keeps_the_low_bytes_of_values_that_do_not_fit():
    x = np.array([[[0x12345678, -0x12345678, 32768, -32769]]], np.int32)
    out, _, total = model.pack_le_bytes(x, [4], 2)
    assert total == 4 and out.tobytes() == bytes([0x78, 0x56, 0x88, 0xA9, 0x00, 0x80, 0xFF, 0x7F])


def test_div_channels_is_exact_for_every_element_of_a_slice(core):
    for channels in range(1, 9):
        assert core.div_check(channels) == -1, channels


def test_split_covers_the_span_once(core):
    for low2 in range(4):
        for length in list(range(0, 40)) + [4095, 4096, 4097, 32768]:
            head, n_dwords, tail = core.split(low2, length)
            assert head + 4 * n_dwords + tail == length and head < 4 and tail < 4
            assert head == min(length, (4 - low2) % 4)
            assert (low2 + head) % 4 == 0 or n_dwords == 0


@pytest.mark.parametrize("bytes_per", model.BYTES)
@pytest.mark.parametrize("channels", model.CHANNELS)
def test_host_build_of_the_core_equals_the_model(core, bytes_per, channels):
    bs = list(model.MIXED)
    for stride in (4096, 4101):
        x = model.rows(bs, channels, stride, bytes_per, seed=100 + stride)
        want, off, total = model.pack_le_bytes(x, bs, bytes_per)
        for addr in range(4):   # the address of out[0]: frame starts then sit on other alignments
            got = core.pack(x, bs, channels, bytes_per, out_addr=addr)
            assert got["rc"] == 0 and got["total"] == total and np.array_equal(got["offsets"], off)
            assert np.array_equal(got["out"], want), (stride, addr)
            assert (got["hits"] == 1).all(), "an output byte stored twice or never: spans overlap or leave a gap"
        assert not model.holds_sentinel(want, bytes_per, channels)
    if bytes_per in (1, 3) and channels in (1, 3):
        assert model.frame_start_alignments(bs, channels, bytes_per, 4096) == {0, 1, 2, 3}


def test_host_build_clamps_block_sizes_to_the_stride_and_refuses_a_short_output(core):
    x = model.rows([9, 9, 9], 2, 9, 3, seed=3)
    bs = [9, 4000000000, 2]
    want, off, total = model.pack_le_bytes(x, bs, 3)
    assert total == 20
    got = core.pack(x, bs, 2, 3)
    assert got["rc"] == 0 and np.array_equal(got["out"], want) and np.array_equal(got["offsets"], off)
    short = core.pack(x, bs, 2, 3, out_capacity=len(want) - 1)
    assert short["rc"] == 1 and short["total"] == total and (short["out"] == 0xEE).all() and not short["hits"].any()
    assert np.array_equal(short["offsets"], off)


def test_many_tiny_frames(core):
    """70000 frames of 1..3 samples at stride 4: more than one workgroup's worth of the scan, more than a grid.y."""
    rng = np.random.default_rng(7)
    bs = rng.integers(1, 4, 70000).astype(np.uint32)
    x = model.rows(bs, 1, 4, 3, seed=8)
    want, off, total = model.pack_le_bytes(x, bs, 3)
    got = core.pack(x, bs, 1, 3, out_addr=1)
    assert got["rc"] == 0 and got["total"] == total and np.array_equal(got["offsets"], off)
    assert np.array_equal(got["out"], want) and (got["hits"] == 1).all()


def test_sanitized_self_check_of_the_core():
    """The stand-alone driver of pcm_pack_cpu.cpp (PPK_MAIN) under ASan + UBSan: exact-size heap blocks for rows and output."""
    exe = pcm_pack_cpu.build_sanitized_driver()
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "self-check OK" in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]


def test_new_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "flacenc_hip.h")).read()
    lib = _capi.load()
    for name in ("flacenc_hip_pack_le_bytes", "flacenc_hip_decode_pcm"):
        assert re.search(r"^int %s\(" % name, header, re.M), name
        assert name in _capi.EXPORTED_SYMBOLS and getattr(lib, name).argtypes, name
    assert re.search(r"#define FLACENC_HIP_DECODE_NO_ROOM 256u", header) and _capi.DECODE_NO_ROOM == 256
    assert re.search(r"#define FLACENC_HIP_DECODE_CHAIN 512u", header) and _capi.DECODE_CHAIN == 512
    assert re.search(r"#define FLACENC_HIP_ABI_VERSION 6\b", header) and _capi.ABI_VERSION == 6
    for name in ("flacenc_hip_debug_set_decode_plan", "flacenc_hip_debug_last_decode_plan"):
        assert name in _capi.DEBUG_SYMBOLS and not hasattr(lib, name) and hasattr(_capi.load_hooks(), name)
    for method in ("pack_le_bytes", "pack_le_bytes_device", "decode_pcm"):
        assert callable(getattr(_capi.Handle, method))


def test_null_handle_is_a_bad_argument():
    lib = _capi.load()
    total = np.zeros(4, np.uint64)
    out = np.zeros(16, np.uint8)
    rows = np.zeros(4, np.int32)
    bs = np.ones(1, np.uint32)
    assert lib.flacenc_hip_pack_le_bytes(None, rows.ctypes.data, 4, bs.ctypes.data, 1, 1, 2, out.ctypes.data, 16, None,
                                         total.ctypes.data, _capi.MEM_HOST) == _capi.ERR_BAD_ARGUMENT
    assert lib.flacenc_hip_pack_le_bytes(None, rows.ctypes.data, 4, bs.ctypes.data, 1, 1, 2, out.ctypes.data, 16, None,
                                         total.ctypes.data, _capi.MEM_DEVICE) == _capi.ERR_BAD_ARGUMENT
    assert lib.flacenc_hip_decode_pcm(None, out.ctypes.data, 16, 2, 16, 4096, 2, out.ctypes.data, 16,
                                      total.ctypes.data) == _capi.ERR_BAD_ARGUMENT
    assert not out.any() and not total.any()
