"""The block-size search's core (flacenc_rs_amd/csrc/variable_block_core.h) built by g++ for the host, also under
ASan + UBSan, and the library's bound functions.  No GPU."""
import shutil
import subprocess

import numpy as np
import pytest

import flac_parse
import vbs_model
from flacenc_rs_amd import _capi, variable_cpu

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


@pytest.fixture(scope="module")
def core():
    return variable_cpu.VariableCore(variable_cpu.build())


def fixed_header(number, bs_code=12, sr_code=9, ch_code=1, ss_code=4, extra=b""):
    """A fixed-blocking header as the frame packer writes it (sync 0xFFF8, coded frame number, CRC-8)."""
    h = bytes([0xFF, 0xF8, (bs_code << 4) | sr_code, (ch_code << 4) | (ss_code << 1)]) + vbs_model.coded_number(number)
    h += extra
    return h + bytes([flac_parse.crc8(h)])


def test_core_self_check_under_sanitizers(tmp_path):
    exe = variable_cpu.build_sanitized_driver(str(tmp_path))
    p = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "0 failures" in p.stdout


@pytest.mark.parametrize("k", range(37))
def test_coded_number_round_trips_through_the_decoder_core(core, k):
    for v in (v for v in ((1 << k) - 1, 1 << k, (1 << k) + 1) if 0 <= v < 1 << 36):
        assert core.coded_number(v) == vbs_model.coded_number(v)
        fixed = fixed_header(k)
        var = core.variable_header(fixed, v)
        assert len(var) == len(fixed) - len(vbs_model.coded_number(k)) + len(vbs_model.coded_number(v))
        st, h = core.parse_header(var, 2, 16)
        assert st == 0, (v, st)
        assert h["variable"] == 1 and h["number"] == v and h["header_bytes"] == len(var) and h["block_size"] == 4096
        # and the test-side parser agrees on every field
        assert var[:2] == b"\xff\xf9" and flac_parse.crc8(var[:-1]) == var[-1]


@pytest.mark.parametrize("bs_code,sr_code,extra", [(12, 9, b""), (6, 12, b"\x7f\x30"), (7, 13, b"\x10\x00\xac\x44"),
                                                   (7, 14, b"\x08\xff\x11\x22"), (1, 0, b"")])
def test_header_rewrite_keeps_every_code_and_extra_byte(core, bs_code, sr_code, extra):
    for number in (0, 127, 128, 5000, (1 << 31) - 1):
        fixed = fixed_header(number, bs_code, sr_code, extra=extra)
        assert core.header_bytes(fixed) == len(fixed)
        for sample in (0, 4096, 1 << 30, (1 << 36) - 1):
            var = core.variable_header(fixed, sample)
            code = vbs_model.coded_number(sample)
            assert var == bytes([0xFF, 0xF9]) + fixed[2:4] + code + extra + bytes([flac_parse.crc8(
                bytes([0xFF, 0xF9]) + fixed[2:4] + code + extra)])


def test_crc16_combine_equals_a_direct_crc(core):
    rng = np.random.default_rng(0xC0C0)
    lengths = [0, 1, 2, 3, 7, 64, 4095, 16384, 65537, 1 << 20] + [int(x) for x in rng.integers(0, 200000, 20)]
    for i, n in enumerate(lengths):
        body = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        number = int(rng.integers(0, 1 << 31))
        bs_code, sr_code, extra = ((12, 9, b""), (7, 12, b"\x01\x02\x2c"))[i % 2]
        fixed = fixed_header(number, bs_code, sr_code, extra=extra)
        sample = int(rng.integers(0, 1 << 36)) >> int(rng.integers(0, 36))
        var = core.variable_header(fixed, sample)
        old = core.crc16(fixed + body)
        got = core.crc16_rehead(old, core.crc16(fixed), core.crc16(var), n)
        assert got == core.crc16(var + body), (n, sample)
        if n <= 4096:  # the table CRC against the test-side bitwise one
            assert core.crc16(var + body) == flac_parse.crc16(var + body)


@pytest.mark.parametrize("levels", [1, 2, 3, 4, 5])
def test_tree_minimum_equals_the_python_statement(core, levels):
    rng = np.random.default_rng(levels)
    for trial in range(400):
        spread = 3 if trial % 2 else 4000  # small spreads: many ties
        lens = [0] + [int(100 * (levels - vbs_model.node_level(n)) + rng.integers(0, spread))
                      for n in range(1, 1 << levels)]
        best, mask, frames = core.tree_min(lens, levels)
        want_best, want_mask, leaves = vbs_model.tree_min(lens, levels)
        assert (best, mask, frames) == (want_best, want_mask, len(leaves))
        assert [core.tiling_node(mask, levels, t) for t in range(frames)] == leaves
        assert core.tiling_node(mask, levels, frames) == 0


def test_ties_keep_the_larger_block(core):
    # children summing exactly to the parent: not split
    best, mask, frames = core.tree_min([0, 100, 50, 50], 2)
    assert (best, mask, frames) == (100, 0, 1)
    best, mask, frames = core.tree_min([0, 100, 50, 49], 2)
    assert (best, mask, frames) == (99, 1, 2)


@pytest.mark.parametrize("channels,bps", [(1, 16), (2, 16), (2, 24), (3, 24), (8, 16)])
def test_bounds_follow_their_formulas(channels, bps):
    for block_size, levels in ((4096, 1), (4096, 4), (4608, 2), (2048, 3), (8192, 5), (256, 1)):
        for total in (0, 1, block_size - 1, block_size, 10 * block_size + 777, 123 * block_size):
            assert _capi.variable_bytes_bound(channels, block_size, levels, bps, total) == \
                vbs_model.variable_bytes_bound(channels, block_size, levels, bps, total)
            assert _capi.variable_max_frames(block_size, levels, total) == \
                vbs_model.variable_max_frames(block_size, levels, total)


def test_bounds_reject_what_the_encoder_rejects():
    assert _capi.variable_max_frames(4096, 0, 4096) == 0
    assert _capi.variable_max_frames(4096, 6, 4096) == 0
    assert _capi.variable_max_frames(4098, 3, 4098) == 0  # not divisible by 4
    assert _capi.variable_max_frames(2048, 5, 2048) == 0  # 128-sample leaves
    assert _capi.variable_max_frames(32768, 1, 32768) == 0  # above the largest block
    assert _capi.variable_bytes_bound(9, 4096, 1, 16, 4096) == 0
    assert _capi.variable_bytes_bound(2, 4096, 1, 7, 4096) == 0
    assert _capi.variable_max_frames(4096, 5, 4096 * 3 + 5) == 3 * 16 + 1
