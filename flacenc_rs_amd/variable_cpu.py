"""The host build of the block-size search's core (csrc/variable_block_core.h via csrc/variable_block_cpu.cpp), compiled
with g++ on demand for the CPU tests: the coded number, the header rewrite, the CRC-16 combine and the tree minimum that
the device kernels of csrc/variable_block.cpp run, plus a self-checking driver built under ASan + UBSan."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
_SOURCES = ("variable_block_cpu.cpp", "variable_block_core.h", "flac_decode_core.h")


def _newest():
    return max(os.path.getmtime(os.path.join(CSRC, s)) for s in _SOURCES)


def build(out_dir: str | None = None) -> str:
    out_dir = out_dir or os.path.join(CSRC, "build", "cpu")
    os.makedirs(out_dir, exist_ok=True)
    lib = os.path.join(out_dir, "libvariable_block_cpu.so")
    if not os.path.exists(lib) or os.path.getmtime(lib) < _newest():
        subprocess.check_call(["g++", "-std=c++17", "-shared", "-fPIC", "-O2", "-Wall", "-Wextra",
                               os.path.join(CSRC, "variable_block_cpu.cpp"), "-o", lib + ".tmp"])
        os.replace(lib + ".tmp", lib)
    return lib


def build_sanitized_driver(out_dir: str | None = None) -> str:
    """The self-check of variable_block_cpu.cpp (VBS_MAIN) under ASan + UBSan, runtimes linked statically."""
    out_dir = out_dir or os.path.join(CSRC, "build", "cpu")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "vbs_san")
    if not os.path.exists(exe) or os.path.getmtime(exe) < _newest():
        subprocess.check_call(["g++", "-std=c++17", "-DVBS_MAIN", "-O1", "-g", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-static-libasan",
                               "-static-libubsan", os.path.join(CSRC, "variable_block_cpu.cpp"), "-o", exe + ".tmp"])
        os.replace(exe + ".tmp", exe)
    return exe


class VariableCore:
    """ctypes view of the host build."""

    def __init__(self, path: str):
        L = C.CDLL(path)
        vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
        for name, args, res in (
                ("vbs_coded_number_bytes", [u64], u32),
                ("vbs_write_coded_number", [vp, u64], u32),
                ("vbs_header_bytes", [vp], u32),
                ("vbs_write_variable_header", [vp, u64, vp], u32),
                ("vbs_crc16", [vp, u64], u32),
                ("vbs_crc16_rehead", [u32, u32, u32, u64], u32),
                ("vbs_tree_min", [vp, u32, vp, vp], u64),
                ("vbs_tiling_node", [u32, u32, u32], u32),
                ("vbs_parse_header", [vp, u32, u32, u32, vp, vp], u32)):
            getattr(L, name).argtypes = args
            getattr(L, name).restype = res
        self._L = L

    def coded_number(self, v: int) -> bytes:
        buf = (C.c_uint8 * 8)()
        n = self._L.vbs_write_coded_number(buf, v)
        assert n == self._L.vbs_coded_number_bytes(v)
        return bytes(buf[:n])

    def header_bytes(self, header: bytes) -> int:
        buf = (C.c_uint8 * 16).from_buffer_copy(bytes(header[:16]).ljust(16, b"\0"))
        return int(self._L.vbs_header_bytes(buf))

    def variable_header(self, fixed_header: bytes, sample_number: int) -> bytes:
        src = (C.c_uint8 * 16).from_buffer_copy(bytes(fixed_header[:16]).ljust(16, b"\0"))
        out = (C.c_uint8 * 16)()
        n = self._L.vbs_write_variable_header(src, sample_number, out)
        return bytes(out[:n])

    def crc16(self, data: bytes) -> int:
        b = np.frombuffer(bytes(data), np.uint8)
        return int(self._L.vbs_crc16(b.ctypes.data if b.size else None, b.size))

    def crc16_rehead(self, crc_old: int, crc_h: int, crc_h_new: int, body_bytes: int) -> int:
        return int(self._L.vbs_crc16_rehead(crc_old, crc_h, crc_h_new, body_bytes))

    def tree_min(self, lens, levels: int):
        """lens[n] for heap nodes n = 1 .. 2^levels - 1 (lens[0] unused) -> (best, mask, frames)."""
        arr = np.zeros(32, np.uint32)
        arr[:len(lens)] = lens
        mask, frames = C.c_uint32(0), C.c_uint32(0)
        best = self._L.vbs_tree_min(arr.ctypes.data, levels, C.byref(mask), C.byref(frames))
        return int(best), mask.value, frames.value

    def tiling_node(self, mask: int, levels: int, t: int) -> int:
        return int(self._L.vbs_tiling_node(mask, levels, t))

    def parse_header(self, data: bytes, channels: int, bits_per_sample: int):
        """flacdec::parse_header -> (status, dict(block_size, channels, bps, header_bytes, variable, number))."""
        b = np.frombuffer(bytes(data), np.uint8).copy()
        out = np.zeros(5, np.uint32)
        num = C.c_uint64(0)
        st = self._L.vbs_parse_header(b.ctypes.data, b.size, channels, bits_per_sample, out.ctypes.data, C.byref(num))
        keys = ("block_size", "channels", "bps", "header_bytes", "variable")
        return int(st), dict(zip(keys, (int(v) for v in out)), number=num.value)
