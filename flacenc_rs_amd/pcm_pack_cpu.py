"""The host build of flacenc_hip_pack_le_bytes' index arithmetic (csrc/pcm_pack_core.h via csrc/pcm_pack_cpu.cpp),
compiled with g++ on demand for the CPU tests: the same walk over frames, slices and lanes as the device kernel of
csrc/pcm_pack.cpp, plus a self-checking driver built under ASan + UBSan."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
_SOURCES = ("pcm_pack_cpu.cpp", "pcm_pack_core.h")


def _newest():
    return max(os.path.getmtime(os.path.join(CSRC, s)) for s in _SOURCES)


def build(out_dir: str | None = None) -> str:
    out_dir = out_dir or os.path.join(CSRC, "build", "cpu")
    os.makedirs(out_dir, exist_ok=True)
    lib = os.path.join(out_dir, "libpcm_pack_cpu.so")
    if not os.path.exists(lib) or os.path.getmtime(lib) < _newest():
        subprocess.check_call(["g++", "-std=c++17", "-shared", "-fPIC", "-O2", "-Wall", "-Wextra",
                               os.path.join(CSRC, "pcm_pack_cpu.cpp"), "-o", lib + ".tmp"])
        os.replace(lib + ".tmp", lib)
    return lib


def build_sanitized_driver(out_dir: str | None = None) -> str:
    """The self-check of pcm_pack_cpu.cpp (PPK_MAIN) under ASan + UBSan, runtimes linked statically: a stand-alone
    program, nothing of it is loaded into Python."""
    out_dir = out_dir or os.path.join(CSRC, "build", "cpu")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "ppk_san")
    if not os.path.exists(exe) or os.path.getmtime(exe) < _newest():
        subprocess.check_call(["g++", "-std=c++17", "-DPPK_MAIN", "-O1", "-g", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-static-libasan",
                               "-static-libubsan", os.path.join(CSRC, "pcm_pack_cpu.cpp"), "-o", exe + ".tmp"])
        os.replace(exe + ".tmp", exe)
    return exe


class PackCore:
    """ctypes view of the host build."""

    def __init__(self, path: str | None = None):
        L = C.CDLL(path or build())
        vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
        L.ppk_pack.argtypes = [vp, u64, vp, u64, u32, u32, vp, u64, u64, vp, vp, vp]
        L.ppk_pack.restype = C.c_int
        L.ppk_div_check.argtypes = [u32]
        L.ppk_div_check.restype = C.c_int64
        L.ppk_slice.restype = u32
        L.ppk_split.argtypes = [u32, u32, vp]
        L.ppk_split.restype = None
        self._L = L
        self.slice = int(L.ppk_slice())

    def pack(self, frames, block_sizes, channels: int, bytes_per_sample: int, out_capacity: int | None = None,
             out_addr: int = 0, fill: int = 0xEE):
        """frames int32 [n_frames, channels, stride] -> dict(rc, out (uint8, `fill` where nothing was stored), offsets,
        total, hits (stores per output byte)); out_capacity defaults to exactly what the block sizes need."""
        x = np.ascontiguousarray(frames, np.int32)
        n, ch, stride = x.shape
        assert ch == channels
        bs = np.ascontiguousarray(block_sizes, np.uint32)
        assert bs.shape == (n,)
        need = int(np.minimum(bs.astype(np.uint64), stride).sum()) * channels * bytes_per_sample
        cap = need if out_capacity is None else out_capacity
        out = np.full(max(cap, 1), fill, np.uint8)
        hits = np.zeros(max(cap, 1), np.uint8)
        off = np.zeros(n + 1, np.uint64)
        total = np.zeros(1, np.uint64)
        rc = self._L.ppk_pack(x.ctypes.data, stride, bs.ctypes.data, n, channels, bytes_per_sample, out.ctypes.data, cap,
                              out_addr, off.ctypes.data, total.ctypes.data, hits.ctypes.data)
        return dict(rc=rc, out=out[:cap], offsets=off, total=int(total[0]), hits=hits[:cap])

    def div_check(self, channels: int) -> int:
        return int(self._L.ppk_div_check(channels))

    def split(self, low2: int, length: int):
        out = np.zeros(3, np.uint32)
        self._L.ppk_split(low2, length, out.ctypes.data)
        return tuple(int(v) for v in out)
