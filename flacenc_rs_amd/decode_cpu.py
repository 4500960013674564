"""The host build of the frame decoder's core (csrc/flac_decode_core.h via csrc/flac_decode_cpu.cpp), compiled with g++
on demand: the CPU tests check the core with it (also under the address / undefined-behaviour sanitizers) and
tools/time_decode.py times it as the multi-threaded CPU baseline.  Same arguments and outputs as the device calls."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
_SOURCES = ("flac_decode_cpu.cpp", "flac_decode_core.h")

DECODE_BAD_HEADER, DECODE_HEADER_CRC, DECODE_FRAME_CRC, DECODE_PARSE = 1, 2, 4, 8
DECODE_LENGTH, DECODE_STREAM_MISMATCH, DECODE_UNSUPPORTED, DECODE_MISMATCH = 16, 32, 64, 128


def build(sanitize: bool = False, out_dir: str | None = None) -> str:
    out_dir = out_dir or os.path.join(CSRC, "build", "cpu")
    os.makedirs(out_dir, exist_ok=True)
    lib = os.path.join(out_dir, "libflac_decode_cpu_san.so" if sanitize else "libflac_decode_cpu.so")
    newest = max(os.path.getmtime(os.path.join(CSRC, s)) for s in _SOURCES)
    if not os.path.exists(lib) or os.path.getmtime(lib) < newest:
        flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                 "-fno-omit-frame-pointer"] if sanitize else ["-O2"]
        subprocess.check_call(["g++", "-std=c++17", "-shared", "-fPIC", "-pthread", "-Wall", "-Wextra", *flags,
                               os.path.join(CSRC, "flac_decode_cpu.cpp"), "-o", lib + ".tmp"])
        os.replace(lib + ".tmp", lib)
    return lib


def build_sanitized_driver(out_dir: str | None = None) -> str:
    """The stand-alone driver of flac_decode_cpu.cpp (FDC_MAIN) under ASan + UBSan; the runtime is linked statically
    so the executable needs nothing in front of it."""
    out_dir = out_dir or os.path.join(CSRC, "build", "cpu")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "fdc_san")
    newest = max(os.path.getmtime(os.path.join(CSRC, s)) for s in _SOURCES)
    if not os.path.exists(exe) or os.path.getmtime(exe) < newest:
        subprocess.check_call(["g++", "-std=c++17", "-DFDC_MAIN", "-O1", "-g", "-pthread", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-static-libasan",
                               "-static-libubsan", os.path.join(CSRC, "flac_decode_cpu.cpp"), "-o", exe + ".tmp"])
        os.replace(exe + ".tmp", exe)
    return exe


def run_sanitized(exe: str, data: bytes, offsets, lengths, channels: int, bits_per_sample: int, max_block_size: int,
                  work_dir: str, max_bits_per_sample: int = 0):
    """-> (status, block_sizes, samples, index offsets, index ok, the driver's stderr); raises on any report.
    max_bits_per_sample: the depth limit the driver decodes under, 0 (= 24), 24 or 32."""
    off = np.ascontiguousarray(offsets, np.uint64)
    ln = np.ascontiguousarray(lengths, np.uint32)
    n = len(off)
    src, dst = os.path.join(work_dir, "corpus.bin"), os.path.join(work_dir, "result.bin")
    with open(src, "wb") as f:
        f.write(np.array([n], np.uint64).tobytes() + np.array([channels, bits_per_sample, max_block_size, max_bits_per_sample],
                                                                np.uint32).tobytes())
        f.write(np.array([len(data)], np.uint64).tobytes() + off.tobytes() + ln.tobytes() + bytes(data))
    p = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=600)
    if p.returncode != 0 or "runtime error" in p.stderr or "AddressSanitizer" in p.stderr:
        raise AssertionError(f"sanitized driver: exit {p.returncode}\n{p.stderr[-4000:]}")
    raw = open(dst, "rb").read()
    st = np.frombuffer(raw, np.uint32, n, 0)
    bs = np.frombuffer(raw, np.uint32, n, 4 * n)
    k = n * channels * max_block_size
    samples = np.frombuffer(raw, np.int32, k, 8 * n).reshape(n, channels, max_block_size)
    at = 8 * n + 4 * k
    found = int(np.frombuffer(raw, np.uint64, 1, at)[0])
    ok = bool(np.frombuffer(raw, np.uint32, 1, at + 8)[0])
    ioff = np.frombuffer(raw, np.uint64, found, at + 12)
    return st, bs, samples, ioff, ok, p.stderr


class DecoderCpu:
    def __init__(self, path: str):
        L = C.CDLL(path)
        vp = C.c_void_p
        L.fdc_decode_frames.argtypes = [vp, vp, vp, C.c_size_t, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp,
                                        C.c_size_t, vp, vp, vp, C.c_int]
        L.fdc_decode_frames.restype = C.c_int
        L.fdc_index_frames.argtypes = [vp, C.c_uint64, C.c_uint32, C.c_uint32, C.c_size_t, vp, vp, vp]
        L.fdc_index_frames.restype = C.c_int
        # the same two with the depth limit (flacenc_hip_set_max_bits_per_sample) behind the other arguments
        L.fdc_decode_frames_depth.argtypes = L.fdc_decode_frames.argtypes + [C.c_uint32]
        L.fdc_decode_frames_depth.restype = C.c_int
        L.fdc_index_frames_depth.argtypes = L.fdc_index_frames.argtypes + [C.c_uint32]
        L.fdc_index_frames_depth.restype = C.c_int
        self._lib = L

    def _decode(self, max_bits_per_sample, *args):
        if max_bits_per_sample is None:
            rc = self._lib.fdc_decode_frames(*args)
            assert rc == 0, rc
            return
        rc = self._lib.fdc_decode_frames_depth(*args, max_bits_per_sample)
        if rc != 0:
            raise ValueError(rc)

    def decode_frames(self, data, offsets, lengths, channels: int, bits_per_sample: int, max_block_size: int,
                      threads: int = 1, expected: np.ndarray | None = None, max_bits_per_sample: int | None = None):
        """-> (samples int32 [n, channels, max_block_size], block_sizes, numbers, status); with `expected` (same
        shape) it verifies instead and the samples are None.  max_bits_per_sample: None for fdc_decode_frames (24
        bits, as it always was), else fdc_decode_frames_depth with that limit, where a refused call raises ValueError."""
        buf = np.frombuffer(bytes(data), np.uint8) if not isinstance(data, np.ndarray) else data
        buf = np.ascontiguousarray(buf, np.uint8)
        off = np.ascontiguousarray(offsets, np.uint64)
        ln = np.ascontiguousarray(lengths, np.uint32)
        n = len(off)
        st = np.zeros(n, np.uint32)
        if expected is not None:
            exp = np.ascontiguousarray(expected, np.int32)
            self._decode(max_bits_per_sample, buf.ctypes.data, off.ctypes.data, ln.ctypes.data, n, channels,
                         bits_per_sample, max_block_size, None, exp.ctypes.data, exp.shape[-1], None, None,
                         st.ctypes.data, threads)
            return None, None, None, st
        out = np.full((n, channels, max_block_size), -1, np.int32)
        bs = np.zeros(n, np.uint32)
        num = np.zeros(n, np.uint64)
        self._decode(max_bits_per_sample, buf.ctypes.data, off.ctypes.data, ln.ctypes.data, n, channels,
                     bits_per_sample, max_block_size, out.ctypes.data, None, max_block_size, bs.ctypes.data,
                     num.ctypes.data, st.ctypes.data, threads)
        return out, bs, num, st

    def index_frames(self, data, channels: int, bits_per_sample: int, max_frames: int,
                     max_bits_per_sample: int | None = None):
        """-> (offsets, lengths, ok); max_bits_per_sample as in decode_frames"""
        buf = np.ascontiguousarray(np.frombuffer(bytes(data), np.uint8) if not isinstance(data, np.ndarray) else data,
                                   np.uint8)
        off = np.zeros(max(1, max_frames), np.uint64)
        ln = np.zeros(max(1, max_frames), np.uint32)
        nf = C.c_uint64(0)
        args = (buf.ctypes.data, buf.size, channels, bits_per_sample, max_frames, off.ctypes.data, ln.ctypes.data,
                C.byref(nf))
        rc = (self._lib.fdc_index_frames(*args) if max_bits_per_sample is None
              else self._lib.fdc_index_frames_depth(*args, max_bits_per_sample))
        return off[: nf.value], ln[: nf.value], rc == 0
