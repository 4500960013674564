"""flacenc_hip_encode_streams without a GPU: csrc/stream_encode_core.h -- the renumbered frame and the plan -- as a
stand-alone program under the sanitizers, held to frames the oracle wrote and to a brute-force statement of the plan; the
descriptor's layout in the C header, the numpy dtype and the Rust binding; the exports of the two libraries."""
import functools
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import encode_streams_cases as cases
import encode_streams_model as model
import flac_parse
from flacenc_rs_amd import _capi
from oracle import oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "flacenc_rs_amd", "csrc")
INCLUDE = os.path.join(ROOT, "include")
NUMBERS = (0, 1, 127, 128, 2047, 2048, 65535, 65536, 1 << 21, 1 << 26, (1 << 31) - 1)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("stream_encode_core") / "stream_encode_core_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-static-libasan",
                           "-static-libubsan", "-I", INCLUDE, "-I", CSRC,
                           os.path.join(ROOT, "tests", "host", "stream_encode_core_test.cpp"), "-o", path])
    return path


def run(exe, *args):
    p = subprocess.run([exe, *args], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-2000:]
    return p.stdout


def oracle_frame(channels, block, bps, rate, number, seed):
    """A frame of verbatim subframes (and one constant one) from the oracle's bit writer."""
    rng = np.random.default_rng(seed)
    lo, hi = -(1 << (bps - 1)), (1 << (bps - 1)) - 1
    subs = []
    for c in range(channels):
        if c == 1:
            subs.append(dict(kind=0, bps=bps, samples=np.full(block, -77, np.int32), dc_offset=-77))
        else:
            subs.append(dict(kind=1, bps=bps, samples=rng.integers(lo, hi + 1, block).astype(np.int32)))
    return orc.write_frame(block, 0, bps, rate, number, subs)


# (block size, sample rate): with and without the extra block-size (1 and 2 bytes) and sample-rate (1 and 2 bytes) bytes
SHAPES = ((192, 44100), (4096, 48000), (100, 44100), (1000, 44100), (192, 50000), (192, 12345), (1000, 12345), (100, 12345),
          (1000, 50000), (31, 44100))


def test_a_frame_written_with_number_0_renumbers_to_the_frame_the_oracle_writes_with_that_number(exe, tmp_path):
    records, extra = [], set()
    for channels in range(1, 9):
        for k, (block, rate) in enumerate(SHAPES):
            if block == 4096 and channels > 2:
                continue
            bps = (16, 24, 8)[(channels + k) % 3]
            seed = 100 * channels + k
            f0 = oracle_frame(channels, block, bps, rate, 0, seed)
            p = flac_parse.parse_frame(f0, stream_bps=bps, stream_rate=rate)
            assert p["number"] == 0 and p["length"] == len(f0)
            extra.add(p["header_bits"] // 8 - 6)
            rec = [struct.pack("<I", len(f0)), f0, struct.pack("<I", len(NUMBERS))]
            for number in NUMBERS:
                f = oracle_frame(channels, block, bps, rate, number, seed)
                assert len(f) == len(f0) - 1 + model.coded_number_bytes(number)
                rec += [struct.pack("<II", number, len(f)), f]
            records.append(b"".join(rec))
    assert extra == {0, 1, 2, 3, 4}   # header bytes beyond sync, codes, a 1-byte number and the CRC-8
    path = tmp_path / "vectors.bin"
    path.write_bytes(struct.pack("<I", len(records)) + b"".join(records))
    out = run(exe, "renumber", str(path))
    assert "renumber OK %d" % (len(records) * len(NUMBERS)) in out


def test_the_checks_of_the_table_and_the_frame_counts(exe):
    assert "checks OK" in run(exe, "checks")


def fake_bound(channels, n, bits):
    return 15 + (channels * (8 + n * bits) + 7) // 8 + 2


def brute_plan(table, block, chunk):
    """The plan, stated frame by frame: classes in order of first appearance; launch order = class, then full frames in
    (stream, index) order, then tails in (length, stream) order; runs = maximal stretches of one class and one length,
    cut every `chunk` frames."""
    key_of = lambda d: (int(d["channels"]), int(d["bits_per_sample"]), int(d["bytes_per_sample"]), int(d["sample_rate"]))
    classes = []
    for d in table:
        if key_of(d) not in classes:
            classes.append(key_of(d))
    frames = []   # (class, is tail, length if tail, stream, index) -> sorted = launch order
    first = [0]
    for s, d in enumerate(table):
        total = int(d["total_samples"])
        per = int(d["channels"]) * int(d["bytes_per_sample"])
        nf = -(-total // block)
        for i in range(nf):
            valid = min(block, total - i * block)
            tail = valid < block
            frames.append(((classes.index(key_of(d)), tail, valid if tail else 0, s, i), int(d["offset"]) + i * block * per,
                           valid))
        first.append(first[-1] + nf)
    frames.sort()
    launch = [(off, valid, first[k[3]] + k[4]) for k, off, valid in frames]
    cls = []
    pack_bytes = max_rows = 0
    at = 0
    for c, k in enumerate(classes):
        mine = [f for f in frames if f[0][0] == c]
        full = sum(1 for f in mine if not f[0][1])
        stride = (fake_bound(k[0], block, k[1]) + 15) & ~15
        cls.append(k + (at, full, len(mine) - full, pack_bytes, stride))
        pack_bytes = (pack_bytes + stride * len(mine) + 255) & ~255
        max_rows = max(max_rows, len(mine) * k[0])
        at += len(mine)
    stream = [None] * len(frames)
    for p, (k, _, _) in enumerate(frames):
        c = cls[k[0]]
        stream[first[k[3]] + k[4]] = (c[7] + (p - c[4]) * c[8], p, k[3], k[4])
    runs = []
    p = 0
    while p < len(frames):
        k = frames[p][0]
        e = p
        while e < len(frames) and frames[e][0][:3] == k[:3]:
            e += 1
        for f in range(p, e, chunk):
            runs.append((f, min(chunk, e - f), frames[p][2], k[0]))
        p = e
    full_runs = sum(1 for r in runs if r[2] == block)
    return dict(launch=launch, stream=stream, first=first, classes=cls, runs=runs, full_runs=full_runs,
                tail_runs=len(runs) - full_runs, pack_bytes=pack_bytes, max_rows=max_rows)


def read_plan(buf, at, n_streams):
    def take(fmt):
        nonlocal at
        v = struct.unpack_from("<" + fmt, buf, at)
        at += struct.calcsize("<" + fmt)
        return v
    F, = take("Q")
    launch = [take("QII") for _ in range(F)]
    stream = [take("QIII") for _ in range(F)]
    first = list(take("%dI" % (n_streams + 1)))
    nc, = take("I")
    classes = [take("9Q") for _ in range(nc)]
    nr, = take("I")
    runs = [take("4I") for _ in range(nr)]
    full_runs, tail_runs = take("II")
    pack_bytes, max_rows = take("QQ")
    return dict(launch=launch, stream=stream, first=first, classes=classes, runs=runs, full_runs=full_runs,
                tail_runs=tail_runs, pack_bytes=pack_bytes, max_rows=max_rows), at


def random_tables():
    rng = np.random.default_rng(20)
    tables = []
    kinds = ((1, 16, 2, 44100), (2, 16, 2, 44100), (2, 24, 3, 48000), (3, 16, 4, 12345), (2, 16, 2, 48000), (8, 8, 1, 8000))
    for t in range(60):
        block = int(rng.choice([64, 192, 1152, 4096]))
        chunk = int(rng.choice([1, 2, 3, 7, 768]))
        n = int(rng.integers(0, 14))
        table = np.zeros(n, _capi.PCM_STREAM_DESC_DTYPE)
        at = 0
        for s in range(n):
            ch, bits, width, rate = kinds[int(rng.integers(0, 2 + t % 5))]
            k = int(rng.integers(0, 5))
            # empty streams, exactly k blocks, tails of 1, 63, 64, a tail shared with other streams, any tail
            tail = int(rng.choice([0, 0, 1, 63, 64, 40, int(rng.integers(1, block))]))
            total = 0 if rng.integers(0, 6) == 0 else k * block + (tail if tail < block else 0)
            at += int(rng.integers(0, 5))
            if rng.integers(0, 8) == 0 and s:   # a span repeated
                table[s] = table[s - 1]
                continue
            table[s] = (at, total, 0, 0, ch, bits, width, rate)
            at += total * ch * width
        tables.append((block, chunk, table))
    # every special length in one class, so that tails of 1, 63 and 64 are runs of their own next to a shared one
    b = 192
    lens = [0, b, 3 * b, b + 1, 1, 2 * b + 63, 63, b + 64, 64, b + 40, 5 * b + 40, 40, 0]
    table = np.zeros(len(lens), _capi.PCM_STREAM_DESC_DTYPE)
    for s, total in enumerate(lens):
        table[s] = (7 * s, total, 0, 0, 1, 16, 2, 44100)
    tables.append((b, 2, table))
    return tables


def test_the_plan_equals_brute_force_on_random_tables(exe, tmp_path):
    tables = random_tables()
    blob = [struct.pack("<I", len(tables))]
    for block, chunk, table in tables:
        blob += [struct.pack("<III", block, chunk, len(table)), table.tobytes()]
    src, dst = tmp_path / "tables.bin", tmp_path / "plans.bin"
    src.write_bytes(b"".join(blob))
    assert "plan OK %d" % len(tables) in run(exe, "plan", str(src), str(dst))
    buf, at = dst.read_bytes(), 0
    seen_tail_runs = set()
    for block, chunk, table in tables:
        got, at = read_plan(buf, at, len(table))
        want = brute_plan(table, block, chunk)
        for key in want:
            assert got[key] == want[key], (key, block, chunk)
        assert len(want["launch"]) == _capi.encode_streams_frames(table, block)
        seen_tail_runs.add(want["tail_runs"])
    assert at == len(buf)
    # the last table: tails 1, 63, 64 and 40 (three streams, chunk 2: two runs) -> 5 tail runs, in ascending length
    want = brute_plan(tables[-1][2], 192, 2)
    assert [r[2] for r in want["runs"] if r[2] != 192] == [1, 40, 40, 63, 64] and want["tail_runs"] == 5


def test_the_descriptor_is_48_bytes_with_the_same_fields_everywhere(tmp_path):
    names = list(_capi.PCM_STREAM_DESC_DTYPE.names)
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "flacenc_hip.h"\nint main(void) {\n'
                   '  printf("%zu", sizeof(flacenc_hip_pcm_stream_desc));\n'
                   + "".join('  printf(" %%zu", offsetof(flacenc_hip_pcm_stream_desc, %s));\n' % n for n in names)
                   + "  return 0;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I", INCLUDE, str(src), "-o", exe])
    got = [int(v) for v in subprocess.check_output([exe], text=True).split()]
    assert got == [48, 0, 8, 16, 24, 32, 36, 40, 44]
    dt = _capi.PCM_STREAM_DESC_DTYPE
    assert names == ["offset", "total_samples", "out_offset", "out_capacity", "channels", "bits_per_sample",
                     "bytes_per_sample", "sample_rate"]
    assert dt.itemsize == 48 and [dt.fields[n][1] for n in names] == got[1:]
    assert [dt.fields[n][0].itemsize for n in names] == [8, 8, 8, 8, 4, 4, 4, 4]
    rust = open(os.path.join(ROOT, "rust", "flacenc_hip.rs")).read()
    m = re.search(r"#\[repr\(C\)\]\s*#\[derive\([^)]*\)\]\s*pub struct PcmStreamDesc \{(.*?)\n\}", rust, flags=re.S)
    assert m, "no #[repr(C)] PcmStreamDesc"
    fields = re.findall(r"pub (\w+):\s*(\w+),", m.group(1))
    assert fields == [(n, "u64" if dt.fields[n][0].itemsize == 8 else "u32") for n in names]
    header = open(os.path.join(INCLUDE, "flacenc_hip.h")).read()
    body = re.search(r"struct flacenc_hip_pcm_stream_desc \{(.*?)\};", header, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(\w+)\s+(\w+);", body) == [("uint64_t" if t == "u64" else "uint32_t", n) for n, t in fields]


def test_header_bindings_and_libraries_agree_on_the_exports():
    header = open(os.path.join(INCLUDE, "flacenc_hip.h")).read()
    rust = open(os.path.join(ROOT, "rust", "flacenc_hip.rs")).read()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _capi.LIB_PATH], text=True)
    hooks = subprocess.check_output(["nm", "-D", "--defined-only", _capi.HOOKS_LIB_PATH], text=True)
    for name in ("flacenc_hip_encode_streams", "flacenc_hip_encode_streams_frames"):
        assert re.search(r"\b(int|size_t) %s\s*\(" % name, header)
        assert name in _capi.EXPORTED_SYMBOLS
        assert re.search(r"\bT %s$" % name, out, flags=re.M) and re.search(r"\bT %s$" % name, hooks, flags=re.M)
        assert re.search(r"pub fn %s\(" % name, rust)
    for name in ("flacenc_hip_debug_set_encode_streams_chunk", "flacenc_hip_debug_last_encode_streams_plan"):
        assert name in _capi.DEBUG_SYMBOLS
        assert name not in out and re.search(r"\bT %s$" % name, hooks, flags=re.M)
    assert re.search(r"#define FLACENC_HIP_ENCODE_NO_ROOM 256u", header) and _capi.ENCODE_NO_ROOM == 256
    assert re.search(r"pub const ENCODE_NO_ROOM: u64 = 256;", rust)
    assert "encode_streams(" in open(os.path.join(ROOT, "flacenc_rs_amd", "host", "flacenc.hpp")).read()
    assert _capi.load().flacenc_hip_abi_version() == 6


def test_the_corpus_holds_what_the_gpu_tests_claim():
    for block in (4096, 1152, 192):
        s = cases.mixed(block)
        assert {x.channels for x in s} == {1, 2, 3}
        assert {(x.bps, x.width) for x in s} == {(16, 2), (24, 3), (16, 4)}
        assert {x.rate for x in s} == {44100, 48000, 12345}
        totals = [x.x.shape[1] for x in s]
        for want in (0, 2 * block, block + 1, block + 63, block + 64, 3 * block + 1000):
            assert want in totals
        lay = cases.layout(s, block)
        assert all(off % 2 == 1 for off, _ in lay.spans) and lay.spans[-1][0] + lay.spans[-1][1] == lay.pcm.size
        for (off, n), x in zip(lay.spans, s):
            assert np.array_equal(lay.pcm[off:off + n], cases.pack(x.x, x.width))
        m = cases.slot_map(lay.table, lay.out_bytes)
        assert not m.all() and int(m.sum()) == int(lay.table["out_capacity"].sum())   # disjoint, fill between them
        # the model's frames parse back to the stream's samples, numbered from 0 (one short stream per block size)
        cfg, mod = model.configs(8)
        x = s[2]
        fr = model.frames(mod, x, block)
        assert len(fr) == 2
        for i, f in enumerate(fr):
            p = flac_parse.parse_frame(f, stream_bps=x.bps, stream_rate=x.rate)
            assert p["number"] == i and np.array_equal(p["channels"], x.x[:, i * block:(i + 1) * block])
    assert model.cut([10, 20, 30], 29) == (1, 10) and model.cut([10, 20, 30], 30) == (2, 30)
    assert model.cut([10, 20, 30], 9) == (0, 0) and model.cut([], 5) == (0, 0) and model.cut([10], 0) == (0, 0)
    assert model.totals([10, 20, 30], 59, 7) == [2, 30, 7, 256] and model.totals([10, 20, 30], 60, 7) == [3, 60, 7, 0]
