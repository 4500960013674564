"""The frame decoder's core (flacenc_rs_amd/csrc/flac_decode_core.h) built by g++ for the host: oracle-written frames,
frames only the test-side writer makes, a seeded mutation corpus under ASan + UBSan, and indexing.  No GPU."""
import os
import shutil

import numpy as np
import pytest

import flac_parse
import flac_write as fw
from flacenc_rs_amd import decode_cpu
from oracle import oracle as orc

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


@pytest.fixture(scope="module")
def dec():
    return decode_cpu.DecoderCpu(decode_cpu.build())


def signal(rng, n, bps, kind="smooth"):
    lo, hi = -(1 << (bps - 1)), (1 << (bps - 1)) - 1
    if kind == "noise":
        return rng.integers(lo, hi + 1, n).astype(np.int64)
    t = np.arange(n)
    x = 0.6 * np.sin(2 * np.pi * t / rng.uniform(20, 200)) + 0.05 * rng.standard_normal(n)
    return np.clip(np.round(x * hi), lo, hi).astype(np.int64)


def lpc_coefs(rng, order, precision):
    """Small stable-ish integer predictor: a decaying first coefficient, the rest small."""
    shift = min(precision - 1, 12)
    c = np.zeros(order, np.int64)
    c[0] = int(0.9 * (1 << shift)) if precision > 1 else 0
    lim = (1 << (precision - 1)) - 1
    c[0] = min(c[0], lim)
    if order > 1:
        c[1:] = rng.integers(-max(1, lim // 64), max(1, lim // 64) + 1, order - 1)
    return np.clip(c, -lim - 1, lim), shift


def rice_params(e, order, n, rice_order, limit=30):
    psize = n >> rice_order
    out, t = [], order
    for q in range(1 << rice_order):
        cnt = psize - (order if q == 0 else 0)
        out.append(min(limit, fw.best_param(e[t:t + cnt], 1)))
        t += cnt
    return np.array(out, np.uint8)


def oracle_subframe(x, bps, kind, rng, order=0, precision=15, rice_order=0):
    """-> the oracle's write_frame description of x coded as `kind`."""
    x = np.asarray(x, np.int64)
    n = len(x)
    if kind == orc.KIND_CONSTANT:
        return dict(kind=kind, bps=bps, dc_offset=int(x[0]))
    if kind == orc.KIND_VERBATIM:
        return dict(kind=kind, bps=bps, samples=x)
    if kind == orc.KIND_FIXED:
        coefs, shift = fw.FIXED_COEFS[order], 0
    else:
        coefs, shift = lpc_coefs(rng, order, precision)
    e = fw.residuals(x, coefs, shift, order)
    d = dict(kind=kind, bps=bps, samples=x, order=order, rice_order=rice_order,
             rice_params=rice_params(e, order, n, rice_order), residual=e)
    if kind == orc.KIND_LPC:
        d.update(shift=shift, precision=precision, coefs=np.array(coefs, np.int16))
    return d


def coded_channels(x, assignment):
    if assignment == 1:
        return [x[0], x[0] - x[1]]
    if assignment == 2:
        return [x[0] - x[1], x[1]]
    if assignment == 3:
        return [(x[0] + x[1]) >> 1, x[0] - x[1]]
    return list(x)


def side_index(assignment):
    return {1: 1, 2: 0, 3: 1}.get(assignment, -1)


def oracle_corpus():
    """(frame bytes, channels, bps, samples [nch, n]) over the shapes the oracle's writer covers."""
    rng = np.random.default_rng(0xDEC0DE)
    out = []
    n = 1152
    for kind in (orc.KIND_CONSTANT, orc.KIND_VERBATIM):
        x = np.full((1, n), 123, np.int64) if kind == orc.KIND_CONSTANT else signal(rng, n, 16, "noise")[None]
        out.append((orc.write_frame(n, 0, 16, 44100, 1, [oracle_subframe(x[0], 16, kind, rng)]), 1, 16, x))
    for order in range(5):
        for method_order in (0, 3, 8):
            nn = 4096
            x = signal(rng, nn, 16)[None]
            sf = oracle_subframe(x[0], 16, orc.KIND_FIXED, rng, order=order, rice_order=method_order)
            out.append((orc.write_frame(nn, 0, 16, 44100, order, [sf]), 1, 16, x))
    for order in (1, 2, 7, 8, 12, 16, 24, 31, 32):
        for precision in (1, 5, 12, 15):
            x = signal(rng, 2048, 16)[None]
            sf = oracle_subframe(x[0], 16, orc.KIND_LPC, rng, order=order, precision=precision, rice_order=2)
            out.append((orc.write_frame(2048, 0, 16, 44100, 7, [sf]), 1, 16, x))
    for bps in (8, 12, 16, 20, 24):
        for assignment in range(4):
            x = np.stack([signal(rng, 4096, bps), signal(rng, 4096, bps)])
            coded = coded_channels(x, assignment)
            side = side_index(assignment)
            sfs = [oracle_subframe(coded[c], bps + (c == side), orc.KIND_LPC if c == 0 else orc.KIND_FIXED, rng,
                                   order=8 if c == 0 else 2, rice_order=4) for c in range(2)]
            out.append((orc.write_frame(4096, assignment, bps, 48000, 3, sfs), 2, bps, x))
    for nch in range(1, 9):
        x = np.stack([signal(rng, 576, 16) for _ in range(nch)])
        sfs = [oracle_subframe(x[c], 16, (orc.KIND_VERBATIM, orc.KIND_FIXED, orc.KIND_LPC)[c % 3], rng, order=3)
               for c in range(nch)]
        out.append((orc.write_frame(576, 0, 16, 44100, 9, sfs), nch, 16, x))
    # every block-size code the oracle's header writer picks, a ragged last frame among them
    for n in (192, 576, 1152, 2304, 4608, 256, 512, 1024, 2048, 4096, 8192, 16384, 32768, 100, 1000, 4095, 1):
        x = signal(rng, n, 16)[None]
        kind = orc.KIND_VERBATIM if n < 8 else orc.KIND_FIXED
        out.append((orc.write_frame(n, 0, 16, 44100, 5, [oracle_subframe(x[0], 16, kind, rng, order=2)]), 1, 16, x))
    return out


def decode_one(dec, data, nch, bps, maxbs=32768):
    out, bs, num, st = dec.decode_frames(data, [0], [len(data)], nch, bps, maxbs)
    return out[0], int(bs[0]), int(num[0]), int(st[0])


def test_oracle_written_frames_decode_to_their_samples(dec):
    corpus = oracle_corpus()
    assert len(corpus) > 80
    for data, nch, bps, x in corpus:
        out, bs, _, st = decode_one(dec, data, nch, bps)
        n = x.shape[1]
        assert st == 0 and bs == n
        assert np.array_equal(out[:, :n], x), (nch, bps, n)
        assert not out[:, n:].any()
        ref = flac_parse.parse_frame(data, stream_bps=bps)
        assert np.array_equal(ref["channels"], x) and ref["length"] == len(data)


def crafted_corpus():
    """Frames the oracle cannot write: (bytes, channels, bps, samples, number)."""
    rng = np.random.default_rng(0xC0FFEE)
    out = []
    # wasted bits on every kind
    for kind, extra in (("constant", {}), ("verbatim", {}), ("fixed", dict(order=2)),
                        ("lpc", dict(order=4, coefs=[3, -3, 1, 0], precision=4, shift=0))):
        for wasted in (1, 3, 7):
            x = (signal(rng, 1024, 16 - wasted) << wasted)[None] if kind != "constant" else np.full((1, 1024), -8 << wasted)
            out.append((fw.frame(x, 0, 16, [dict(kind=kind, wasted=wasted, **extra)]), 1, 16, x, 0))
    # escaped partitions: width 0 (all-zero residual) and widths above 0, both methods
    x0 = np.full((1, 4096), 5, np.int64)
    out.append((fw.frame(x0, 0, 16, [dict(kind="fixed", order=1, porder=2, params=[("esc", 0)] * 4)]), 1, 16, x0, 0))
    for method in (0, 1):
        x = signal(rng, 4096, 16, "noise")[None]
        params = [("esc", 18), 14 + method * 10, ("esc", 31), 3]
        out.append((fw.frame(x, 0, 16, [dict(kind="fixed", order=1, method=method, porder=2, params=params)], number=1), 1,
                    16, x, 1))
    # RICE2 parameters 15..30
    for p in range(15, 31):
        x = signal(rng, 512, 24, "noise")[None]
        out.append((fw.frame(x, 0, 24, [dict(kind="fixed", order=0, method=1, params=[p])], number=p), 1, 24, x, p))
    # variable blocking with multi-byte sample numbers; 8-bit / 16-bit block-size codes; sample-rate codes 12..14
    for i, number in enumerate((0, 0x7F, 0x80, 0x7FF, 0x800, 0xFFFF, 0x1FFFFF, 0x3FFFFFF, 0x7FFFFFFF, 0xFFFFFFFFF)):
        n = (17, 256, 300, 4097, 1, 65, 4096, 1152, 999, 8191)[i]
        x = signal(rng, n, 16)[None]
        sr = (12, 13, 14, 0, 9)[i % 5]
        sf = dict(kind="verbatim") if n < 4 else dict(kind="lpc", order=3, coefs=[2, -1, 0], precision=3, shift=0)
        out.append((fw.frame(x, 0, 16, [sf], number=number, variable=True, sr_code=sr, sr_value=44), 1, 16, x, number))
    # sample-size code 0 (the stream's bit depth), every block-size code 1..15
    for code, n in ((1, 192), (2, 576), (3, 1152), (4, 2304), (5, 4608), (6, 7), (7, 300), (8, 256), (9, 512),
                    (10, 1024), (11, 2048), (12, 4096), (13, 8192), (14, 16384), (15, 32768)):
        x = np.stack([signal(rng, n, 20), signal(rng, n, 20)])
        sfs = [dict(kind="fixed", order=min(3, n)), dict(kind="fixed", order=min(1, n), method=1)]
        out.append((fw.frame(x, 10, 20, sfs, number=code, bs_code=code, ss_code=0), 2, 20, x, code))
    return out


def test_crafted_frames_decode_to_their_inputs(dec):
    for data, nch, bps, x, number in crafted_corpus():
        out, bs, num, st = decode_one(dec, data, nch, bps)
        n = x.shape[1]
        assert (st, bs, num) == (0, n, number)
        assert np.array_equal(out[:, :n], x)


def test_header_checks(dec):
    rng = np.random.default_rng(3)
    x = signal(rng, 1024, 16)[None]
    good = fw.frame(x, 0, 16, [dict(kind="fixed", order=2)])
    assert decode_one(dec, good, 1, 16)[3] == 0
    assert decode_one(dec, good, 2, 16)[3] == decode_cpu.DECODE_STREAM_MISMATCH
    assert decode_one(dec, good, 1, 20)[3] == decode_cpu.DECODE_STREAM_MISMATCH
    assert decode_one(dec, good, 1, 16, maxbs=1023)[3] == decode_cpu.DECODE_UNSUPPORTED
    assert decode_one(dec, good + b"\0", 1, 16)[3] == decode_cpu.DECODE_LENGTH
    assert decode_one(dec, b"\0" + good[1:], 1, 16)[3] == decode_cpu.DECODE_BAD_HEADER
    bad = bytearray(good)
    bad[5] ^= 0xFF  # the CRC-8
    assert decode_one(dec, bytes(bad), 1, 16)[3] == decode_cpu.DECODE_HEADER_CRC
    bad = bytearray(good)
    bad[-1] ^= 1
    out, bs, _, st = decode_one(dec, bytes(bad), 1, 16)
    assert st == decode_cpu.DECODE_FRAME_CRC and bs == 0 and not out.any()
    # a 32-bit frame is UNSUPPORTED
    hdr = fw.header(1024, 0, 24, 0, ss_code=7)
    assert decode_one(dec, hdr + b"\0" * 8, 1, 24)[3] & decode_cpu.DECODE_UNSUPPORTED
    # negative LPC shift -> PARSE
    neg = fw.frame(x, 0, 16, [dict(kind="lpc", order=1, coefs=[0], precision=2, shift=-1)])
    assert decode_one(dec, neg, 1, 16)[3] == decode_cpu.DECODE_PARSE
    # verify: one perturbed expected sample
    exp = np.zeros((1, 1, 1024), np.int32)
    exp[0, 0] = x[0]
    assert dec.decode_frames(good, [0], [len(good)], 1, 16, 1024, expected=exp)[3][0] == 0
    exp[0, 0, 500] += 1
    assert dec.decode_frames(good, [0], [len(good)], 1, 16, 1024, expected=exp)[3][0] == decode_cpu.DECODE_MISMATCH


def mutation_corpus(seed=0x5EED, per_frame=6):
    """(bytes, offsets, lengths, originals [(nch, bps, x)]) of mutated mono 16-bit frames."""
    rng = np.random.default_rng(seed)
    base = [f for f in oracle_corpus() if f[1] == 1 and f[2] == 16 and f[3].shape[1] <= 4096]
    base += [f[:4] for f in crafted_corpus() if f[1] == 1 and f[2] == 16]
    blobs = []
    for data, _, _, x in base:
        for k in range(per_frame):
            b = bytearray(data)
            mode = k % 3
            if mode == 0:
                for _ in range(1 + k):
                    i = int(rng.integers(len(b) * 8))
                    b[i // 8] ^= 0x80 >> (i % 8)
            elif mode == 1:
                b = b[: int(rng.integers(0, len(b)))]
            else:
                cut = int(rng.integers(0, len(b)))
                b = b[:cut] + bytearray(rng.integers(0, 256, int(rng.integers(0, 64)), np.uint8).tobytes())
            blobs.append((bytes(b), x))
    for _ in range(40):
        blobs.append((rng.integers(0, 256, int(rng.integers(0, 300)), np.uint8).tobytes(), None))
    offsets = np.cumsum([0] + [len(b) for b, _ in blobs[:-1]]).astype(np.uint64)
    return b"".join(b for b, _ in blobs), offsets, np.array([len(b) for b, _ in blobs], np.uint32), blobs


def test_mutation_corpus_gives_a_status_or_a_valid_decode(dec, tmp_path):
    data, offsets, lengths, blobs = mutation_corpus()
    out, bs, _, st = dec.decode_frames(data, offsets, lengths, 1, 16, 32768, threads=4)
    assert (st != 0).sum() > 0.8 * len(blobs)
    for f, (b, x) in enumerate(blobs):
        if st[f]:
            assert bs[f] == 0 and not out[f].any()
        else:  # a CRC collision or a mutation the CRC does not see must still decode validly
            ref = flac_parse.parse_frame(b, stream_bps=16)
            assert bs[f] == ref["block_size"] and np.array_equal(out[f, :, : bs[f]], ref["channels"])
    # the same corpus under ASan + UBSan, each frame from a buffer of exactly its own bytes: no report, same results
    exe = decode_cpu.build_sanitized_driver(str(tmp_path))
    st2, bs2, out2, _, _, err = decode_cpu.run_sanitized(exe, data, offsets, lengths, 1, 16, 32768, str(tmp_path))
    assert np.array_equal(st2, st) and np.array_equal(bs2, bs) and np.array_equal(out2, out), err


def planted_stream(n_frames=12, seed=11):
    """Mono 16-bit frames back to back; frame 3 is Verbatim and its samples spell a valid header (CRC-8 and all)."""
    rng = np.random.default_rng(seed)
    frames, xs = [], []
    for f in range(n_frames):
        x = signal(rng, 1152, 16)[None]
        if f == 3:
            fake = fw.header(1152, 0, 16, 200)
            fake = fake + b"\0" * (len(fake) % 2)
            spelled = np.frombuffer(fake, ">i2").astype(np.int64)
            x[0, 100:100 + len(spelled)] = spelled
            frames.append(fw.frame(x, 0, 16, [dict(kind="verbatim")], number=f))
        else:
            frames.append(fw.frame(x, 0, 16, [dict(kind="fixed", order=2)], number=f))
        xs.append(x)
    offsets = np.cumsum([0] + [len(b) for b in frames[:-1]]).astype(np.uint64)
    return b"".join(frames), offsets, np.array([len(b) for b in frames], np.uint32), xs


def test_index_follows_the_chain_past_a_planted_header(dec):
    data, offsets, lengths, xs = planted_stream()
    fake = fw.header(1152, 0, 16, 200)
    assert data.count(fake) == 1 and data.index(fake) > int(offsets[3])   # the plant is really there
    off, ln, ok = dec.index_frames(data, 1, 16, 64)
    assert ok and np.array_equal(off, offsets) and np.array_equal(ln, lengths)
    off, _, ok = dec.index_frames(data[:-1], 1, 16, 64)      # the chain no longer ends at n_bytes
    assert not ok and np.array_equal(off, offsets[:-1])
    _, _, ok = dec.index_frames(data, 1, 16, 5)              # more frames than max_frames
    assert not ok
    out, _, _, st = dec.decode_frames(data, offsets, lengths, 1, 16, 1152)
    assert not st.any() and all(np.array_equal(out[f], xs[f]) for f in range(len(xs)))
