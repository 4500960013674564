"""The block-size search on the GPU (flacenc_hip_encode_variable[_async]): every chosen frame's body is the fixed-blocking
encode+pack call's frame for the same samples at that block size, the tilings are the tree minimum over those frames'
lengths, and the variable-blocking stream decodes, verifies and indexes back to the input."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import flac_parse
import util
import vbs_model
from flacenc_rs_amd import _capi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOP = 1 << 36


@pytest.fixture(scope="module")
def h():
    with _capi.Handle(0) as handle:
        yield handle


def cfg_of(order=8, flags=0, use_fixed=True):
    return _capi.make_frame_config(_capi.make_config(lpc_order=order, flags=flags), use_fixed=use_fixed)


def material(n_sb, channels, S, bps, seed):
    """Superblocks whose quarters are independent sigen frames (a change of material every S/4 samples)."""
    q = _capi.sigen_frames(n_sb * 4, channels, S // 4, bps, 150.0, 0.5, 0.2, seed=seed)
    return np.ascontiguousarray(q.reshape(n_sb, 4, channels, S // 4).transpose(0, 2, 1, 3).reshape(n_sb, channels, S))


def music(S, channels=2):
    """The golden real-audio fixtures, tiled: ras103, ras22, sus109 one after the other."""
    ch = [np.concatenate([util.test_signal(nm, c % 2) for nm in ("ras103", "ras22", "sus109")]) for c in range(channels)]
    x = np.stack(ch, axis=1)
    n_sb = (len(x) + S - 1) // S
    rows = np.zeros((n_sb * S, channels), np.int32)
    rows[:len(x)] = x
    return np.ascontiguousarray(rows.reshape(n_sb, S, channels).transpose(0, 2, 1)), len(x)


def cut(x, total):
    """Zero beyond total_samples (what flacenc_hip_fill_le_bytes leaves in the last superblock)."""
    x = x.copy()
    S = x.shape[2]
    if total % S:
        x[total // S, :, total % S:] = 0
    return x[: (total + S - 1) // S]


def encode_pack(h, cfg, x, bps, rate=44100, first_frame=0):
    """The fixed-blocking encode+pack call on frames x [n, channels, b] -> list of frame bytes."""
    n, C, b = x.shape
    dx = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    slot = h.frame_bytes_bound(b, bps) if C == 2 else h.frame_bytes_bound_channels(C, b, bps)
    out = torch.zeros(n * slot, dtype=torch.uint8, device="cuda")
    ln = torch.zeros(n, dtype=torch.int32, device="cuda")
    res = torch.zeros(n * (752 if C == 2 else 368 * C), dtype=torch.uint8, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    if C == 2:
        h.encode_pack_stereo_frames_device(cfg, dx.data_ptr(), n, b, b, bps, rate, first_frame, 1, res.data_ptr(),
                                           out.data_ptr(), slot, ln.data_ptr(), s)
    else:
        h.encode_pack_frames_device(cfg, dx.data_ptr(), n, C, b, b, bps, rate, first_frame, 1, res.data_ptr(),
                                    out.data_ptr(), slot, ln.data_ptr(), s)
    torch.cuda.synchronize()
    o, lens = out.cpu().numpy(), ln.cpu().numpy()
    return [o[f * slot:f * slot + lens[f]].tobytes() for f in range(n)]


def header_len(frame):
    """Bytes of a frame header (sync .. CRC-8) from its codes and the coded number's first byte."""
    first = frame[4]
    ones = 0
    while ones < 8 and (first >> (7 - ones)) & 1:
        ones += 1
    bs, sr = frame[2] >> 4, frame[2] & 15
    extra = {6: 1, 7: 2}.get(bs, 0) + {12: 1, 13: 2, 14: 2}.get(sr, 0)
    return 4 + max(ones, 1) + extra + 1


def expected(h, cfg, x, total, S, levels, bps, first, rate=44100):
    """The rule of include/flacenc_hip.h restated over the fixed path's frames: -> (chosen frames, split masks), a
    chosen frame = (fixed-blocking bytes, frame number in its level, block size, sample number)."""
    n_full, tail = divmod(total, S)
    C = x.shape[1]
    fixed = []
    for k in range(levels):
        b = S >> k
        xs = x[:n_full].reshape(n_full, C, 1 << k, b).transpose(0, 2, 1, 3).reshape(n_full << k, C, b)
        fixed.append(encode_pack(h, cfg, xs, bps, rate) if n_full else [])
    chosen, masks = [], []
    for i in range(n_full):
        lens, node = [0] * (1 << levels), {}
        for n in range(1, 1 << levels):
            k = vbs_model.node_level(n)
            j = n - (1 << k)
            idx, b = (i << k) + j, S >> k
            sample = first + i * S + j * b
            fr = fixed[k][idx]
            lens[n] = len(fr) - len(vbs_model.coded_number(idx)) + len(vbs_model.coded_number(sample))
            node[n] = (fr, idx, b, sample)
        _, mask, leaves = vbs_model.tree_min(lens, levels)
        masks.append(mask)
        chosen += [node[n] for n in leaves]
    if tail:
        fr = encode_pack(h, cfg, x[n_full:n_full + 1, :, :tail], bps, rate, first_frame=n_full)[0]
        chosen.append((fr, n_full, tail, first + n_full * S))
        masks.append(0)
    return chosen, masks


def check(h, cfg, x, total, S, levels, bps, first=0, rate=44100, got=None):
    """Run the search (unless `got` is given) and hold every output to the fixed path and the decoder."""
    x = cut(x, total)
    C = x.shape[1]
    v = got or h.encode_variable(x, bps, cfg, levels, total_samples=total, block_size=S, sample_rate=rate,
                                 first_sample_number=first)
    chosen, masks = expected(h, cfg, x, total, S, levels, bps, first, rate)
    assert not v["overflow"]
    assert v["split_masks"].tolist() == masks
    assert v["frames"] == len(chosen)
    data = v["data"]
    pos = 0
    for f, (fr, idx, b, sample) in enumerate(chosen):
        off, ln = int(v["offsets"][f]), int(v["lengths"][f])
        assert off == pos and int(v["block_sizes"][f]) == b
        g = data[off:off + ln]
        hf, hv = header_len(fr), header_len(g)
        assert ln == len(fr) - hf + hv
        # body parity: every byte between header and CRC-16
        assert g[hv:-2] == fr[hf:-2], f
        code = vbs_model.coded_number(sample)
        head = bytes([0xFF, 0xF9]) + fr[2:4] + code + fr[4 + len(vbs_model.coded_number(idx)):hf - 1]
        assert g[:hv] == head + bytes([flac_parse.crc8(head)])  # (the CRC-16: the decoder's status below)
        pos += ln
    assert pos == v["bytes"] == len(data)
    # header fields by the test-side parser on a few frames
    for f in sorted({0, len(chosen) // 2, len(chosen) - 1}):
        p = flac_parse.parse_frame(data[int(v["offsets"][f]):], stream_bps=bps, stream_rate=rate)
        assert p["variable"] == 1 and p["number"] == chosen[f][3] and p["block_size"] == chosen[f][2]
    # decode, verify, index
    out, bs, num, st = h.decode_frames(data, v["offsets"], v["lengths"], C, bps, S)
    assert not st.any(), np.flatnonzero(st)[:8]
    assert bs.tolist() == v["block_sizes"].tolist()
    starts = np.concatenate([[0], np.cumsum(bs)[:-1]]).astype(np.uint64) + np.uint64(first)
    assert num.tolist() == starts.tolist()
    flat = np.concatenate([x[i] for i in range(len(x))], axis=1)[:, :total] if len(x) else np.zeros((C, 0))
    dec = np.concatenate([out[f, :, :bs[f]] for f in range(len(bs))], axis=1)
    assert np.array_equal(dec, flat)
    expect = np.zeros_like(out)
    for f in range(len(bs)):
        s0 = int(starts[f]) - first
        expect[f, :, :bs[f]] = flat[:, s0:s0 + bs[f]]
    assert not h.verify_frames(data, v["offsets"], v["lengths"], C, bps, S, expect).any()
    off, ln, ok = h.index_frames(data, C, bps, len(chosen) + 4)
    assert ok and off.tolist() == v["offsets"].tolist() and ln.tolist() == v["lengths"].tolist()
    return v


CASES = [(S, L) for S in (4096, 4608, 2048, 8192) for L in range(1, 6) if (S >> (L - 1)) >= 256 and L <= 4 or
         (L == 5 and (S >> 4) >= 256)]


@pytest.mark.parametrize("bps", [16, 24])
@pytest.mark.parametrize("S,levels", CASES)
def test_round_trip_and_body_parity(h, S, levels, bps):
    n_sb = 5
    total = n_sb * S - 777
    x = material(n_sb, 2, S, bps, seed=S * 7 + levels + bps)
    first = TOP - total if levels % 2 else 12345  # 7-byte sample numbers at the top of the range
    check(h, cfg_of(), x, total, S, levels, bps, first=first)


@pytest.mark.parametrize("S,levels", [(4096, 1), (4096, 3), (4096, 5), (2048, 2), (4608, 4)])
def test_golden_music(h, S, levels):
    x, total = music(S)
    check(h, cfg_of(), x, total, S, levels, 16, first=TOP - total if levels == 5 else 0)


@pytest.mark.parametrize("channels", [1, 3, 8])
@pytest.mark.parametrize("bps", [16, 24])
def test_independent_channels(h, channels, bps):
    S = 4096
    x = material(3, channels, S, bps, seed=channels * 31 + bps)
    check(h, cfg_of(), x, 3 * S - 100, S, 3, bps, first=99)


@pytest.mark.parametrize("flags", [_capi.FLAG_GENERIC_KERNEL, 32, 128])  # GENERIC_KERNEL, REFERENCE_ / CANONICAL_SUM_ORDER
def test_parity_modes_carry_through(h, flags):
    S = 4096
    x = material(3, 2, S, 16, seed=flags)
    check(h, cfg_of(flags=flags), x, 3 * S, S, 3, 16)


SEARCH_FLAGS = {"wasted": _capi.FLAG_WASTED_BITS, "orders": _capi.FLAG_ORDER_SEARCH, "windows": _capi.FLAG_WINDOW_SEARCH,
                "all": _capi.FLAG_WASTED_BITS | _capi.FLAG_ORDER_SEARCH | _capi.FLAG_WINDOW_SEARCH}


@pytest.mark.parametrize("S", [4096, 2048])  # (three levels: leaves of 1024 and 512 samples, the sub-wave shapes)
@pytest.mark.parametrize("name", list(SEARCH_FLAGS))
def test_wasted_bits_and_the_lpc_searches_carry_through(h, name, S):
    """Under WASTED_BITS, ORDER_SEARCH, WINDOW_SEARCH (the handle's default list) and all three, the search is held as
    under the parity modes: body parity with the fixed path frame by frame, the tree-minimum tilings, decode, verify
    and index."""
    x = material(5, 2, S, 16, seed=S + len(name)).astype(np.int64)
    x[1] <<= 8         # 16-bit content in a 24-bit container: wasted bits in some superblocks only,
    x[3, 0] <<= 3      # in one channel of another,
    x[4, :, S // 2:] <<= 5  # and in one half of the last
    check(h, cfg_of(flags=SEARCH_FLAGS[name]), x.astype(np.int32), 5 * S - 321, S, 3, 24)


def test_strict_gain_on_changing_material(h):
    """Quarters alternate between digital silence and a loud tone: coding the quarters alone wins."""
    S, n_sb = 4096, 8
    t = np.arange(S // 4)
    tone = np.round(20000 * np.sin(2 * np.pi * t / 37.0)).astype(np.int32)
    quarter = np.stack([tone, tone // 2])
    x = np.zeros((n_sb, 2, S), np.int32)
    for i in range(n_sb):
        for q in range(0, 4, 2):
            x[i, :, (q + i % 2) * S // 4:(q + i % 2 + 1) * S // 4] = quarter
    v = check(h, cfg_of(), x, n_sb * S, S, 3, 16)
    fixed_total = sum(map(len, encode_pack(h, cfg_of(), x, 16)))
    assert v["bytes"] < fixed_total
    assert (v["split_masks"] != 0).any() and v["frames"] > n_sb


def device_form(h, cfg, x, total, S, levels, bps, first, cap, mf, canary=0):
    """encode_variable_device with every output in a device buffer of `canary` bytes more than its room."""
    n_sb, C, stride = x.shape
    dx = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    out = torch.full((cap + canary + 1,), 0xAB, dtype=torch.uint8, device="cuda")
    off = torch.full((mf + canary + 1,), -1, dtype=torch.int64, device="cuda")
    ln = torch.full((mf + canary + 1,), -1, dtype=torch.int32, device="cuda")
    bs = torch.full((mf + canary + 1,), -1, dtype=torch.int32, device="cuda")
    masks = torch.full((n_sb + 1,), -1, dtype=torch.int32, device="cuda")
    tot = torch.zeros(2, dtype=torch.int64, device="cuda")
    h.encode_variable_device(cfg, dx.data_ptr(), total, C, S, levels, stride, bps, 44100, first, out.data_ptr(), cap,
                             off.data_ptr(), ln.data_ptr(), bs.data_ptr(), mf, masks.data_ptr(), tot.data_ptr(),
                             torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    u = lambda t, dt: t.cpu().numpy().view(dt)  # noqa: E731
    return u(out, np.uint8), u(off, np.uint64), u(ln, np.uint32), u(bs, np.uint32), u(masks, np.uint32), u(tot, np.uint64)


def test_host_form_equals_device_form(h):
    S, levels, bps = 4096, 4, 16
    x = cut(material(4, 2, S, bps, seed=5), 4 * S - 333)
    total = 4 * S - 333
    host = h.encode_variable(x, bps, cfg_of(), levels, total_samples=total, first_sample_number=77)
    cap, mf = _capi.variable_bytes_bound(2, S, levels, bps, total), _capi.variable_max_frames(S, levels, total)
    out, off, ln, bs, masks, tot = device_form(h, cfg_of(), x, total, S, levels, bps, 77, cap, mf)
    n = int(tot[0])
    assert n == host["frames"] and int(tot[1]) == host["bytes"]
    assert out[:int(tot[1])].tobytes() == host["data"]
    assert off[:n].tolist() == host["offsets"].tolist() and ln[:n].tolist() == host["lengths"].tolist()
    assert bs[:n].tolist() == host["block_sizes"].tolist() and masks[:4].tolist() == host["split_masks"].tolist()


def test_errors_and_overflow(h):
    S, bps = 4096, 16
    x = cut(material(3, 2, S, bps, seed=9), 3 * S - 5)
    total = 3 * S - 5
    cfg = cfg_of()
    for levels in (0, 6):
        with pytest.raises(_capi.FlacencHipError) as e:
            h.encode_variable(x, bps, cfg, levels, total_samples=total)
        assert e.value.code == _capi.ERR_BAD_ARGUMENT
    with pytest.raises(_capi.FlacencHipError) as e:  # 4098 is not divisible by 4
        h.encode_variable(np.zeros((1, 2, 4098), np.int32), bps, cfg, 3, out_capacity=1 << 16, max_frames=64)
    assert e.value.code == _capi.ERR_BAD_ARGUMENT
    with pytest.raises(_capi.FlacencHipError) as e:  # past 2^36
        h.encode_variable(x, bps, cfg, 2, total_samples=total, first_sample_number=TOP - total + 1)
    assert e.value.code == _capi.ERR_BAD_ARGUMENT
    assert not h.encode_variable(x, bps, cfg, 2, total_samples=total, first_sample_number=TOP - total)["overflow"]
    cap, mf = _capi.variable_bytes_bound(2, S, 3, bps, total), _capi.variable_max_frames(S, 3, total)
    _, _, _, _, _, tot = device_form(h, cfg, x, total, S, 3, bps, 0, cap, mf)
    need_bytes, need_frames = int(tot[1]), int(tot[0])
    # exactly enough room: written, and nothing beyond it
    out, off, ln, bs, _, tot = device_form(h, cfg, x, total, S, 3, bps, 0, need_bytes, need_frames, canary=64)
    assert int(tot[0]) == need_frames and (out[need_bytes:] == 0xAB).all()
    assert (off[need_frames:] == np.uint64(2 ** 64 - 1)).all() and (ln[need_frames:] == 0xFFFFFFFF).all()
    # one byte / one frame short: the flag, what it needs, and nothing written
    for room, frames in ((need_bytes - 1, need_frames), (need_bytes, need_frames - 1)):
        out, off, ln, bs, _, tot = device_form(h, cfg, x, total, S, 3, bps, 0, room, frames, canary=64)
        assert int(tot[0]) == need_frames | _capi.VARIABLE_OVERFLOW and int(tot[1]) == need_bytes
        assert (out == 0xAB).all() and (ln == 0xFFFFFFFF).all() and (bs == 0xFFFFFFFF).all()
    v = h.encode_variable(x, bps, cfg, 3, total_samples=total, max_frames=need_frames - 1)
    assert v["overflow"] and v["frames"] == need_frames and v["data"] == b""


def test_marked_lists_across_mixed_pipelines(h):
    """ADVICE medium: a sub-wave frames call that marks, a 4096-sample qlpc_batch on the same handle (the fused path,
    no clean-up launch behind it), the same sub-wave call again -- byte-identical to the generic path each time; then
    the block-size search on that material, which runs those pipelines one after the other in one call."""
    n, bps, nf = 576, 24, 200
    rng = np.random.default_rng(11)
    base = (rng.integers(0, 2, (8, n)) * 2 - 1).astype(np.int32) * (2 ** 23 - 1)
    x = np.ascontiguousarray(np.stack([base[rng.integers(0, 8, nf)], base[rng.integers(0, 8, nf)]], axis=1))
    x[::9] = _capi.sigen_frames(len(x[::9]), 2, n, bps, 120.0, 0.4, 0.1, seed=4)
    gen, genres = h.encode_stereo_frames(x, bps, cfg_of(flags=_capi.FLAG_GENERIC_KERNEL))
    first, fres = h.encode_stereo_frames(x, bps, cfg_of())
    assert first.tobytes() == gen.tobytes() and np.array_equal(fres, genres)
    y = _capi.sigen_frames(64, 1, 4096, 16, 200.0, 0.4, 0.2, seed=8).reshape(64, 4096)
    h.qlpc_batch(y, 16, _capi.make_config(lpc_order=8))
    again, ares = h.encode_stereo_frames(x, bps, cfg_of())
    assert again.tobytes() == gen.tobytes() and np.array_equal(ares, genres)
    # the search over superblocks of 4 x 576 samples
    S = 4 * n
    xs = np.ascontiguousarray(x[: nf // 4 * 4].reshape(nf // 4, 4, 2, n).transpose(0, 2, 1, 3).reshape(-1, 2, S))
    check(h, cfg_of(), xs, len(xs) * S, S, 3, bps)


def test_tools_round_trip(tmp_path):
    flac, wav = str(tmp_path / "v.flac"), str(tmp_path / "v.wav")
    enc = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "encode_flac.py"), flac, "--seconds", "3",
                          "--levels", "3"], capture_output=True, text=True, timeout=600)
    assert enc.returncode == 0, enc.stderr[-2000:]
    dec = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "decode_flac.py"), flac, wav],
                         capture_output=True, text=True, timeout=600)
    assert dec.returncode == 0 and "MD5 OK" in dec.stdout, dec.stdout + dec.stderr[-2000:]
    data = open(flac, "rb").read()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import decode_flac
    info, start = decode_flac.read_metadata(data)
    min_block, max_block = int.from_bytes(data[8:10], "big"), int.from_bytes(data[10:12], "big")
    assert max_block == 4096 and info["total_samples"] == 3 * 44100
    # the frames' own block sizes: min over all but the last, max = the superblock
    pos, sizes = start, []
    while pos < len(data):
        p = flac_parse.parse_frame(data[pos:], stream_bps=16, stream_rate=44100)
        assert p["variable"] == 1 and p["number"] == sum(sizes)
        sizes.append(p["block_size"])
        pos += p["length"]
    assert sum(sizes) == 3 * 44100 and min_block == min(sizes[:-1]) and max(sizes) <= 4096
    # the PCM: what the tool encoded
    import wave
    with wave.open(wav, "rb") as w:
        pcm = np.frombuffer(w.readframes(w.getnframes()), "<i2").reshape(-1, 2)
    n, rate = 4096, 44100
    nf = (3 * rate + n - 1) // n
    want = np.ascontiguousarray(_capi.sigen_frames(nf, 2, n, 16, rate / 440.0, 0.8, 0.2, seed=1)
                                .transpose(0, 2, 1)).reshape(-1, 2)[:3 * rate]
    assert np.array_equal(pcm, want)
