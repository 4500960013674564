"""flacenc_hip_recover_streams on the GPU: every batch of tests/recover_cases.py against the model of
tests/recover_model.py through the C ABI, in host and in device memory -- slot prefixes, all eight totals, the gap
records in order, call_totals and FILL wherever the rule says untouched --, the consequence for undamaged streams
(flacenc_hip_decode_streams' bytes), isolation, the plan, the errors and garbage.  Every comparison is exact."""
import functools

import numpy as np
import pytest

import recover_cases as rc
import recover_model as model
import streams_cases as cases
from flacenc_rs_amd import _capi

pytestmark = pytest.mark.gpu
FILL = cases.FILL
GAP_FILL = 0x5B5B5B5B5B5B5B5B


@functools.lru_cache(None)
def wanted(name):
    batch, origins = rc.all_batches()[name]
    return model.expected_batch(batch, origins)


def run_host(h, batch, origins, max_gaps, gaps="own", max_frames=None):
    out = batch.fresh_out()
    table = np.full((max_gaps + 2, 3), GAP_FILL, np.uint64)
    _, totals, _, call = h.recover_streams(batch.data, batch.table, batch.max_frames() if max_frames is None else max_frames,
                                           out, origins=origins, max_gaps=max_gaps,
                                           gaps=None if gaps is None else table)
    assert (table[max_gaps:] == GAP_FILL).all()
    return out, totals, table, call


def run_device(h, batch, origins, max_gaps, gaps="own", max_frames=None):
    import torch
    dev = torch.device("cuda:0")
    d_in = torch.from_numpy(batch.data if len(batch.data) else np.zeros(1, np.uint8)).to(dev)
    d_out = torch.full((max(1, batch.out_bytes),), FILL, dtype=torch.uint8, device=dev)
    d_tot = torch.full((len(batch.streams), 8), -1, dtype=torch.int64, device=dev)
    d_gaps = torch.full((max_gaps + 2, 3), GAP_FILL, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    call, _ = h.recover_streams_device(d_in.data_ptr(), len(batch.data), batch.table.copy(),
                                       batch.max_frames() if max_frames is None else max_frames, d_out.data_ptr(),
                                       d_out.numel(), d_tot.data_ptr(), origins=origins,
                                       gaps_ptr=0 if gaps is None else d_gaps.data_ptr(), max_gaps=max_gaps)
    table = d_gaps.cpu().numpy().astype(np.uint64)
    assert (table[max_gaps:] == GAP_FILL).all()
    return d_out.cpu().numpy(), d_tot.cpu().numpy().astype(np.uint64), table, call


RUNS = {"host": run_host, "device": run_device}


@pytest.mark.parametrize("memory", ["host", "device"])
@pytest.mark.parametrize("name", ["damage", "room", "odd", "crowd", "garbage"])
def test_every_case_batch_equals_the_model(hooks_handle, name, memory):
    batch, origins = rc.all_batches()[name]
    want = wanted(name)
    n_gaps = len(model.gap_records(want))
    out, totals, gaps, call = RUNS[memory](hooks_handle, batch, origins, n_gaps)
    model.check_batch(batch, out, totals, gaps, call, want)


@pytest.mark.parametrize("memory", ["host", "device"])
def test_the_gap_table_takes_what_fits_and_nothing_beyond(hooks_handle, memory):
    batch, origins = rc.all_batches()["damage"]
    want = wanted("damage")
    total = len(model.gap_records(want))
    assert total > 8
    for max_gaps, gaps in ((0, None), (0, "own"), (total, "own"), (total - 1, "own"), (total + 5, "own"), (3, "own")):
        out, totals, table, call = RUNS[memory](hooks_handle, batch, origins, max_gaps, gaps)
        assert call[2] == total
        model.check_batch(batch, out, totals, table[:max_gaps], call, want, max_gaps=max_gaps)
        assert (table[min(total, max_gaps):] == GAP_FILL).all()


def uniform(s):
    """A stream of streams_cases whose coded numbers place its frames back to back from 0: variable blocking, or fixed
    blocking with every block but the last of max_block_size samples."""
    return s.name.startswith("variable") or all(n == s.mbs for _, n in s.frame_sizes[:-1])


def test_undamaged_streams_give_what_decode_streams_gives(hooks_handle):
    h = hooks_handle
    streams = [s for s in cases.mixed() if uniform(s)]
    assert len(streams) >= 18 and {s.channels for s in streams} == {1, 2, 3, 8}
    # streams the library's own encoder writes, origin 0
    rng = np.random.default_rng(9)
    for channels, bps, n, frames, tail in ((2, 16, 192, 6, 40), (1, 8, 64, 9, 17), (3, 24, 128, 5, 100)):
        width = (bps + 7) // 8
        x = np.cumsum(rng.integers(-40, 41, (channels, frames * n + tail)), axis=1).clip(-100, 100)
        pcm = cases.pack(x, width)
        cfg = _capi.make_frame_config(_capi.make_config(lpc_order=8), use_fixed=True)
        data, lens = h.encode_pcm(pcm, channels, cfg, width, bps, n, 44100)
        streams.append(cases.Stream("encoder %d" % channels, np.array(data, copy=True), channels, bps, n, pcm))
    batch = cases.Batch(streams, seed=3)
    ref = batch.fresh_out()
    ref_totals, ref_call, _ = h.decode_streams(batch.data, batch.table, batch.max_frames(), ref)
    assert not ref_totals[:, 3].any()
    out, totals, gaps, call = run_host(h, batch, None, 4)
    assert np.array_equal(out, ref)
    assert np.array_equal(totals[:, :2], ref_totals[:, :2]) and not totals[:, 2:].any()
    assert call == [ref_call[0], ref_call[1], 0, 0] and (gaps == GAP_FILL).all()
    for i, s in enumerate(streams):
        assert np.array_equal(batch.slot(out, i), s.pcm), s.name
    out_d, totals_d, _, call_d = run_device(h, batch, [0] * len(streams), 0, None)
    assert np.array_equal(out_d, ref) and np.array_equal(totals_d, totals) and call_d == call


def test_damage_in_one_stream_changes_nothing_for_the_others(hooks_handle):
    h = hooks_handle
    streams = [s for s in cases.mixed() if uniform(s) and len(s.data)]
    batch = cases.Batch(streams, seed=8)
    clean = run_device(h, batch, None, 0, None)
    for k in (0, 1, len(streams) // 2, len(streams) - 1):
        s = streams[k]
        bad = s.data.copy()
        bad[len(bad) // 2] ^= 0x04
        hurt = cases.Batch(streams[:k] + [s.but("hurt", bad)] + streams[k + 1:], capacities=batch.capacities, seed=8)
        assert hurt.out_offsets == batch.out_offsets and hurt.offsets == batch.offsets
        out, totals, _, call = run_device(h, hurt, None, 0, None)
        for i in range(len(streams)):
            same = np.array_equal(batch.slot(out, i), batch.slot(clean[0], i)) and np.array_equal(totals[i], clean[1][i])
            assert same == (i != k), (k, i)
        assert int(totals[k][5]) >= 1 and int(totals[k][0]) == int(clean[1][k][0]) - 1


def test_the_plan_depends_on_neither_the_streams_nor_the_damage(hooks_handle):
    h = hooks_handle
    items = rc.damage_streams()
    four = [items["undamaged " + n][0] for n in ("mono", "stereo", "3ch", "8ch")]
    many = cases.Batch([four[i % 4] for i in range(64)], capacities=[4096] * 64, spacing=2)
    run_host(h, cases.Batch(four, capacities=[4096] * 4), None, 4, max_frames=many.max_frames())
    plan4 = h.debug_last_recover_plan()
    run_host(h, many, None, 4)
    plan64 = h.debug_last_recover_plan()
    assert plan4 == plan64 and plan4[3] == 4 and plan4[1] == 2 and plan4[2] <= 6
    # 0 and 50 damaged streams of 64
    hurt = []
    for i in range(64):
        s = four[i % 4]
        bad = s.data.copy()
        bad[len(bad) // 3] ^= 0x20
        hurt.append(s.but("hurt %d" % i, bad) if i < 50 else s)
    hb = cases.Batch(hurt, capacities=[4096] * 64, spacing=2)
    out, totals, gaps, call = run_host(h, hb, None, 64)
    assert h.debug_last_recover_plan() == plan64 and call[2] >= 25 and sum(int(t[5]) for t in totals) >= 50
    for kind in (run_device,):
        kind(h, many, None, 4)
        plan_d = h.debug_last_recover_plan()
        kind(h, hb, None, 64)
        assert h.debug_last_recover_plan() == plan_d and plan_d[1] == 2 and plan_d[2] <= 3


def test_the_other_calls_are_not_disturbed(hooks_handle):
    """Plans and outputs of flacenc_hip_decode_streams and flacenc_hip_decode_ranges on a fixed batch are the same before
    and after a flacenc_hip_recover_streams call on the same handle."""
    h = hooks_handle
    batch = cases.Batch(cases.mixed(), seed=9)
    ranges = [(10, 100, 4096 * i, i) for i in range(len(batch.streams)) if len(batch.streams[i].data)]

    def both():
        out = batch.fresh_out()
        totals, call, _ = h.decode_streams(batch.data, batch.table, batch.max_frames(), out)
        plan_s = h.debug_last_decode_streams_plan()
        r_out = np.full(4096 * (len(batch.streams) + 1), FILL, np.uint8)
        r_totals, r_call, _ = h.decode_ranges(batch.data, batch.table, ranges, batch.max_frames(), r_out)
        return (out, totals, call, tuple(plan_s), r_out, r_totals, r_call, tuple(h.debug_last_decode_ranges_plan()))

    before = both()
    b, origins = rc.all_batches()["damage"]
    run_host(h, b, origins, 8)
    run_device(h, b, origins, 8)
    after = both()
    for x, y in zip(before, after):
        assert np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y


def test_arguments(hooks_handle):
    h = hooks_handle
    items = rc.damage_streams()
    batch = cases.Batch([items[n][0] for n in ("body bit", "undamaged mono", "frame removed")], capacities=[4096] * 3,
                        gaps=[4, 4, 4])
    lib, E = h._lib, _capi
    out = batch.fresh_out()
    totals = np.full((3, 8), 0x77, np.uint64)
    gaps = np.full((8, 3), 0x77, np.uint64)
    call = np.zeros(4, np.uint64)

    def rc_(table=None, data=None, n_bytes=None, n_streams=None, max_frames=None, out_ptr=None, out_bytes=None,
            totals_ptr=None, call_ptr=None, table_ptr=None, kind=E.MEM_HOST, gaps_ptr=None, max_gaps=8):
        t = batch.table if table is None else table
        d = batch.data
        return lib.flacenc_hip_recover_streams(
            h._h, d.ctypes.data if data is None else data, len(d) if n_bytes is None else n_bytes,
            t.ctypes.data if table_ptr is None else table_ptr, len(t) if n_streams is None else n_streams, None,
            batch.max_frames() if max_frames is None else max_frames, out.ctypes.data if out_ptr is None else out_ptr,
            len(out) if out_bytes is None else out_bytes, totals.ctypes.data if totals_ptr is None else totals_ptr,
            gaps.ctypes.data if gaps_ptr is None else (gaps_ptr or None), max_gaps,
            call.ctypes.data if call_ptr is None else call_ptr, kind)

    def changed(i, **fields):
        t = batch.table.copy()
        for k, v in fields.items():
            t[i][k] = v
        return t

    bad = [dict(data=0), dict(table_ptr=0), dict(out_ptr=0), dict(totals_ptr=0), dict(call_ptr=0), dict(kind=7),
           dict(n_streams=(1 << 24) + 1), dict(max_frames=(1 << 30) + 1), dict(n_bytes=len(batch.data) - 60),
           dict(out_bytes=len(out) - 30), dict(table=batch.table[::-1].copy()),
           dict(table=changed(1, offset=batch.table[0]["offset"] + 3)),
           dict(table=changed(2, n_bytes=len(batch.data))), dict(table=changed(1, out_capacity=len(out))),
           dict(table=changed(0, out_offset=(1 << 64) - 1)), dict(table=changed(0, channels=0)),
           dict(table=changed(2, channels=9)), dict(table=changed(1, max_block_size=0)),
           dict(table=changed(1, max_block_size=65537)), dict(table=changed(0, bytes_per_sample=5)),
           dict(table=changed(0, bytes_per_sample=1)), dict(gaps_ptr=0, max_gaps=1)]
    for kw in bad:
        assert rc_(**kw) == E.ERR_BAD_ARGUMENT, kw
    for bits in (3, 25, 32):
        assert rc_(table=changed(1, bits_per_sample=bits, bytes_per_sample=4)) == E.ERR_UNSUPPORTED
    untouched = lambda: (out == FILL).all() and (gaps == 0x77).all()
    assert untouched() and (totals == 0x77).all() and not call.any()
    assert rc_(n_streams=0) == E.OK and (totals == 0x77).all() and untouched()
    # too few frames: the flag, zero totals, nothing written; the retry succeeds
    want = [model.expected(s.data, s.channels, s.bps, s.mbs, s.width, 4096) for s in batch.streams]
    frames = sum(t[0] + t[3] for _, t, _ in want)
    assert rc_(max_frames=frames - 1) == E.OK
    assert int(call[0]) == E.INDEX_ERROR and not call[1:].any() and not totals.any() and untouched()
    assert rc_(max_frames=frames) == E.OK and rc_(gaps_ptr=0, max_gaps=0) == E.OK
    model.check_batch(batch, out, totals, gaps, call, want, max_gaps=8)


def test_decode_many_through_errors_writes_the_recovered_wavs(hooks_handle, tmp_path):
    """tools/decode_many.py --through-errors on one intact and one damaged .flac of tools/encode_flac.py: the intact
    file's PCM is its input and its MD5 matches; the damaged one keeps its length, has one block of silence where the
    broken frame was and reads "damaged"; tools/decode_flac.py says the same for the one file."""
    import os
    import subprocess
    import sys
    import wave
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tools"))
    import decode_flac
    import decode_many
    import encode_flac
    h = hooks_handle
    n = 256
    x = np.cumsum(np.random.default_rng(78).integers(-300, 301, (6 * n + 77, 2)), axis=0).astype(np.int32).clip(-30000, 30000)
    good = encode_flac.encode_pcm(x, 16, 44100, h, block_size=n)[0]
    info, start = decode_flac.read_metadata(good)
    bad = bytearray(good)
    bad[start + (len(good) - start) // 2] ^= 0x40
    results = decode_many.recover_all([good, bytes(bad)], h)
    want = np.ascontiguousarray(x.astype("<i2")).reshape(-1).view(np.uint8)
    pcm, _, totals, gaps = results[0]
    assert np.array_equal(pcm, want) and totals[2:] == [0] * 6 and gaps == []
    assert decode_many.recovered_status(pcm, info, totals) == "MD5 OK"
    pcm, _, totals, gaps = results[1]
    assert totals[0] == 6 and totals[1] == len(x) and totals[2] == n and len(gaps) == 1 and gaps[0][1] == n
    lo, hi = gaps[0][0] * 4, (gaps[0][0] + n) * 4
    assert not pcm[lo:hi].any() and np.array_equal(pcm[:lo], want[:lo]) and np.array_equal(pcm[hi:], want[hi:])
    assert decode_many.recovered_status(pcm, info, totals) == "damaged"
    paths = [str(tmp_path / "good.flac"), str(tmp_path / "bad.flac")]
    open(paths[0], "wb").write(good)
    open(paths[1], "wb").write(bytes(bad))
    p = subprocess.run([sys.executable, os.path.join(root, "tools", "decode_many.py"), *paths, "--out-dir",
                        str(tmp_path / "wavs"), "--through-errors"], check=True, capture_output=True, text=True)
    assert p.stdout.count("MD5 OK") == 1 and p.stdout.count("damaged") == 1 and "1 breaks" in p.stdout
    with wave.open(str(tmp_path / "wavs" / "bad.wav"), "rb") as w:
        assert w.getnframes() == len(x) and w.getnchannels() == 2
    p = subprocess.run([sys.executable, os.path.join(root, "tools", "decode_flac.py"), paths[1],
                        str(tmp_path / "one.wav"), "--through-errors"], check=True, capture_output=True, text=True)
    assert "damaged" in p.stdout and "%d of silence in 1 gaps" % n in p.stdout
