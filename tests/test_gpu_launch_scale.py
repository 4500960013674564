"""Launches at bench size and addresses past 2^31 / 2^32 bytes and elements (tests/scale_cases.py; DESIGN.md, "Launch
size and address range").

Tiled launches.  K = 32 base frames run in a small launch whose frame bytes are held to the CPU model frame by frame
(tests/stream_seam_cases.Model: the oracle's controller and bit writer and the project's models on top of it).  A launch
of N frames, frame f = base frame idx[f], built on the device, must then return base[idx[f]] for every f -- all bytes of
the decision records, the residual rows, and with frame number 0 / step 0 the frame bytes and lengths -- compared on the
device with torch.equal.  The oracle sees K frames whatever N is.  After the launch the hooks library reports the
handle's device buffers (flacenc_hip_debug_scratch_bytes): a case that claims a seam inside handle scratch asserts that
the largest buffer passed it, so a later chunking change cannot quietly turn the case into a small one.

Sparse launches.  The K frames once each in a layout whose stride puts one row with a seam (S31, S32, E31, E32) strictly
inside it and the others on both sides: input rows, residual rows, packed frames.  Truth is the dense launch.  The
allocation is torch.empty and never filled but for the rows, 4 KiB of sentinel either side of each and every place a row
beyond 2^31 bytes would land at had its offset been cut to 32 bits (bytes or elements, signed or unsigned); the pointer
the library gets lies 2 GiB + 64 KiB inside the allocation, so such a place is memory this test owns.  Every sentinel
must survive.

Tables.  Frame tables (decode, verify, md5_spans, place_frames) and stream tables (encode_streams, encode_streams_planar,
decode_streams, decode_ranges, decode_ranges_planar) with entries below 2^32, one span and one slot straddling it at
2^32 - len / 2, and entries above: equal to the call with dense tables, sentinels kept.  The block-size search runs
65 551 superblocks with sample numbers from 2^31, where a superblock's decision does not depend on its position.

Every comparison is of integers and bytes: exact.  A case skips only when the device has less free memory than
need_bytes(case) + 10 %; both numbers are in the reason."""
import time

import numpy as np
import pytest

import scale_cases as sc
import stream_seam_cases as ssc
from flacenc_rs_amd import _capi

pytestmark = pytest.mark.gpu

RATE = 44100
K = sc.K
CASES = {c.name: c for c in sc.cases()}
RES, CRES, PAR = sc.RES_BYTES, sc.CRES_BYTES, sc.PARAMS_BYTES


def _torch():
    import torch
    return torch


def _fits(need, what):
    torch = _torch()
    free, _ = torch.cuda.mem_get_info()
    if free < need + need // 10:
        pytest.skip(f"{what}: {free} bytes free on the device, {need} needed + 10 %")


def _stream():
    return _torch().cuda.current_stream().cuda_stream


def _u8(t):
    """A 2-D byte view [rows, bytes per row] of a contiguous tensor whose first dimension counts the rows."""
    torch = _torch()
    return t.view(torch.uint8).reshape(t.shape[0], -1)


def tile(base, idx_t):
    """base[idx] built in pieces on the device (frame f of the launch = base frame idx[f])."""
    torch = _torch()
    n = idx_t.numel()
    out = torch.empty((n,) + tuple(base.shape[1:]), dtype=base.dtype, device=base.device)
    per = max(1, base[0].numel() * base.element_size())
    step = max(1, sc.COMPARE_CHUNK // per)
    for a in range(0, n, step):
        torch.index_select(base, 0, idx_t[a:a + step], out=out[a:a + step])
    return out


def first_diff(got, base, idx_t, lens=None):
    """got [n, ...] against base[idx] row by row, in pieces, on the device -> None or (frame, byte).  lens: only the first
    lens[f] bytes of row f count (packed frames)."""
    torch = _torch()
    g2, b2 = _u8(got), _u8(base)
    assert g2.shape[1] == b2.shape[1], (g2.shape, b2.shape)
    n, w = g2.shape
    step = max(1, sc.COMPARE_CHUNK // w)
    cols = torch.arange(w, device=g2.device)[None, :] if lens is not None else None
    for a in range(0, n, step):
        want = b2.index_select(0, idx_t[a:a + step])
        g = g2[a:a + step]
        if lens is None:
            if torch.equal(g, want):
                continue
            ne = g != want
        else:
            ne = (g != want) & (cols < lens[a:a + step, None])
            if not bool(ne.any()):
                continue
        f, byte = ne.nonzero()[0].tolist()
        return a + f, byte
    return None


def frame_cfg(case):
    return _capi.make_frame_config(_capi.make_config(lpc_order=case.order, flags=case.flags), use_fixed=case.use_fixed)


def out_stride_of(case):
    return case.out_stride or (sc.stereo_bound(case.block, case.bps) if case.channels == 2
                               else sc.frame_bound(case.channels, case.block, case.bps))


def make_handle(case):
    h = _capi.Handle(0, hooks=True)
    if case.route in ("fused", "fused_pack", "certified4608", "channels"):
        h.debug_set_adaptive_order(False)  # the fused kernel's own certificate, whatever the material was
    return h


def run_frames(h, case, x_t, n, stride_elems=None, residual=None, residual_stride=None, out=None, out_stride=None,
               x_ptr=None):
    """The case's entry points over n frames at x_t (or x_ptr): -> dict of device tensors records, residual (None for
    the encode + pack calls), out, lens.  Frame numbers 0, step 0."""
    torch = _torch()
    cfg = frame_cfg(case)
    ch, b, bps = case.channels, case.block, case.bps
    stride = stride_elems or sc.padded(b)
    ptr = x_ptr if x_ptr is not None else x_t.data_ptr()
    ostride = out_stride or out_stride_of(case)
    rec_bytes = RES if ch == 2 else CRES * ch
    rec = torch.zeros((n, rec_bytes), dtype=torch.uint8, device="cuda")
    lens = torch.zeros(n, dtype=torch.int32, device="cuda")
    out_t = out if out is not None else torch.zeros((n, ostride), dtype=torch.uint8, device="cuda")
    out_ptr = out_t.data_ptr() if hasattr(out_t, "data_ptr") else int(out_t)
    s = _stream()
    if case.extra.get("encode_pack"):
        if ch == 2:
            h.encode_pack_stereo_frames_device(cfg, ptr, n, b, stride, bps, RATE, 0, 0, rec.data_ptr(), out_ptr, ostride,
                                               lens.data_ptr(), s)
        else:
            h.encode_pack_frames_device(cfg, ptr, n, ch, b, stride, bps, RATE, 0, 0, rec.data_ptr(), out_ptr, ostride,
                                        lens.data_ptr(), s)
        torch.cuda.synchronize()
        return {"records": rec, "residual": None, "out": out_t, "lens": lens}
    rstride = residual_stride or sc.padded(b)
    res_t = residual if residual is not None else torch.empty((n, ch, rstride), dtype=torch.int32, device="cuda")
    res_ptr = res_t.data_ptr() if hasattr(res_t, "data_ptr") else int(res_t)
    if ch == 2:
        h.encode_stereo_frames_device(cfg, ptr, n, b, stride, bps, rec.data_ptr(), res_ptr, rstride, s)
        h.pack_stereo_frames_device(ptr, n, b, stride, rec.data_ptr(), res_ptr, rstride, bps, RATE, 0, 0, out_ptr, ostride,
                                    lens.data_ptr(), s)
    else:
        h.encode_frames_device(cfg, ptr, n, ch, b, stride, bps, rec.data_ptr(), res_ptr, rstride, s)
        h.pack_frames_device(ptr, n, ch, b, stride, rec.data_ptr(), res_ptr, rstride, bps, RATE, 0, 0, out_ptr, ostride,
                             lens.data_ptr(), s)
    torch.cuda.synchronize()
    return {"records": rec, "residual": res_t, "out": out_t, "lens": lens}


def model_frame(case):
    """x int32 [channels, block] -> the bytes of that frame at number 0 by the CPU model of the case's flags."""
    flags = case.flags & ~_capi.FLAG_FUSED_PACK
    if flags == _capi.FLAG_PRECISION_SEARCH:  # (tests/stream_seam_cases.py has no model of these two)
        import order_model
        import precision_model
        from oracle import oracle as orc
        model = precision_model.Model()
        ofc = orc.make_frame_config(order_model.config(case.order), use_fixed=case.use_fixed)
        return lambda x: model.stereo_frame_bytes(x[0], x[1], case.bps, ofc, number=0, sample_rate=RATE)
    if flags & _capi.FLAG_RICE_ESCAPE and not flags & ~(_capi.FLAG_RICE_ESCAPE | _capi.FLAG_PRECISION_SEARCH):
        import escape_model
        import wasted_model
        fc = wasted_model.frame_config(order=case.order, use_fixed=case.use_fixed)
        analyse = None
        if flags & _capi.FLAG_PRECISION_SEARCH:
            # the search's winner is chosen unescaped and the escape pass runs on it (tests/test_gpu_rice_escape.py holds
            # the candidate batch to exactly this composition)
            import order_model
            import precision_model

            def analyse(x, w, _qlpc):
                rec, resid, _, _ = precision_model.record(x, w, order_model.config(case.order))
                if rec["status"] != 0:
                    return rec
                return dict(rec, residual=resid, coefs=rec["coefs"][:rec["order"]])
        return lambda x: escape_model.stereo_frame_bytes(x[0], x[1], case.bps, fc, number=0, analyse=analyse)
    _, model = ssc.configs(case.order, case.use_fixed, flags)
    assert model is not None, "no CPU model for these flags"
    return lambda x: model.frame(x, case.bps, RATE, 0)


_BASE = {}


def base_run(case):
    """The K base frames through the case's entry points, held to the CPU model frame by frame.  Shared by the cases of
    one configuration and never modified."""
    torch = _torch()
    key = (case.channels, case.block, case.bps, case.order, case.flags, case.use_fixed, bool(case.extra.get("encode_pack")),
           case.route in ("fused", "fused_pack", "certified4608", "channels"))
    if key in _BASE:
        return _BASE[key]
    assert sc.padded(case.block) == case.block  # rows are compared whole
    x = sc.base_frames(case.channels, case.block, case.bps)
    x_t = torch.from_numpy(x).cuda()
    h = make_handle(case)
    try:
        got = run_frames(h, case, x_t, K)
    finally:
        h.close()
    model = model_frame(case)
    out, lens = got["out"].cpu().numpy(), got["lens"].cpu().numpy()
    for f in range(K):
        want = model(x[f])
        assert int(lens[f]) == len(want) and out[f, :len(want)].tobytes() == want, (case.name, "base frame", f)
    got["x"] = x_t
    _BASE[key] = got
    return got


def check_scratch(h, case, report):
    total, largest = h.debug_scratch_bytes()
    report.append(f"scratch total {total} largest {largest}")
    bufs = {b.name: b for b in sc.buffers(case)}
    for name, seam in case.seams:
        if bufs[name].kind == "scratch":
            assert largest > sc.SEAMS[seam], (case.name, name, seam, largest)
    if case.route == "search" and case.flags & ~_capi.FLAG_RICE_ESCAPE:
        slices = h.debug_last_search_slices()
        report.append(f"slices {slices}")
        assert slices == sc.search_slices(case) if case.flags == _capi.FLAG_ORDER_SEARCH | _capi.FLAG_WINDOW_SEARCH else slices >= 1
        if case.flags == _capi.FLAG_ORDER_SEARCH | _capi.FLAG_WINDOW_SEARCH:
            assert slices >= 3, slices  # the slice loop runs more than twice
    # the route, by what it leaves behind: the kernels that decide inside (the fused 4096 / 4608 kernel, its bit writer, the
    # Independent(n) wave kernel) take no candidate rows from the handle, every other route all of them
    if case.channels == 2 and case.route != "wasted":
        cand_rows = sc.grown(4 * case.n * 4 * sc.padded(case.block))
        inside = case.route in ("fused", "fused_pack", "two_pass", "certified4608")
        assert (largest < cand_rows) if inside else (largest >= cand_rows), (case.name, case.route, largest, cand_rows)
    return total, largest


def tiled_frames_case(name):
    torch = _torch()
    case = CASES[name]
    _fits(sc.need_bytes(case), name)
    t0 = time.time()
    base = base_run(case)
    idx = sc.case_idx(case)
    idx_t = torch.from_numpy(idx).cuda()
    report = [name, f"N {case.n}"]
    x_big = tile(base["x"], idx_t)
    h = make_handle(case)
    got = None
    try:
        t1 = time.time()
        got = run_frames(h, case, x_big, case.n)
        report.append(f"launch {time.time() - t1:.3f} s")
        check_scratch(h, case, report)
        del x_big
        bad = first_diff(got["records"], base["records"], idx_t)
        assert bad is None, (name, "record of frame %d differs from base frame %d at byte %d" % (bad[0], idx[bad[0]], bad[1]))
        if got["residual"] is not None:
            bad = first_diff(got["residual"], base["residual"], idx_t)
            assert bad is None, (name, "residual of frame %d differs from base frame %d at byte %d" % (bad[0], idx[bad[0]], bad[1]))
        want_lens = base["lens"].index_select(0, idx_t)
        assert torch.equal(got["lens"], want_lens), (name, "out_len", int((got["lens"] != want_lens).nonzero()[0]))
        bad = first_diff(got["out"], base["out"], idx_t, lens=want_lens)
        assert bad is None, (name, "bytes of frame %d differ from base frame %d at byte %d" % (bad[0], idx[bad[0]], bad[1]))
        # the comparison itself: one bit in the last frame's record and in its last byte is found, one behind it is not
        last, end = case.n - 1, int(want_lens[case.n - 1])
        got["records"][last, -1] ^= 1
        assert first_diff(got["records"], base["records"], idx_t) == (last, got["records"].shape[1] - 1)
        got["out"][last, end] ^= 1
        assert first_diff(got["out"], base["out"], idx_t, lens=want_lens) is None
        got["out"][last, end - 1] ^= 1
        assert first_diff(got["out"], base["out"], idx_t, lens=want_lens) == (last, end - 1)
    finally:
        h.close()
        del got
        torch.cuda.empty_cache()
    report.append(f"wall {time.time() - t0:.2f} s")
    print(" | ".join(report))


FRAME_CASES = [c.name for c in sc.cases() if c.route not in ("qlpc_batch", "fixed_batch", "packer", "decode")]


@pytest.mark.parametrize("name", FRAME_CASES)
def test_tiled_launch(name):
    tiled_frames_case(name)


def test_tiled_packer_lengths_and_wire_at_a_64k_stride():
    """The stand-alone packer, the lengths kernel and the wire records over tiled records and rows: out_stride 64 KiB puts
    the packed frames past 2^32 bytes."""
    torch = _torch()
    case = CASES["packer out_stride 64 KiB"]
    _fits(sc.need_bytes(case), case.name)
    t0 = time.time()
    src = CASES["fused 4096/16/8 past S32"]
    base = base_run(src)
    idx = sc.case_idx(case)
    idx_t = torch.from_numpy(idx).cuda()
    n, b, bps = case.n, case.block, case.bps
    x_big, rec, resid = tile(base["x"], idx_t), tile(base["records"], idx_t), tile(base["residual"], idx_t)
    out = torch.zeros((n, case.out_stride), dtype=torch.uint8, device="cuda")
    assert out.numel() > sc.S32
    lens = torch.zeros(n, dtype=torch.int32, device="cuda")
    lens2, lens3 = torch.zeros_like(lens), torch.zeros_like(lens)
    h = _capi.Handle(0, hooks=True)
    try:
        s = _stream()
        h.pack_stereo_frames_device(x_big.data_ptr(), n, b, b, rec.data_ptr(), resid.data_ptr(), b, bps, RATE, 0, 0,
                                    out.data_ptr(), case.out_stride, lens.data_ptr(), s)
        h.stereo_frame_lengths_device(rec.data_ptr(), n, b, bps, RATE, 0, 0, lens2.data_ptr(), s)
        wb = h.frame_wire_bytes(b)
        wire = torch.zeros((n, wb), dtype=torch.uint8, device="cuda")
        wire_b = torch.zeros((K, wb), dtype=torch.uint8, device="cuda")
        h.stereo_frame_wire_device(rec.data_ptr(), n, b, bps, RATE, 0, 0, wire.data_ptr(), wb, lens3.data_ptr(), s)
        h.stereo_frame_wire_device(base["records"].data_ptr(), K, b, bps, RATE, 0, 0, wire_b.data_ptr(), wb, None, s)
        torch.cuda.synchronize()
        want_lens = base["lens"].index_select(0, idx_t)
        assert torch.equal(lens, want_lens) and torch.equal(lens2, want_lens) and torch.equal(lens3, want_lens)
        ostride = sc.stereo_bound(b, bps)
        base_out = torch.nn.functional.pad(base["out"], (0, case.out_stride - ostride))  # the K frames at the wide stride
        bad = first_diff(out, base_out, idx_t, lens=want_lens)
        assert bad is None, ("packed frame", bad, idx[bad[0]])
        bad = first_diff(wire, wire_b, idx_t)
        assert bad is None, ("wire record", bad, idx[bad[0]])
        print(case.name, "| scratch", h.debug_scratch_bytes(), f"| wall {time.time() - t0:.2f} s")
    finally:
        h.close()
        del x_big, rec, resid, out
        torch.cuda.empty_cache()


def test_tiled_decode_and_verify():
    """decode_frames / verify_frames over N frames whose bytes are the K base frames' (offsets tile them): the rows must be
    the tiled input, every status 0; the output rows pass 2^32 bytes."""
    torch = _torch()
    case = CASES["decode / verify 4096"]
    _fits(sc.need_bytes(case) + 2 * case.n * 2 * 4 * case.block, case.name)
    t0 = time.time()
    base = base_run(CASES["fused 4096/16/8 past S32"])
    idx = sc.case_idx(case)
    idx_t = torch.from_numpy(idx).cuda()
    n, b, bps = case.n, case.block, case.bps
    ostride = base["out"].shape[1]
    offsets = (idx_t * ostride).contiguous()
    lengths = base["lens"].index_select(0, idx_t).contiguous()
    rows = torch.empty((n, 2, b), dtype=torch.int32, device="cuda")
    assert rows.numel() * 4 > sc.S32
    bs = torch.zeros(n, dtype=torch.int32, device="cuda")
    num = torch.full((n,), -1, dtype=torch.int64, device="cuda")
    st = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    st2 = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    h = _capi.Handle(0, hooks=True)
    try:
        s = _stream()
        h.decode_frames_device(base["out"].data_ptr(), offsets.data_ptr(), lengths.data_ptr(), n, 2, bps, b, rows.data_ptr(), b,
                               bs.data_ptr(), num.data_ptr(), st.data_ptr(), s)
        torch.cuda.synchronize()
        assert not bool(st.any()), ("status", int(st.nonzero()[0]))
        assert bool((bs == b).all()) and not bool(num.any())
        bad = first_diff(rows, base["x"], idx_t)
        assert bad is None, ("decoded rows", bad, idx[bad[0]])
        h.verify_frames_device(base["out"].data_ptr(), offsets.data_ptr(), lengths.data_ptr(), n, 2, bps, b, rows.data_ptr(), b,
                               st2.data_ptr(), s)
        torch.cuda.synchronize()
        assert not bool(st2.any()), ("verify status", int(st2.nonzero()[0]))
        # one sample wrong beyond 2^32 bytes: exactly that frame reports MISMATCH
        f = n - 3
        rows[f, 1, b - 1] += 1
        h.verify_frames_device(base["out"].data_ptr(), offsets.data_ptr(), lengths.data_ptr(), n, 2, bps, b, rows.data_ptr(), b,
                               st2.data_ptr(), s)
        torch.cuda.synchronize()
        assert st2.nonzero().flatten().tolist() == [f] and int(st2[f]) == _capi.DECODE_MISMATCH
        print(case.name, "| scratch", h.debug_scratch_bytes(), f"| wall {time.time() - t0:.2f} s")
    finally:
        h.close()
        del rows
        torch.cuda.empty_cache()


@pytest.mark.parametrize("name", [c.name for c in sc.cases() if c.route == "qlpc_batch"])
def test_tiled_candidate_batch(name):
    """flacenc_hip_qlpc_batch_async with R[] and the unquantised coefficients wanted, and the stereo batch: the K base
    rows are held to the oracle as smoke() holds them; the rows of the large launch to those."""
    torch = _torch()
    from oracle import oracle as orc
    case = CASES[name]
    _fits(sc.need_bytes(case), name)
    t0 = time.time()
    stereo = bool(case.extra.get("stereo"))
    b, bps, n = case.block, case.bps, case.n
    qcfg = _capi.make_config(lpc_order=case.order, flags=case.flags)
    ocfg = orc.make_config(lpc_order=case.order, acorr=orc.ACORR_CANONICAL)
    x = sc.base_frames(2, b, bps)
    idx = sc.placement(n // 4 if stereo else n, K, seed=0xBA7C + n)
    idx_t = torch.from_numpy(idx).cuda()

    def run(h, x_t, units):
        rows = units * (4 if stereo else 1)
        par = torch.zeros((rows, PAR), dtype=torch.uint8, device="cuda")
        res = torch.empty((rows, b), dtype=torch.int32, device="cuda")
        R = torch.zeros((rows, 33), dtype=torch.float64, device="cuda")
        A = torch.zeros((rows, 32), dtype=torch.float64, device="cuda")
        if stereo:
            h.stereo_qlpc_batch_device(qcfg, x_t.data_ptr(), units, b, b, bps, par.data_ptr(), res.data_ptr(), b, _stream())
        else:
            width = torch.full((rows,), bps, dtype=torch.uint8, device="cuda")
            h.qlpc_batch_device(qcfg, x_t.data_ptr(), rows, b, b, width.data_ptr(), par.data_ptr(), res.data_ptr(), b,
                                R.data_ptr(), A.data_ptr(), _stream())
        torch.cuda.synchronize()
        return par, res, R, A

    h = _capi.Handle(0, hooks=True)
    try:
        # the base rows: channel 0 of every base frame (plain), the K frames (stereo)
        xb = torch.from_numpy(np.ascontiguousarray(x if stereo else x[:, 0])).cuda()
        par_b, res_b, R_b, A_b = run(h, xb, K)
        pb = par_b.cpu().numpy().view(_capi.PARAMS_DTYPE).reshape(-1)
        rb = res_b.cpu().numpy()
        for f in range(K):
            l, r = x[f, 0], x[f, 1]
            m, s_ = orc.stereo_to_midside(l, r)
            sigs = ((l, bps), (r, bps), (m, bps), (s_, bps + 1)) if stereo else ((l, bps),)
            for role, (sig, w) in enumerate(sigs):
                want = orc.estimated_qlpc(sig, w, ocfg)
                got = pb[f * len(sigs) + role]
                assert int(got["status"]) == want.get("status", 0), (f, role)
                if int(got["status"]) != 0:
                    continue
                k = want["order"]
                assert int(got["order"]) == k and int(got["shift"]) == want["shift"], (f, role)
                assert got["coefs"][:k].tolist() == want["coefs"].tolist(), (f, role)
                assert np.array_equal(rb[f * len(sigs) + role], want["residual"]), (f, role)
                assert int(got["subframe_bits"]) == want["subframe_bits"], (f, role)
        x_big = tile(xb, idx_t)
        par, res, R, A = run(h, x_big, len(idx))
        total, largest = h.debug_scratch_bytes()
        if stereo:  # four rows per unit: compare unit-wise
            par, res = par.reshape(len(idx), -1), res.reshape(len(idx), -1)
            par_b, res_b = par_b.reshape(K, -1), res_b.reshape(K, -1)
        for what, g, w in (("records", par, par_b), ("residual", res, res_b)) + (() if stereo else (("R[]", R, R_b), ("coefficients", A, A_b))):
            bad = first_diff(g, w, idx_t)
            assert bad is None, (name, what, bad, idx[bad[0]])
        print(name, f"| scratch total {total} largest {largest} | wall {time.time() - t0:.2f} s")
    finally:
        h.close()
        torch.cuda.empty_cache()


@pytest.mark.parametrize("name", [c.name for c in sc.cases() if c.route == "fixed_batch"])
def test_tiled_fixed_batch(name):
    """flacenc_hip_fixed_lpc_batch_async in both layouts with the selector keys: the base rows against the oracle's
    fixed_lpc as tests/test_gpu_parity.py holds them, the large launch against the base rows."""
    torch = _torch()
    from oracle import oracle as orc
    case = CASES[name]
    _fits(sc.need_bytes(case), name)
    t0 = time.time()
    stereo = bool(case.extra.get("stereo"))
    b, bps, n = case.block, case.bps, case.n
    per = 4 if stereo else 1
    cfg = _capi.make_frame_config(_capi.make_config(lpc_order=8), use_fixed=True)
    fc = orc.make_fixed_config(sum_mode=orc.SUMABS_CANONICAL)
    x = sc.base_frames(2, b, bps)
    idx = sc.placement(n // per, K, seed=0xF1ED + n)
    idx_t = torch.from_numpy(idx).cuda()

    def run(h, x_t, units):
        rows = units * per
        par = torch.zeros((rows, PAR), dtype=torch.uint8, device="cuda")
        res = torch.empty((rows, b), dtype=torch.int32, device="cuda")
        keys = torch.zeros(rows, dtype=torch.int64, device="cuda")
        h.fixed_lpc_batch_device(cfg, x_t.data_ptr(), units, b, b, None, bps,
                                 _capi.LAYOUT_STEREO_FRAMES if stereo else _capi.LAYOUT_SUBFRAMES, par.data_ptr(),
                                 res.data_ptr(), b, keys.data_ptr(), _stream())
        torch.cuda.synchronize()
        return par, res, keys

    h = _capi.Handle(0, hooks=True)
    try:
        xb = torch.from_numpy(np.ascontiguousarray(x if stereo else x[:, 0])).cuda()
        par_b, res_b, keys_b = run(h, xb, K)
        pb = par_b.cpu().numpy().view(_capi.PARAMS_DTYPE).reshape(-1)
        rb, kb = res_b.cpu().numpy(), keys_b.cpu().numpy().view(np.uint64)
        for f in range(K):
            l, r = x[f, 0], x[f, 1]
            sigs = [l, r, *orc.stereo_to_midside(l, r)] if stereo else [l]
            for role, sig in enumerate(sigs):
                w = orc.fixed_lpc(sig, bps + (1 if role == 3 else 0), 2 ** 63, fc)
                p, k = pb[f * per + role], f * per + role
                assert int(p["order"]) == w["order"] and int(kb[k]) == w["estimate"][w["order"]], (f, role)
                assert int(p["subframe_bits"]) == w["subframe_bits"] and int(p["code_bits"]) == w["code_bits"], (f, role)
                assert p["rice_params"][: 1 << w["rice_order"]].tolist() == w["rice_params"].tolist(), (f, role)
                assert np.array_equal(rb[k], w["residual"]), (f, role)
        x_big = tile(xb, idx_t)
        par, res, keys = run(h, x_big, len(idx))
        total, largest = h.debug_scratch_bytes()
        for what, g, w in (("records", par, par_b), ("residual", res, res_b), ("keys", keys, keys_b)):
            bad = first_diff(g.reshape(len(idx), -1), w.reshape(K, -1), idx_t)
            assert bad is None, (name, what, bad, idx[bad[0]])
        print(name, f"| scratch total {total} largest {largest} | wall {time.time() - t0:.2f} s")
    finally:
        h.close()
        torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------- sparse layouts
class Sparse:
    """Byte spans (n_rows rows of row_bytes at stride_bytes, or explicit (start, end) spans) from a pointer LEAD bytes
    inside a torch.empty allocation; sentinel in the guards and at every 32-bit alias of a span, nothing else filled."""

    def __init__(self, n_rows=0, row_bytes=0, stride_bytes=0, spans=None):
        torch = _torch()
        self.spans = spans or [(r * stride_bytes, r * stride_bytes + row_bytes) for r in range(n_rows)]
        self.n_rows = len(self.spans)
        total = sc.LEAD + max(e for _, e in self.spans) + sc.GUARD
        self.buf = torch.empty(total, dtype=torch.uint8, device="cuda")
        assert (self.buf.data_ptr() + sc.LEAD) % 16 == 0
        self.ptr = self.buf.data_ptr() + sc.LEAD
        self.n_bytes = total - sc.LEAD
        self.regions = sc.canary_regions_for(self.spans)
        for s, e in self.regions:
            self.buf[sc.LEAD + s:sc.LEAD + e] = sc.SENTINEL

    def row(self, r):
        s, e = self.spans[r]
        return self.buf[sc.LEAD + s:sc.LEAD + e]

    def put(self, rows2d):
        for r in range(self.n_rows):
            self.row(r).copy_(rows2d[r][:self.spans[r][1] - self.spans[r][0]])

    def rows(self):
        torch = _torch()
        return torch.stack([self.row(r) for r in range(self.n_rows)])

    def hit_a_canary_and_see_it(self):
        """The check itself: a byte of the last region changed is reported, then put back."""
        s, e = self.regions[-1]
        self.buf[sc.LEAD + e - 1] = 0
        with pytest.raises(AssertionError, match="sentinel overwritten at byte %d " % (e - 1)):
            self.assert_canaries("self-check")
        self.buf[sc.LEAD + e - 1] = sc.SENTINEL

    def assert_canaries(self, what):
        torch = _torch()
        ok = torch.stack([(self.buf[sc.LEAD + s:sc.LEAD + e] == sc.SENTINEL).all() for s, e in self.regions])
        if not bool(ok.all()):
            i = int((~ok).nonzero()[0])
            s, e = self.regions[i]
            at = int((self.buf[sc.LEAD + s:sc.LEAD + e] != sc.SENTINEL).nonzero()[0])
            raise AssertionError(f"{what}: sentinel overwritten at byte {s + at} from the pointer (region {s}..{e})")


SPARSE_SHAPES = {"4096 fused": "fused 4096/16/8 past S32", "1152 sub-wave": "sub-wave 1152/16/8",
                 "4096 Independent(3)": "Independent(3) 4096/16/8"}


@pytest.mark.parametrize("seam", list(sc.SEAMS))
@pytest.mark.parametrize("shape", list(SPARSE_SHAPES))
def test_sparse_rows_across_a_seam(shape, seam):
    """encode_stereo_frames with the seam inside one input row (residual dense), then inside one residual row (input
    dense), then pack_stereo_frames with the seam inside one packed frame: all equal to the dense launch."""
    torch = _torch()
    import dataclasses
    case = dataclasses.replace(CASES[SPARSE_SHAPES[shape]], extra={})  # encode, then pack: the residual rows are the caller's
    b, bps, ch = case.block, case.bps, case.channels
    s = sc.SEAMS[seam]
    row_bytes = 4 * b
    stride = sc.sparse_stride(s, row_bytes, 33)
    ostride_b = out_stride_of(case)
    ostride = sc.sparse_stride(s, ostride_b, 17)
    _fits(max(sc.LEAD + ch * K * stride, sc.LEAD + K * ostride) + (1 << 30), f"{shape} {seam}")
    t0 = time.time()
    base = base_run(case)
    ident = torch.arange(K, device="cuda")
    cfg = frame_cfg(case)
    h = make_handle(case)
    try:
        st = _stream()
        # 1. the input rows
        sp = Sparse(ch * K, row_bytes, stride)
        sp.put(_u8(base["x"].reshape(ch * K, b)))
        got = run_frames(h, case, None, K, stride_elems=stride // 4, x_ptr=sp.ptr)
        sp.assert_canaries("input rows")
        sp.hit_a_canary_and_see_it()
        for key in ("records", "residual", "lens"):
            assert torch.equal(got[key], base[key]), (shape, seam, "sparse input", key)
        assert first_diff(got["out"], base["out"], ident, lens=base["lens"]) is None
        del sp, got
        torch.cuda.empty_cache()
        # 2. the residual rows (and the packer reading them there)
        sp = Sparse(ch * K, row_bytes, stride)
        got = run_frames(h, case, base["x"], K, residual=sp.ptr, residual_stride=stride // 4)
        sp.assert_canaries("residual rows")
        assert torch.equal(sp.rows(), _u8(base["residual"].reshape(ch * K, b))), (shape, seam, "sparse residual")
        assert torch.equal(got["records"], base["records"]) and torch.equal(got["lens"], base["lens"])
        assert first_diff(got["out"], base["out"], ident, lens=base["lens"]) is None
        del sp, got
        torch.cuda.empty_cache()
        # 3. the packed frames
        sp = Sparse(K, ostride_b, ostride)
        lens = torch.zeros(K, dtype=torch.int32, device="cuda")
        if ch == 2:
            h.pack_stereo_frames_device(base["x"].data_ptr(), K, b, b, base["records"].data_ptr(),
                                        base["residual"].data_ptr(), b, bps, RATE, 0, 0, sp.ptr, ostride, lens.data_ptr(), st)
        else:
            h.pack_frames_device(base["x"].data_ptr(), K, ch, b, b, base["records"].data_ptr(), base["residual"].data_ptr(), b,
                                 bps, RATE, 0, 0, sp.ptr, ostride, lens.data_ptr(), st)
        torch.cuda.synchronize()
        sp.assert_canaries("packed frames")
        assert torch.equal(lens, base["lens"])
        assert first_diff(sp.rows(), base["out"], ident, lens=base["lens"]) is None, (shape, seam, "sparse out")
        del sp
    finally:
        h.close()
        torch.cuda.empty_cache()
    print(f"sparse {shape} {seam} | stride {stride} out_stride {ostride} | wall {time.time() - t0:.2f} s")


def test_fill_le_bytes_takes_65535_frames_and_refuses_one_more():
    """flacenc_hip_fill_le_bytes_async is bounded by a grid dimension: 65 535 frames work, 65 536 are BAD_ARGUMENT and
    nothing is written."""
    torch = _torch()
    ch, bpsmp, b = 2, 2, 64
    n = 65535
    rng = np.random.default_rng(9)
    pcm = rng.integers(-32768, 32768, ((n + 1) * b, ch), dtype=np.int16)
    pcm_t = torch.from_numpy(pcm).cuda()
    rows = torch.full((n + 1, ch, b), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    with _capi.Handle(0) as h:
        h.fill_le_bytes_device(pcm_t.data_ptr(), n * b, ch, bpsmp, n, b, rows.data_ptr(), b, _stream())
        torch.cuda.synchronize()
        want = pcm_t[:n * b].to(torch.int32).reshape(n, b, ch).permute(0, 2, 1)
        assert torch.equal(rows[:n], want) and bool((rows[n] == 0x5A5A5A5A).all())
        rows.fill_(0x5A5A5A5A)
        with pytest.raises(_capi.FlacencHipError) as e:
            h.fill_le_bytes_device(pcm_t.data_ptr(), (n + 1) * b, ch, bpsmp, n + 1, b, rows.data_ptr(), b, _stream())
        assert e.value.code == _capi.ERR_BAD_ARGUMENT
        torch.cuda.synchronize()
        assert bool((rows == 0x5A5A5A5A).all())


# ------------------------------------------------------------------------------------------------- byte tables
def test_byte_tables_with_a_frame_across_2_32():
    """decode_frames / verify_frames offsets, md5_spans, place_frames source and destination: half of the K base frames'
    bytes below 2^32, one frame straddling it at 2^32 - len / 2, the rest above.  Truth is the dense table."""
    import hashlib
    torch = _torch()
    case = CASES["fused 4096/16/8 past S32"]
    b, bps = case.block, case.bps
    _fits(2 * (sc.LEAD + sc.S32 + K * sc.stereo_bound(b, bps)) + (1 << 30), "byte tables")
    t0 = time.time()
    base = base_run(case)
    lens_h = base["lens"].cpu().numpy().astype(np.int64)
    slot = base["out"].shape[1]
    off = sc.straddling_offsets(lens_h, slot)
    spans = [(int(o), int(o + n)) for o, n in zip(off, lens_h)]
    frames_h = base["out"].cpu().numpy()
    off_t = torch.from_numpy(off).cuda()
    h = _capi.Handle(0)
    try:
        st_ = _stream()
        src = Sparse(spans=spans)
        src.put(base["out"])
        rows = torch.empty((K, 2, b), dtype=torch.int32, device="cuda")
        bs = torch.zeros(K, dtype=torch.int32, device="cuda")
        num = torch.full((K,), -1, dtype=torch.int64, device="cuda")
        st, st2 = torch.full((K,), -1, dtype=torch.int32, device="cuda"), torch.full((K,), -1, dtype=torch.int32, device="cuda")
        h.decode_frames_device(src.ptr, off_t.data_ptr(), base["lens"].data_ptr(), K, 2, bps, b, rows.data_ptr(), b,
                               bs.data_ptr(), num.data_ptr(), st.data_ptr(), st_)
        h.verify_frames_device(src.ptr, off_t.data_ptr(), base["lens"].data_ptr(), K, 2, bps, b, base["x"].data_ptr(), b,
                               st2.data_ptr(), st_)
        torch.cuda.synchronize()
        assert not bool(st.any()) and not bool(st2.any()) and bool((bs == b).all())
        assert torch.equal(rows, base["x"])
        dig = torch.zeros((K, 16), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()  # (md5_spans runs on the handle's own stream)
        h.md5_spans_device(src.ptr, src.n_bytes, off.astype(np.uint64), lens_h.astype(np.uint64), dig.data_ptr())
        want = np.stack([np.frombuffer(hashlib.md5(frames_h[f, :lens_h[f]].tobytes()).digest(), np.uint8) for f in range(K)])
        assert np.array_equal(dig.cpu().numpy(), want)
        # place_frames: the sparse table is the source, then the destination
        dense = np.concatenate([[0], np.cumsum(lens_h)[:-1]]).astype(np.int64)
        dense_t = torch.from_numpy(dense).cuda()
        total = int(lens_h.sum())
        dst = torch.full((total + 64,), sc.SENTINEL, dtype=torch.uint8, device="cuda")
        h.place_frames_device(src.ptr, off_t.data_ptr(), base["lens"].data_ptr(), K, dst.data_ptr(), dense_t.data_ptr(), st_)
        torch.cuda.synchronize()
        want_stream = np.concatenate([frames_h[f, :lens_h[f]] for f in range(K)])
        assert np.array_equal(dst[:total].cpu().numpy(), want_stream) and bool((dst[total:] == sc.SENTINEL).all())
        src.assert_canaries("source table")
        dst2 = Sparse(spans=spans)
        h.place_frames_device(dst.data_ptr(), dense_t.data_ptr(), base["lens"].data_ptr(), K, dst2.ptr, off_t.data_ptr(), st_)
        torch.cuda.synchronize()
        dst2.assert_canaries("destination table")
        for f in range(K):
            assert torch.equal(dst2.row(f), base["out"][f, :lens_h[f]]), f
        dst2.hit_a_canary_and_see_it()
    finally:
        h.close()
        torch.cuda.empty_cache()
    print(f"byte tables across 2^32 | straddling frame at {off[K // 2]} + {lens_h[K // 2]} | wall {time.time() - t0:.2f} s")


def test_pack_le_bytes_262147_frames():
    """flacenc_hip_pack_le_bytes on 262 147 stereo 16-bit frames of 4096: the packed PCM passes 2^32 bytes, the rows it
    reads 2^31 elements."""
    torch = _torch()
    n, ch, b = 262147, 2, 4096
    _fits(n * ch * b * 4 + 2 * n * ch * b * 2 + 3 * sc.COMPARE_CHUNK, "pack_le_bytes")
    t0 = time.time()
    x_t = torch.from_numpy(sc.base_frames(ch, b, 16)).cuda()
    idx = sc.placement(n, K, seed=0x1E + n)
    idx_t = torch.from_numpy(idx).cuda()
    x_big = tile(x_t, idx_t)
    assert x_big.numel() > (1 << 31)
    pcm_b = x_t.permute(0, 2, 1).to(torch.int16).contiguous()  # [K, b, ch]: interleaved little-endian
    bs = torch.full((n,), b, dtype=torch.int32, device="cuda")
    out = torch.empty(n * b * ch * 2, dtype=torch.uint8, device="cuda")
    assert out.numel() > sc.S32
    offs = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
    total = torch.zeros(1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()  # (pack_le_bytes runs on the handle's own stream)
    with _capi.Handle(0) as h:
        h.pack_le_bytes_device(x_big.data_ptr(), b, bs.data_ptr(), n, ch, 2, out.data_ptr(), out.numel(), offs.data_ptr(),
                               total.data_ptr())
    torch.cuda.synchronize()
    assert int(total[0]) == n * b and torch.equal(offs, torch.arange(n + 1, device="cuda") * b)
    bad = first_diff(out.reshape(n, -1), pcm_b, idx_t)
    assert bad is None, (bad, idx[bad[0]])
    del x_big, out
    torch.cuda.empty_cache()
    print(f"pack_le_bytes 262147 frames | wall {time.time() - t0:.2f} s")


def test_fill_le_bytes_65535_frames_of_8_channels():
    """flacenc_hip_fill_le_bytes_async at its largest launch: 8 channels x 4 bytes x 65 535 frames of 4096 is 8.6 GB of
    packed PCM in and as many bytes of rows out -- both past 2^32 bytes, and 32 768 elements short of 2^31 (the frame
    limit keeps this call below that seam at this block size)."""
    torch = _torch()
    n, ch, b = 65535, 8, 4096
    _fits(2 * n * ch * b * 4 + 3 * sc.COMPARE_CHUNK, "fill_le_bytes")
    t0 = time.time()
    x_t = torch.from_numpy(sc.base_frames(ch, b, 24)).cuda()
    idx = sc.placement(n, K, seed=0xF111)
    idx_t = torch.from_numpy(idx).cuda()
    pcm = tile(x_t.permute(0, 2, 1).contiguous(), idx_t)  # [n, b, ch] int32: the stream's bytes
    assert sc.S32 < pcm.numel() * 4 < sc.E31
    rows = torch.empty((n, ch, b), dtype=torch.int32, device="cuda")
    with _capi.Handle(0) as h:
        h.fill_le_bytes_device(pcm.data_ptr(), n * b, ch, 4, n, b, rows.data_ptr(), b, _stream())
        torch.cuda.synchronize()
    bad = first_diff(rows, x_t, idx_t)
    assert bad is None, (bad, idx[bad[0]])
    del pcm, rows
    torch.cuda.empty_cache()
    print(f"fill_le_bytes 65535 frames x 8 channels | wall {time.time() - t0:.2f} s")


@pytest.mark.parametrize("seam", list(sc.SEAMS))
def test_sparse_decode_and_le_bytes_rows_across_a_seam(seam):
    """The rows decode_frames writes, the rows pack_le_bytes reads and the rows fill_le_bytes writes, at a stride that puts
    the seam strictly inside row 33: equal to the dense call, every sentinel kept."""
    torch = _torch()
    case = CASES["fused 4096/16/8 past S32"]
    b, bps = case.block, case.bps
    row_bytes = 4 * b
    stride = sc.sparse_stride(sc.SEAMS[seam], row_bytes, 33)
    _fits(sc.LEAD + 2 * K * stride + (1 << 30), f"sparse rows {seam}")
    t0 = time.time()
    base = base_run(case)
    x_rows = _u8(base["x"].reshape(2 * K, b))
    pcm_b = base["x"].permute(0, 2, 1).to(torch.int16).contiguous()  # [K, b, 2]: interleaved 16-bit PCM
    ostride = base["out"].shape[1]
    offsets = (torch.arange(K, device="cuda") * ostride).contiguous()
    h = _capi.Handle(0)
    try:
        st_ = _stream()
        # decode_frames: the output rows
        sp = Sparse(2 * K, row_bytes, stride)
        bs = torch.zeros(K, dtype=torch.int32, device="cuda")
        st = torch.full((K,), -1, dtype=torch.int32, device="cuda")
        h.decode_frames_device(base["out"].data_ptr(), offsets.data_ptr(), base["lens"].data_ptr(), K, 2, bps, b, sp.ptr,
                               stride // 4, bs.data_ptr(), None, st.data_ptr(), st_)
        torch.cuda.synchronize()
        sp.assert_canaries("decode_frames rows")
        assert not bool(st.any()) and torch.equal(sp.rows(), x_rows), (seam, "decode_frames rows")
        # verify_frames reads its expected rows there
        h.verify_frames_device(base["out"].data_ptr(), offsets.data_ptr(), base["lens"].data_ptr(), K, 2, bps, b, sp.ptr,
                               stride // 4, st.data_ptr(), st_)
        torch.cuda.synchronize()
        assert not bool(st.any())
        # pack_le_bytes reads the same rows (they are the input's)
        sizes = torch.full((K,), b, dtype=torch.int32, device="cuda")
        out = torch.full((K * b * 2 * 2 + 64,), sc.SENTINEL, dtype=torch.uint8, device="cuda")
        offs = torch.zeros(K + 1, dtype=torch.int64, device="cuda")
        total = torch.zeros(1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        h.pack_le_bytes_device(sp.ptr, stride // 4, sizes.data_ptr(), K, 2, 2, out.data_ptr(), K * b * 4, offs.data_ptr(),
                               total.data_ptr())
        torch.cuda.synchronize()
        assert int(total[0]) == K * b and torch.equal(out[:K * b * 4], pcm_b.view(torch.uint8).reshape(-1))
        assert bool((out[K * b * 4:] == sc.SENTINEL).all())
        sp.assert_canaries("pack_le_bytes rows")
        del sp
        torch.cuda.empty_cache()
        # fill_le_bytes: the output rows
        sp = Sparse(2 * K, row_bytes, stride)
        h.fill_le_bytes_device(pcm_b.data_ptr(), K * b, 2, 2, K, b, sp.ptr, stride // 4, st_)
        torch.cuda.synchronize()
        sp.assert_canaries("fill_le_bytes rows")
        assert torch.equal(sp.rows(), x_rows), (seam, "fill_le_bytes rows")
        del sp
    finally:
        h.close()
        torch.cuda.empty_cache()
    print(f"sparse decode / le_bytes rows {seam} | stride {stride} | wall {time.time() - t0:.2f} s")


def test_stream_tables_across_2_32():
    """The stream tables of encode_streams, encode_streams_planar, decode_streams, decode_ranges and decode_ranges_planar:
    eight streams of four frames, input spans and output slots with four below 2^32, one straddling it at 2^32 - len / 2
    and three above.  Truth is the same call on the same data with dense tables."""
    torch = _torch()
    S, F, b, bps = 8, 4, 4096, 16
    L = F * b * 2 * 2                          # a stream's packed PCM
    cap = F * sc.stereo_bound(b, bps)          # a stream's slot of frames
    _fits(6 * (sc.LEAD + sc.S32 + S * 2 * L) + (1 << 30), "stream tables")
    t0 = time.time()
    x = sc.base_frames(2, b, bps)
    pcm_h = np.ascontiguousarray(x.reshape(S, F, 2, b).transpose(0, 1, 3, 2)).astype("<i2").reshape(S, -1).view(np.uint8)
    assert pcm_h.shape == (S, L)
    pcm_t = torch.from_numpy(pcm_h.copy()).cuda()
    planar_h = np.ascontiguousarray(x.reshape(S, F, 2, b).transpose(0, 2, 1, 3)).reshape(S, -1).view(np.uint8)  # [S, 2 * F * b * 4]
    planar_t = torch.from_numpy(planar_h.copy()).cuda()
    cfg = _capi.make_frame_config(_capi.make_config(lpc_order=8), use_fixed=True)

    def dense(n, slot):
        return np.arange(n, dtype=np.int64) * slot

    def sparse(lengths, slot):
        return sc.straddling_offsets(np.asarray(lengths, np.int64), slot)

    def spans_of(off, lengths):
        return [(int(o), int(o) + int(n)) for o, n in zip(off, lengths)]

    def i64(*shape):
        return torch.zeros(shape, dtype=torch.int64, device="cuda")

    h = _capi.Handle(0)
    try:
        # ---- encode_streams: dense, then sparse input offsets and output slots
        def encode(pcm_ptr, pcm_bytes, in_off, out_ptr, out_bytes, out_off):
            lens, totals = torch.zeros(S * F, dtype=torch.int32, device="cuda"), i64(S, 4)
            table = [(in_off[s], F * b, out_off[s], cap, 2, bps, 2, RATE) for s in range(S)]
            torch.cuda.synchronize()
            call, _ = h.encode_streams_device(pcm_ptr, pcm_bytes, table, cfg, b, out_ptr, out_bytes, lens.data_ptr(), S * F,
                                              totals.data_ptr())
            return lens, totals, call
        out_d = torch.full((S * cap,), sc.SENTINEL, dtype=torch.uint8, device="cuda")
        lens_d, tot_d, call_d = encode(pcm_t.data_ptr(), S * L, dense(S, L), out_d.data_ptr(), S * cap, dense(S, cap))
        nb = tot_d[:, 1].cpu().numpy()
        assert call_d[0] == S * F and (tot_d[:, 0] == F).all() and not bool(tot_d[:, 3].any()) and (nb > 0).all()
        flac_d = out_d.reshape(S, cap)
        in_off, out_off = sparse([L] * S, L), sparse([cap] * S, cap)
        src, dst = Sparse(spans=spans_of(in_off, [L] * S)), Sparse(spans=spans_of(out_off, [cap] * S))
        src.put(pcm_t)
        lens_s, tot_s, call_s = encode(src.ptr, src.n_bytes, in_off, dst.ptr, dst.n_bytes, out_off)
        assert call_s == call_d and torch.equal(lens_s, lens_d) and torch.equal(tot_s, tot_d)
        for s in range(S):
            assert torch.equal(dst.row(s)[:nb[s]], flac_d[s, :nb[s]]), ("encode_streams", s)
        src.assert_canaries("encode_streams pcm")
        dst.assert_canaries("encode_streams slots")
        del src, dst
        # ---- encode_streams_planar: int32 rows, the same streams
        def encode_planar(ptr, nbytes, in_off, out_ptr, out_bytes, out_off):
            lens, totals = torch.zeros(S * F, dtype=torch.int32, device="cuda"), i64(S, 4)
            dig = torch.zeros((S, 16), dtype=torch.uint8, device="cuda")
            table = [(in_off[s], F * b, out_off[s], cap, 2, bps, 2, RATE) for s in range(S)]
            torch.cuda.synchronize()
            call, _ = h.encode_streams_planar_device(ptr, nbytes, _capi.SAMPLE_I32, F * b, table, cfg, b, out_ptr, out_bytes,
                                                     lens.data_ptr(), S * F, totals.data_ptr(), dig.data_ptr())
            return lens, totals, dig, call
        P = 2 * F * b * 4
        out_p = torch.full((S * cap,), sc.SENTINEL, dtype=torch.uint8, device="cuda")
        lens_p, tot_p, dig_p, call_p = encode_planar(planar_t.data_ptr(), S * P, dense(S, P), out_p.data_ptr(), S * cap,
                                                     dense(S, cap))
        assert call_p == call_d and torch.equal(lens_p, lens_d) and torch.equal(tot_p, tot_d) and torch.equal(out_p, out_d)
        in_off = sparse([P] * S, P)
        src, dst = Sparse(spans=spans_of(in_off, [P] * S)), Sparse(spans=spans_of(out_off, [cap] * S))
        src.put(planar_t)
        lens_s, tot_s, dig_s, call_s = encode_planar(src.ptr, src.n_bytes, in_off, dst.ptr, dst.n_bytes, out_off)
        assert call_s == call_d and torch.equal(lens_s, lens_d) and torch.equal(tot_s, tot_d) and torch.equal(dig_s, dig_p)
        for s in range(S):
            assert torch.equal(dst.row(s)[:nb[s]], flac_d[s, :nb[s]]), ("encode_streams_planar", s)
        src.assert_canaries("encode_streams_planar rows")
        dst.assert_canaries("encode_streams_planar slots")
        del src, dst
        torch.cuda.empty_cache()
        # ---- decode_streams: the frames just made, sparse spans in, sparse slots out
        def decode(ptr, nbytes, in_off, out_ptr, out_bytes, out_off):
            totals = i64(S, 4)
            table = [(in_off[s], nb[s], out_off[s], L, 2, bps, b, 2) for s in range(S)]
            torch.cuda.synchronize()
            call, _ = h.decode_streams_device(ptr, nbytes, table, 4096, out_ptr, out_bytes, totals.data_ptr())
            return totals, call, table
        pcm_back = torch.full((S * L,), sc.SENTINEL, dtype=torch.uint8, device="cuda")
        dt_d, dcall_d, _ = decode(out_d.data_ptr(), S * cap, dense(S, cap), pcm_back.data_ptr(), S * L, dense(S, L))
        assert dcall_d == [S * F, S * F * b] and torch.equal(pcm_back.reshape(S, L), pcm_t)
        f_off, o_off = sparse(nb, cap), sparse([L] * S, L)
        src, dst = Sparse(spans=spans_of(f_off, nb)), Sparse(spans=spans_of(o_off, [L] * S))
        src.put(flac_d)
        dt_s, dcall_s, streams = decode(src.ptr, src.n_bytes, f_off, dst.ptr, dst.n_bytes, o_off)
        assert dcall_s == dcall_d and torch.equal(dt_s, dt_d) and torch.equal(dst.rows(), pcm_t)
        src.assert_canaries("decode_streams spans")
        dst.assert_canaries("decode_streams slots")
        del dst
        # ---- decode_ranges and decode_ranges_planar: one crop per stream from the sparse spans into sparse slots
        first, count = 1000, 9000
        for planar in (False, True):
            slot = count * 2 * (4 if planar else 2)

            def ranges_call(out_ptr, out_bytes, r_off):
                totals = i64(S, 4)
                ranges = [(first, count, r_off[s], s) for s in range(S)]
                torch.cuda.synchronize()
                if planar:
                    call, _ = h.decode_ranges_planar_device(src.ptr, src.n_bytes, streams, ranges, 4096, out_ptr, out_bytes,
                                                            _capi.SAMPLE_I32, totals.data_ptr())
                else:
                    call, _ = h.decode_ranges_device(src.ptr, src.n_bytes, streams, ranges, 4096, out_ptr, out_bytes,
                                                     totals.data_ptr())
                return totals, call
            crop_d = torch.full((S * slot,), sc.SENTINEL, dtype=torch.uint8, device="cuda")
            rt_d, rcall_d = ranges_call(crop_d.data_ptr(), S * slot, dense(S, slot))
            assert (rt_d[:, 0] == count).all() and not bool(rt_d[:, 1].any())
            if planar:
                want = torch.from_numpy(np.ascontiguousarray(
                    x.reshape(S, F, 2, b).transpose(0, 2, 1, 3).reshape(S, 2, F * b)[:, :, first:first + count])).cuda()
                assert torch.equal(crop_d.view(torch.int32).reshape(S, 2, count), want)
            else:
                assert torch.equal(crop_d.reshape(S, slot), pcm_t[:, first * 4:(first + count) * 4])
            r_off = sparse([slot] * S, slot)
            dst = Sparse(spans=spans_of(r_off, [slot] * S))
            rt_s, rcall_s = ranges_call(dst.ptr, dst.n_bytes, r_off)
            assert rcall_s == rcall_d and torch.equal(rt_s, rt_d) and torch.equal(dst.rows(), crop_d.reshape(S, slot))
            dst.assert_canaries("decode_ranges%s slots" % ("_planar" if planar else ""))
            del dst
        src.assert_canaries("decode_ranges spans")
        del src
    finally:
        h.close()
        torch.cuda.empty_cache()
    print(f"stream tables across 2^32 | wall {time.time() - t0:.2f} s")


def test_tiled_block_size_search():
    """flacenc_hip_encode_variable_async, 2 levels, 65 551 superblocks of 4096: the levels' packed frames in handle scratch
    pass 2^31 bytes.  Sample numbers start at 2^31, so every coded number takes 7 bytes and a superblock's decision and
    lengths do not depend on where it stands.  The K base superblocks are held to the fixed-blocking path and the decoder
    by tests/test_gpu_variable_block.check; the tiled launch must repeat their split masks, block sizes and lengths,
    lay its frames back to back, and decode -- both CRCs, numbers, every sample -- to the tiled input."""
    torch = _torch()
    import test_gpu_variable_block as tvb
    n, S, levels, bps, first = 65551, 4096, 2, 16, 1 << 31
    _fits(24 << 30, "block-size search")
    t0 = time.time()
    cfg = _capi.make_frame_config(_capi.make_config(lpc_order=8), use_fixed=True)
    x = sc.base_frames(2, S, bps)
    idx = sc.placement(n, K, seed=0xB10C + n)
    idx_t = torch.from_numpy(idx).cuda()
    h = _capi.Handle(0, hooks=True)
    try:
        h.debug_set_adaptive_order(False)
        v = tvb.check(h, cfg, x, K * S, S, levels, bps, first=first)
        splits = int(v["split_masks"].astype(bool).sum())
        masks_b = torch.from_numpy(v["split_masks"].astype(np.int32)).cuda()
        cnt_b = np.where(v["split_masks"] != 0, 2, 1)
        start_b = np.concatenate([[0], np.cumsum(cnt_b)[:-1]])
        len_b, bs_b = np.zeros((K, 2), np.int32), np.zeros((K, 2), np.int32)
        for k in range(K):
            len_b[k, :cnt_b[k]] = v["lengths"][start_b[k]:start_b[k] + cnt_b[k]]
            bs_b[k, :cnt_b[k]] = v["block_sizes"][start_b[k]:start_b[k] + cnt_b[k]]
        x_big = tile(torch.from_numpy(x).cuda(), idx_t)
        total = n * S
        cap = _capi.variable_bytes_bound(2, S, levels, bps, total)
        mf = _capi.variable_max_frames(S, levels, total)
        out = torch.empty(cap, dtype=torch.uint8, device="cuda")
        off, ln = torch.zeros(mf, dtype=torch.int64, device="cuda"), torch.zeros(mf, dtype=torch.int32, device="cuda")
        bs, masks = torch.zeros(mf, dtype=torch.int32, device="cuda"), torch.full((n,), -1, dtype=torch.int32, device="cuda")
        tot = torch.zeros(2, dtype=torch.int64, device="cuda")
        h.encode_variable_device(cfg, x_big.data_ptr(), total, 2, S, levels, S, bps, RATE, first, out.data_ptr(), cap,
                                 off.data_ptr(), ln.data_ptr(), bs.data_ptr(), mf, masks.data_ptr(), tot.data_ptr(), _stream())
        torch.cuda.synchronize()
        scratch_total, largest = h.debug_scratch_bytes()
        assert largest > sc.S31, largest  # the levels' packed frames
        # decisions and lengths: the base superblock's, frame after frame
        assert torch.equal(masks, masks_b.index_select(0, idx_t))
        valid = (torch.arange(2, device="cuda")[None, :] < torch.from_numpy(cnt_b).cuda().index_select(0, idx_t)[:, None])
        want_ln = torch.from_numpy(len_b).cuda().index_select(0, idx_t)[valid]
        want_bs = torch.from_numpy(bs_b).cuda().index_select(0, idx_t)[valid]
        m = int(want_ln.numel())
        assert int(tot[0]) == m and int(tot[1]) == int(want_ln.sum())
        assert torch.equal(ln[:m], want_ln) and torch.equal(bs[:m], want_bs)
        assert torch.equal(off[:m], torch.cumsum(want_ln.to(torch.int64), 0) - want_ln)
        # the way back: every frame parses with both CRCs, carries its sample number and decodes to the tiled input
        sb = torch.arange(n, device="cuda")[:, None].expand(n, 2)[valid]
        half = torch.arange(2, device="cuda")[None, :].expand(n, 2)[valid]
        expect = x_big.index_select(0, sb)
        second = half == 1
        expect[second] = expect[second].roll(-(S // 2), dims=2)
        st = torch.full((m,), -1, dtype=torch.int32, device="cuda")
        h.verify_frames_device(out.data_ptr(), off.data_ptr(), ln.data_ptr(), m, 2, bps, S, expect.data_ptr(), S, st.data_ptr(),
                               _stream())
        torch.cuda.synchronize()
        assert not bool(st.any()), ("verify status", int(st.nonzero()[0]))
        del expect
        rows = torch.empty((m, 2, S), dtype=torch.int32, device="cuda")
        got_bs, num = torch.zeros(m, dtype=torch.int32, device="cuda"), torch.zeros(m, dtype=torch.int64, device="cuda")
        h.decode_frames_device(out.data_ptr(), off.data_ptr(), ln.data_ptr(), m, 2, bps, S, rows.data_ptr(), S,
                               got_bs.data_ptr(), num.data_ptr(), st.data_ptr(), _stream())
        torch.cuda.synchronize()
        assert not bool(st.any()) and torch.equal(got_bs, want_bs)
        assert torch.equal(num, first + sb * S + half * (S // 2))
        print(f"block-size search {n} superblocks | {splits} of {K} base superblocks split | frames {m} | scratch total {scratch_total} largest {largest} | "
              f"wall {time.time() - t0:.2f} s")
    finally:
        h.close()
        torch.cuda.empty_cache()
