"""Launch size and address range: the cases of tests/test_gpu_launch_scale.py, the material they run, where their
buffers cross 2^31 / 2^32 bytes or elements, what they need in device memory, and the checkers of their results.  Pure
numpy (the bench signal comes from the host generator of the library, no GPU); tests/test_scale_cases_cpu.py holds
every statement made here without a device.

Tiling.  K distinct base frames run in a small launch that is held to the CPU model as the other suites hold one.  A
launch of N frames is then built on the device, frame f = base frame idx[f] (placement), and must return
base_result[idx[f]] for every f: records, residual rows and -- with frame numbers 0, step 0 -- frame bytes and lengths.

Seams.  Four offsets from any pointer the library is given or owns: S31 = 2^31 bytes, S32 = 2^32 bytes (2^30 int32
elements), E31 = 2^31 elements (8 GiB), E32 = 2^32 elements (16 GiB).  A dense case names the seams its buffers pass:
its N is the smallest count that puts a whole row beyond the seam, raised to the next odd count with a partial last
workgroup where the kernel takes several frames per workgroup.  Rows of a power-of-two size tile the seam exactly -- a
row ends at it and the next one starts there -- so only buffers whose row size does not divide the seam have a row with
the seam strictly inside (seam_rows says which of the two holds).  The sparse cases of the GPU file choose their stride
so that one row always has the seam strictly inside it (sparse_stride).

Memory.  need_bytes(case) is caller buffers + handle scratch by the sizing rules of api_candidates.cpp (candidate_scratch,
attach_scratch), api_frames.cpp (the encode + pack calls' residual rows, the
wasted-bits rows) and api_pack.cpp (the escape list), each grown as flacenc_hip::ensure grows a buffer (a quarter more +
256 bytes), + the largest temporary the comparison makes.  The rule is a condition, not a measurement: at most 64 GiB
per case on a card of 288 GB that is shared."""
from dataclasses import dataclass, field

import numpy as np

K = 32
S31, S32, E31, E32 = 1 << 31, 1 << 32, 1 << 33, 1 << 34  # byte offsets
SEAMS = {"S31": S31, "S32": S32, "E31": E31, "E32": E32}
MEMORY_RULE = 64 << 30
COMPARE_CHUNK = 256 << 20  # the comparison gathers base[idx[a:b]] in pieces of at most this many bytes
GUARD = 4096               # bytes of sentinel either side of every row of a sparse layout
LEAD = (2 << 30) + (64 << 10)  # a sparse buffer's pointer lies this far inside its allocation
SENTINEL = 0xA5

RES_BYTES, CRES_BYTES, PARAMS_BYTES = 752, 368, 352
SEARCH_SCRATCH_CAP = 768 << 20  # kSearchScratchCap (order_search.h)


def padded(block):
    """padded_stride (api_internal.h): the row stride of handle scratch, whole 16-byte groups."""
    return (block + 3) & ~3


def grown(nbytes):
    """What flacenc_hip::ensure allocates for a request (api_handle.cpp)."""
    return nbytes + nbytes // 4 + 256 if nbytes else 0


def stereo_bound(block, bps):
    """flacenc_hip_stereo_frame_bytes_bound (frame_pack.cpp), rounded to 16 as the C ABI rounds it."""
    bits = 2 * 8 + block * (2 * bps + 1)
    return (15 + (bits + 7) // 8 + 2 + 15) & ~15


def frame_bound(channels, block, bps):
    """flacenc_hip_frame_bytes_bound."""
    bits = channels * (8 + block * bps)
    return (15 + (bits + 7) // 8 + 2 + 15) & ~15


# ---------------------------------------------------------------------------------------------- material
def special_frames(bps):
    """Base-frame indices whose subframes the order certificate recomputes or marks (near-pure tones, a block that
    opens on a clipped plateau) and, at 24 bits, the frames with wasted bits: what a seam's row is made of."""
    return (20, 21, 22, 23) + ((28, 29) if bps == 24 else ())


def base_frames(channels, block, bps):
    """int32 [K, channels, block]: 0-7 the bench signal, 8-13 the golden music fixtures, 14-19 extreme_signals'
    worst cases, 20-21 near-pure tones, 22-23 a block opening on a clipped plateau, 24 silence, 25 a constant, 26-27
    full-scale noise (Verbatim), 28-31 more of the bench signal -- at 24 bits 28-29 frames with wasted bits and 30-31
    a full-range ramp with noise in the low bits (escapes)."""
    import extreme_signals as xs
    from flacenc_rs_amd import _capi

    lo, hi = -(1 << (bps - 1)), (1 << (bps - 1)) - 1
    t = np.arange(block, dtype=np.float64)
    rng = np.random.default_rng(0x5CA1E + 131 * block + bps + 7 * channels)
    x = np.zeros((K, channels, block), np.int64)
    bench = _capi.sigen_frames(12, channels, block, bps, 200.0, 0.4, 0.4, seed=0xF1AC0001, nthreads=2)
    x[0:8] = bench[0:8]
    x[28:32] = bench[8:12]
    for i in range(6):
        for c in range(channels):
            x[8 + i, c] = xs.music(block, bps, seed=i, start=(i * channels + c) * 977)
    ext = np.concatenate([xs.extreme_frames(rng, block, bps) for _ in range((channels + 1) // 2)], axis=1)
    x[14:20] = ext[:, :channels]
    for i in range(2):  # near-pure tones: the autocorrelation matrix is all but singular
        for c in range(channels):
            period = (17.0, 5.5)[i] * (1.0 + 0.01 * c)
            x[20 + i, c] = np.rint(0.9 * hi * np.sin(2 * np.pi * t / period + 0.3 * c)) + rng.integers(-1, 2, block) * i
    for i in range(2):  # a clipped plateau at the block's start, then a tone
        for c in range(channels):
            tone = 0.7 * hi * np.sin(2 * np.pi * t / (40.0 + 7 * i + c))
            x[22 + i, c] = np.rint(tone)
            x[22 + i, c, :block // (5 + i)] = hi if (c + i) % 2 == 0 else lo
    x[25] = int(hi // 3)
    x[26:28] = rng.integers(lo, hi + 1, (2, channels, block))
    if bps == 24:
        x[28:30] = (bench[8:10].astype(np.int64) >> 6) << 6
        x[29, channels - 1] = (x[29, channels - 1] >> 9) << 9
        ramp = np.linspace(lo, hi, block).astype(np.int64)
        for c in range(channels):
            x[30, c] = np.clip(ramp + rng.integers(-(1 << 14), 1 << 14, block), lo, hi)
            x[31, c] = np.clip(-ramp + rng.integers(-(1 << 10), 1 << 10, block), lo, hi)
    assert x.min() >= lo and x.max() <= hi
    return np.ascontiguousarray(x.astype(np.int32))


def placement(n, k, seed, pins=None, special=()):
    """idx int64 [n]: launch position f runs base frame idx[f].  The first 16 positions hold 16 base frames and the last
    16 the other 16, `special` among them (k frames do not fit 16 positions twice over: between them the two ends hold
    every base frame); positions 16 .. 16 + 2k hold every base frame once at an even and once at an odd position;
    `pins` {position: base frame} come last (the frames whose rows meet a seam) -- a pin among the last 16 positions
    (a launch that is the smallest to cross its seam) moves the special frame it names there; the rest is uniform."""
    assert n >= 32 + 2 * k and k == 32 and len(special) <= 16
    pins = dict(pins or {})
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, k, n).astype(np.int64)
    others = [int(f) for f in rng.permutation(k) if int(f) not in special]
    head, tail = others[:16], others[16:] + [int(f) for f in special]
    tail_pins = {pos: f for pos, f in pins.items() if pos >= n - 16}
    assert all(f in special for f in tail_pins.values()) and len(set(tail_pins.values())) == len(tail_pins), tail_pins
    free = [f for f in tail if f not in tail_pins.values()]
    rng.shuffle(free)
    idx[:16] = head
    for pos in range(n - 16, n):
        idx[pos] = tail_pins[pos] if pos in tail_pins else free.pop()
    p2 = rng.permutation(k)
    idx[16:16 + 2 * k:2] = p2
    idx[17:17 + 2 * k:2] = np.roll(p2, 1)
    for pos, frame in pins.items():
        if pos < n - 16:
            assert 16 + 2 * k <= pos, (pos, n)
            idx[pos] = frame
    return idx


# ---------------------------------------------------------------------------------------------- cases
@dataclass(frozen=True)
class Buf:
    """`rows` rows of row_bytes at stride_bytes; rows_per_frame consecutive rows hold one frame's data
    (row r belongs to frame r // rows_per_frame)."""
    name: str
    kind: str          # "caller" or "scratch"
    rows: int
    row_bytes: int
    stride_bytes: int
    rows_per_frame: int = 1

    @property
    def nbytes(self):
        return (self.rows - 1) * self.stride_bytes + self.row_bytes if self.rows else 0


@dataclass(frozen=True)
class Case:
    name: str
    route: str      # what the launch must run as: fused, fused_pack, two_pass, certified4608, subwave, bigblock, general,
                    # wasted, search, channels, qlpc_batch, fixed_batch, packer, decode
    channels: int   # 2: stereo frames with the stereo decision; else Independent(channels); 0: candidate rows
    block: int
    bps: int
    order: int
    flags: int
    n: int          # frames (rows for the candidate batches)
    seams: tuple    # (buffer name, seam name) this case claims
    use_fixed: bool = True
    out_stride: int = 0  # 0: the bound
    extra: dict = field(default_factory=dict, hash=False, compare=False)


def buffers(case):
    """Every large buffer of a case: the caller's and the handle's scratch (requests, before ensure's growth)."""
    n, b, ch = case.n, case.block, case.channels
    row, prow = 4 * b, 4 * padded(b)
    out = []
    if case.route in ("qlpc_batch", "fixed_batch"):
        out += [Buf("in", "caller", n, row, prow), Buf("residual", "caller", n, row, prow),
                Buf("records", "caller", n, PARAMS_BYTES, PARAMS_BYTES)]
        if case.extra.get("want_fp"):
            out += [Buf("autocorr", "caller", n, 33 * 8, 33 * 8), Buf("lpc_coefs", "caller", n, 32 * 8, 32 * 8)]
        if case.route == "fixed_batch":
            out += [Buf("keys", "caller", n, 8, 8), Buf("d_sumabs", "scratch", n, 1280, 1280)]
        out += [Buf("d_split", "scratch", n, 408, 408)]
        return out
    rows_in = n * ch
    if case.route == "decode":
        bound = stereo_bound(b, case.bps)
        return [Buf("bytes", "caller", K, bound, bound), Buf("offsets", "caller", n, 8, 8),
                Buf("lengths", "caller", n, 4, 4), Buf("out", "caller", rows_in, row, prow, ch),
                Buf("expected", "caller", K * ch, row, prow, ch), Buf("d_dec", "scratch", n, 64 * ch + 64, 64 * ch + 64)]
    rec = RES_BYTES if ch == 2 else CRES_BYTES * ch
    ostride = case.out_stride or (stereo_bound(b, case.bps) if ch == 2 else frame_bound(ch, b, case.bps))
    out += [Buf("in", "caller", rows_in, row, prow, ch), Buf("records", "caller", n, rec, rec),
            Buf("out", "caller", n, ostride, ostride), Buf("out_len", "caller", n, 4, 4),
            Buf("d_esc", "scratch", n + 16, 4, 4)]
    if case.extra.get("encode_pack"):
        out.append(Buf("d_presid", "scratch", rows_in, prow, prow, ch))
    else:
        out.append(Buf("residual", "caller", rows_in, row, prow, ch))
    per = 4 if ch == 2 else ch
    cand = n * per  # candidate rows
    split = Buf("d_split", "scratch", cand, 408, 408)
    sumabs = Buf("d_sumabs", "scratch", cand, 1280, 1280)
    cands = [Buf("d_cparams", "scratch", cand, PARAMS_BYTES, PARAMS_BYTES), Buf("d_cresid", "scratch", cand, prow, prow, per),
             Buf("d_minmax", "scratch", cand, 8, 8)]
    fixed = [Buf("d_fparams", "scratch", cand, PARAMS_BYTES, PARAMS_BYTES), Buf("d_fresid", "scratch", cand, prow, prow, per),
             Buf("d_fkeys", "scratch", cand, 8, 8)] if case.use_fixed else []
    if case.route in ("fused", "fused_pack", "two_pass", "certified4608", "channels"):
        out += [split, sumabs]
    elif case.route in ("subwave", "bigblock", "general", "search"):
        out += [split, sumabs] + cands + fixed
        if case.route == "search":
            out.append(Buf("d_order", "scratch", 1, SEARCH_SCRATCH_CAP, SEARCH_SCRATCH_CAP))  # the slices' bound
        if case.route == "bigblock" and b > 16384:
            out.append(Buf("d_tables", "scratch", cand, 256 * 32 * 4, 256 * 32 * 4))
    elif case.route == "wasted":
        m = case.extra["wasted_frames"]  # frames the scan marks: an upper bound by the placement
        out += [split, sumabs, Buf("d_wk", "scratch", n, 4, 4), Buf("d_wlist", "scratch", n + 1, 4, 4),
                Buf("d_wrows", "scratch", m * 4, prow, prow), Buf("d_wbps", "scratch", m * 4, 1, 1),
                Buf("d_cparams", "scratch", m * 4, PARAMS_BYTES, PARAMS_BYTES), Buf("d_cresid", "scratch", m * 4, prow, prow),
                Buf("d_fparams", "scratch", m * 4, PARAMS_BYTES, PARAMS_BYTES), Buf("d_fresid", "scratch", m * 4, prow, prow),
                Buf("d_fkeys", "scratch", m * 4, 8, 8)]
    elif case.route != "packer":
        raise ValueError(case.route)
    return out


def search_slices(case, windows=6):
    """How many slices launch_order_search (order_search.cpp) cuts a search case's subframes into: slice_subframes and
    bytes_per_subframe restated for ORDER_SEARCH | WINDOW_SEARCH with a fresh handle's five extra windows, one precision."""
    per = windows * 33 * 8 + windows * case.order * 36 * 4 + 4
    k = max(4, (SEARCH_SCRATCH_CAP // per) & ~3)
    n_sub = 4 * case.n
    return -(-n_sub // min(k, n_sub))


def need_bytes(case):
    """Device memory a case takes at its peak: caller buffers, handle scratch as ensure grows it, the K base frames and
    their results (small), idx, and the comparison's chunk with the boolean it reduces."""
    total = 0
    for buf in buffers(case):
        total += grown(buf.nbytes) if buf.kind == "scratch" else buf.nbytes
    total += 8 * case.n + 3 * COMPARE_CHUNK
    total += K * max(1, case.channels) * (8 * padded(case.block) + 4 * 16928)
    return total


def seam_rows(case):
    """{(buffer, seam): (row, inside)} for every seam the case claims: `row` is the row of that buffer that holds the byte
    at the seam; inside is True when the seam lies strictly inside it (row start < seam < row end) and False when the row
    starts exactly at the seam (rows of a size that divides it).  Raises if the buffer does not reach the seam with one
    whole row beyond it."""
    bufs = {b.name: b for b in buffers(case)}
    out = {}
    for name, seam in case.seams:
        b, s = bufs[name], SEAMS[seam]
        row = s // b.stride_bytes
        start = row * b.stride_bytes
        if start + b.row_bytes <= s:  # the seam falls into the gap behind the row's data: the next row is the first beyond
            row, start = row + 1, start + b.stride_bytes
        inside = start < s
        if row >= b.rows or (inside and row + 1 >= b.rows):
            raise ValueError(f"{case.name}: {name} does not put a whole row beyond {seam}")
        out[(name, seam)] = (row, inside)
    return out


def seam_pins(case):
    """placement's pins: the frame of every seam row of a per-frame buffer is a special frame, and so are its
    neighbours on both sides where they lie in front of the last 16 positions."""
    bufs = {b.name: b for b in buffers(case)}
    sp = special_frames(case.bps)
    pins = {}
    rows = sorted(seam_rows(case).items())
    for d in (0, -1, 1):
        for i, ((name, _), (row, _)) in enumerate(rows):
            per = bufs[name].rows_per_frame
            if bufs[name].rows != case.n * per:
                continue  # a table that is not per frame (the base bytes of the decode case, the wasted-bits rows)
            f = row // per + d
            if f in pins or f < 16 + 2 * K or f >= case.n or (d and f >= case.n - 16):
                continue
            used = {v for p, v in pins.items() if p >= case.n - 16}
            pins[f] = next(v for v in sp[(i + d) % len(sp):] + sp if f < case.n - 16 or v not in used)
    return pins


def case_idx(case):
    return placement(case.n, K, seed=0xD1CE + case.n, pins=seam_pins(case), special=special_frames(case.bps))


def sparse_stride(seam_bytes, row_bytes, row, unit=16):
    """The row stride in bytes (a multiple of `unit`: 4 elements) that puts row `row` of a layout with the seam strictly
    inside it, as near to its middle as the unit allows: row * stride < seam < row * stride + row_bytes."""
    stride = ((seam_bytes - row_bytes // 2) // row) // unit * unit
    assert stride >= row_bytes and row * stride < seam_bytes < row * stride + row_bytes
    return stride


def aliases(offset, length, lead=LEAD):
    """Where a write to [offset, offset + length) of a buffer lands if its address was formed in fewer than 64 bits: the
    byte offset cut to 32 bits unsigned or signed, and the element index (offset / 4) cut likewise.  Intervals
    (start, end) relative to the pointer, inside [-lead, ...), the true place excluded."""
    out = set()
    for unit in (1, 4):
        o = offset // unit
        low = o & 0xFFFFFFFF
        for cand in (low, low - (1 << 32) if low >= (1 << 31) else low):
            at = cand * unit + offset % unit
            if at != offset and at >= -lead:
                out.add((at, at + length))
    return sorted(out)


def subtract(intervals, holes):
    """intervals minus holes, both lists of (start, end)."""
    out = []
    for s, e in intervals:
        parts = [(s, e)]
        for hs, he in holes:
            nxt = []
            for a, b in parts:
                if he <= a or hs >= b:
                    nxt.append((a, b))
                else:
                    if a < hs:
                        nxt.append((a, hs))
                    if he < b:
                        nxt.append((he, b))
            parts = nxt
        out += parts
    return out


def canary_regions_for(spans, lead=LEAD, guard=GUARD):
    """The sentinel regions around the byte spans (start, end) of a sparse buffer: `guard` bytes either side of every
    span and every alias of a span that ends beyond 2^31 bytes, minus the spans themselves.  (start, end) relative to
    the pointer."""
    regions = []
    for s, e in spans:
        regions += [(s - guard, s), (e, e + guard)]
        if e > S31:
            regions += aliases(s, e - s, lead)
    regions = [(max(s, -lead), e) for s, e in regions if e > -lead]
    return sorted(set(subtract(regions, spans)))


def canary_regions(n_rows, row_bytes, stride_bytes, lead=LEAD, guard=GUARD):
    """canary_regions_for n_rows rows of row_bytes at stride_bytes."""
    return canary_regions_for([(r * stride_bytes, r * stride_bytes + row_bytes) for r in range(n_rows)], lead, guard)


def straddling_offsets(lengths, slot, seam=S32, at=None):
    """Byte offsets for the frames of a table, `slot` bytes apart: the first half below the seam from 0 on, frame `at`
    (default the middle one) at seam - length / 2 so that its bytes straddle the seam, the rest above it."""
    n = len(lengths)
    at = n // 2 if at is None else at
    off = np.zeros(n, np.int64)
    for f in range(n):
        if f < at:
            off[f] = f * slot
        elif f == at:
            off[f] = seam - int(lengths[f]) // 2
        else:
            off[f] = seam + (f - at) * slot
    assert off[at] < seam < off[at] + int(lengths[at]) and off[at - 1] + slot <= off[at]
    return off


# ---------------------------------------------------------------------------------------------- checkers
def check_tiled(got, base, idx):
    """got [n, bytes] must equal base[idx] row for row -> None, or (frame, byte) of the first difference."""
    got = np.asarray(got).reshape(len(idx), -1)
    base = np.asarray(base).reshape(len(base), -1)
    step = max(1, COMPARE_CHUNK // max(1, got.shape[1]))
    for a in range(0, len(idx), step):
        bad = got[a:a + step] != base[idx[a:a + step]]
        if bad.any():
            f, byte = np.argwhere(bad)[0]
            return int(a + f), int(byte)
    return None


def check_canaries(buf, regions, lead=LEAD, sentinel=SENTINEL):
    """buf uint8 [..] whose element `lead` is the pointer's byte 0 -> None, or (region, byte offset from the pointer) of the
    first sentinel byte that changed."""
    buf = np.asarray(buf)
    for i, (s, e) in enumerate(regions):
        bad = np.flatnonzero(buf[lead + s:lead + e] != sentinel)
        if bad.size:
            return i, int(s + bad[0])
    return None


# ---------------------------------------------------------------------------------------------- the table
def _flags():
    from flacenc_rs_amd import _capi
    return _capi


def cases():
    """The dense tiled launches of tests/test_gpu_launch_scale.py."""
    F = _flags()
    REF, GEN, FP = F.FLAG_REFERENCE_SUM_ORDER, F.FLAG_GENERIC_KERNEL, F.FLAG_FUSED_PACK
    ep = {"encode_pack": True}
    out = [
        # the fused 4096 kernel: encode + pack in one kernel, in two launches, and the two-pass form
        Case("fused_pack 4096/16/8 past S31", "fused_pack", 2, 4096, 16, 8, FP, 98317, (("in", "S31"),), extra=ep),
        Case("fused_pack 4096/16/12 past S32", "fused_pack", 2, 4096, 16, 12, FP, 131101, (("in", "S32"),), extra=ep),
        Case("fused 4096/16/8 past S32", "fused", 2, 4096, 16, 8, 0, 131101, (("in", "S32"), ("residual", "S32"))),
        Case("fused 4096/16/12 past S31", "fused", 2, 4096, 16, 12, 0, 98317, (("in", "S31"), ("residual", "S31"))),
        Case("two-pass 4096/16/8 past S32", "two_pass", 2, 4096, 16, 8, REF, 131101,
             (("in", "S32"), ("residual", "S32"))),
        Case("certified 4608/16/10 past S31", "certified4608", 2, 4608, 16, 10, 0, 98317,
             (("in", "S31"), ("residual", "S31"))),
        # several frames per workgroup
        Case("sub-wave 1152/16/8", "subwave", 2, 1152, 16, 8, 0, 393241,
             (("in", "S31"), ("residual", "S31"), ("d_cresid", "S32"))),
        Case("sub-wave 576/24/6", "subwave", 2, 576, 24, 6, 0, 524309, (("in", "S31"), ("d_cresid", "S32"))),
        Case("sub-wave 256/16/8, 2^21 frames", "subwave", 2, 256, 16, 8, 0, 2097169,
             (("in", "S32"), ("residual", "S32"), ("d_cresid", "E31"))),
        # big blocks
        Case("big block 8192/24/24", "bigblock", 2, 8192, 24, 24, 0, 65551, (("in", "S32"), ("residual", "S32"))),
        Case("big block 16384/24/32", "bigblock", 2, 16384, 24, 32, 0, 32771, (("in", "S32"), ("residual", "S32"))),
        Case("big block 4096/16/16", "bigblock", 2, 4096, 16, 16, 0, 98317, (("in", "S31"), ("d_cresid", "S32"))),
        # the general route: four + four candidate rows per frame in handle scratch
        Case("general 4096 GENERIC_KERNEL scratch past S32", "general", 2, 4096, 16, 8, GEN, 98317,
             (("in", "S31"), ("d_cresid", "S32"), ("d_fresid", "S32"))),
        Case("general 4096 GENERIC_KERNEL scratch past E31", "general", 2, 4096, 16, 8, GEN, 131101,
             (("in", "S32"), ("d_cresid", "E31"), ("d_fresid", "E31"))),
        Case("general ragged 1000", "general", 2, 1000, 16, 8, 0, 134219, (("d_cresid", "S31"), ("d_fresid", "S31"))),
        # wasted bits: the marks list gets tens of thousands of entries
        Case("WASTED_BITS 4096/24/8", "wasted", 2, 4096, 24, 8, F.FLAG_WASTED_BITS, 98317,
             (("in", "S31"), ("residual", "S31")), extra={"wasted_frames": 98317 // 3}),
        # searches: at least 3 slices of the search scratch
        Case("ORDER_SEARCH|WINDOW_SEARCH 4096/16/12", "search", 2, 4096, 16, 12,
             F.FLAG_ORDER_SEARCH | F.FLAG_WINDOW_SEARCH, 49157, (("d_cresid", "S31"),)),
        Case("ORDER_GUESS 4096/16/12", "search", 2, 4096, 16, 12, F.FLAG_ORDER_GUESS, 49157, (("d_cresid", "S31"),)),
        Case("PRECISION_SEARCH 4096/16/8", "search", 2, 4096, 16, 8, F.FLAG_PRECISION_SEARCH, 49157, (("d_cresid", "S31"),)),
        Case("RICE_ESCAPE 4096/24/8", "search", 2, 4096, 24, 8, F.FLAG_RICE_ESCAPE, 49157, (("d_cresid", "S31"),)),
        Case("PRECISION_SEARCH|RICE_ESCAPE 4096/24/8", "search", 2, 4096, 24, 8,
             F.FLAG_PRECISION_SEARCH | F.FLAG_RICE_ESCAPE, 49157, (("d_cresid", "S31"),)),
        # Independent(n) frames: 262 147 rows and more
        Case("Independent(1) 4096/16/8", "channels", 1, 4096, 16, 8, 0, 262147, (("in", "S32"),), extra=ep),
        Case("Independent(3) 4096/16/8", "channels", 3, 4096, 16, 8, 0, 87383, (("in", "S32"),), extra=ep),
        Case("Independent(8) 4096/16/8", "channels", 8, 4096, 16, 8, 0, 32769, (("in", "S32"),), extra=ep),
        # the stand-alone packer at a stride of 64 KiB
        Case("packer out_stride 64 KiB", "packer", 2, 4096, 16, 8, 0, 98317, (("out", "S32"), ("in", "S31")),
             out_stride=64 << 10),
        # candidate batches, R[] and the unquantised coefficients wanted
        Case("qlpc batch 4096/16/8 with R[] and coefficients", "qlpc_batch", 0, 4096, 16, 8, 0, 262147,
             (("in", "S32"), ("residual", "S32")), extra={"want_fp": True}),
        Case("stereo qlpc batch 4096/16/8", "qlpc_batch", 0, 4096, 16, 8, 0, 262148,
             (("residual", "S32"),), extra={"stereo": True}),
        Case("fixed_lpc batch 4096/16", "fixed_batch", 0, 4096, 16, 8, 0, 262147, (("in", "S32"), ("residual", "S32"))),
        Case("stereo fixed_lpc batch 4096/16", "fixed_batch", 0, 4096, 16, 8, 0, 262148, (("residual", "S32"),),
             extra={"stereo": True}),
        # the way back
        Case("decode / verify 4096", "decode", 2, 4096, 16, 8, 0, 131101, (("out", "S32"),)),
    ]
    return out


def case(name):
    for c in cases():
        if c.name == name:
            return c
    raise KeyError(name)
