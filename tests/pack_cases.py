"""Hand-built decision records for the frame packers (frame_pack_kernel / channel_pack_kernel behind
flacenc_hip_pack_stereo_frames and flacenc_hip_pack_frames), with the frame each of them must become.  Nothing here comes
from the project's encoder: a PackCase is the decoded channels, the stream's bits per sample, the channel assignment and,
per output channel, a subframe description in the keywords of flac_write.write_subframe with an explicit Rice partition
order and explicit parameters.  From a case follow
  * the expected frame, written by tests/flac_write.py from RFC 9639 (expected()), and
  * the packer's inputs (record(), residual_rows(), samples()): a FRAME_RESULT_DTYPE or CHANNEL_RESULT_DTYPE record, the
    residual rows = flac_write.residuals of the role's signal >> wasted with the warm-up slots zero, and the input rows.
tests/test_pack_cases_cpu.py holds both to flac_parse and to the oracle's restatement of Frame::write before a GPU sees
a record; tests/test_gpu_pack_records.py packs them.

The packer's domain (check_domain asserts every line for every case; a case outside it is a bug of this generator):
  * the record describes a subframe the project's decoder reads;
  * order <= block_size >> rice_order (the first partition may be empty, never negative);
  * Rice parameters 0..30, no escape codes; RICE2 (5-bit parameters) exactly when some parameter exceeds 14;
  * shift 0..15, precision 1..15 (LPC), Fixed orders 0..4 with FIXED_LPC_COEFS, shift 0 and precision 0;
  * every sample fits its width (bits_per_sample, + 1 for the side role, - wasted), every residual fits an int32;
  * the frame's subframe bits sum to at most channels * (8 + n * bits_per_sample): the packer's LDS image is sized from
    flacenc_hip_*_frame_bytes_bound, so a larger frame would be written outside it.  (That excludes the corner25 frames of
    decode_cases as they stand -- about 6.7 kbit in a 4.9 kbit image -- so family E rebuilds them with a silent tail.)

path(n, porder) restates which of the packer's residual paths a subframe takes; groups() sorts the cases into launches
(one entry point, channel count, block size, bits per sample, sample rate and frame-number sequence each)."""
import collections
import functools

import numpy as np

import decode_cases as dc
import flac_write as fw
from flacenc_rs_amd import _capi

KIND = {"constant": 0, "verbatim": 1, "fixed": 2, "lpc": 3}
ROLES = {0: (0, 1), 1: (0, 3), 2: (3, 1), 3: (2, 3)}      # select_channels: (L,R), (L,S), (S,R), (M,S)
STEREO_TAG = {0: 1, 1: 8, 2: 9, 3: 10}
FIXED_LPC_COEFS = [[0, 0, 0, 0], [1, 0, 0, 0], [2, -1, 0, 0], [3, -3, 1, 0], [4, -6, 4, -1]]
PACK_THREADS = 256
LDS_LIMIT = 150 * 1024
KNOWN_RATES = {88200: 1, 176400: 2, 192000: 3, 8000: 4, 16000: 5, 22050: 6, 24000: 7, 32000: 8, 44100: 9, 48000: 10,
               96000: 11}


class PackCase:
    """name, family (A..I), x int64 [nch, n], bps, stereo (a FRAME_RESULT record; else CHANNEL_RESULT records),
    assignment 0..3, subs (per output channel the write_subframe keywords, all explicit), edges (the listed edges this
    case is there for)."""

    def __init__(self, name, family, x, bps, subs, assignment=0, stereo=True, edges=()):
        self.name, self.family, self.bps, self.assignment, self.stereo = name, family, bps, assignment, stereo
        self.x = np.asarray(x, np.int64)
        self.subs = [_explicit(dict(s)) for s in subs]
        self.edges = set(edges)
        assert self.x.ndim == 2 and len(self.subs) == self.x.shape[0] and (not stereo or self.x.shape[0] == 2)
        assert stereo or assignment == 0

    @property
    def n(self):
        return self.x.shape[1]

    @property
    def channels(self):
        return self.x.shape[0]

    @property
    def tag(self):
        return STEREO_TAG[self.assignment] if self.stereo else self.channels - 1

    def __repr__(self):
        return "PackCase(%s)" % self.name


def _explicit(sf):
    for k, v in dict(order=0, coefs=None, precision=0, shift=0, wasted=0, method=0, porder=0, params=None).items():
        sf.setdefault(k, v)
    return sf


# ---------------------------------------------------------------- what a case says about its subframes
def roles(case):
    return ROLES[case.assignment] if case.stereo else (0,) * case.channels


def coded_signals(case):
    """Per output channel (the signal the subframe codes, its width): L, R, M = (l + r) >> 1, S = l - r at bps + 1."""
    if not case.stereo:
        return [(case.x[c], case.bps) for c in range(case.channels)]
    l, r = case.x
    sig = (l, r, (l + r) >> 1, l - r)
    return [(sig[role], case.bps + (1 if role == 3 else 0)) for role in roles(case)]


def path(n, porder):
    """The residual path of a Fixed / LPC subframe, as frame_pack_body chooses it."""
    part_len = n >> porder
    if n % 4096 == 0:
        return "aligned"                                    # the ALIGNED instance: rice_runs16 only
    if n % 16 == 0 and part_len % 16 == 0:
        return "runs"                                       # rice_runs16 inside the general instance
    per = (n + PACK_THREADS - 1) // PACK_THREADS            # the per-sample walk over a slice of `per` samples
    return "walk cached" if per <= 16 else "walk uncached"


def paths(case):
    return [path(case.n, sf["porder"]) if sf["kind"] in ("fixed", "lpc") else None for sf in case.subs]


def shifted_residual(case, c):
    """The residual row of output channel c: of the role's signal >> wasted, warm-up slots zero (int64)."""
    sf = case.subs[c]
    if sf["kind"] not in ("fixed", "lpc"):
        return np.zeros(case.n, np.int64)
    sig, _ = coded_signals(case)[c]
    coefs = fw.FIXED_COEFS[sf["order"]] if sf["kind"] == "fixed" else sf["coefs"]
    return fw.residuals(sig >> sf["wasted"], coefs, sf["shift"], sf["order"])


def subframe_bit_list(case, c):
    """The bits of subframe c written alone (flac_write.write_subframe on an empty BitWriter)."""
    cache = case.__dict__.setdefault("_bits", {})
    if c not in cache:
        sig, w = coded_signals(case)[c]
        bw = fw.BitWriter()
        fw.write_subframe(bw, sig, w, **case.subs[c])
        cache[c] = bw.bits
    return cache[c]


def rate_header(rate):
    """flac_write.header's sample-rate keywords for `rate` (RFC 9639 section 9.1.2), with the reference's preference: a
    tabulated rate, else kHz in 8 bits, else tens of Hz in 16 bits, else Hz in 16 bits, else 0 = "from STREAMINFO"."""
    if rate in KNOWN_RATES:
        return dict(sr_code=KNOWN_RATES[rate])
    if rate and rate % 1000 == 0 and rate // 1000 <= 255:
        return dict(sr_code=12, sr_value=rate // 1000)
    if rate and rate % 10 == 0 and rate // 10 <= 65535:
        return dict(sr_code=14, sr_value=rate // 10)
    if rate and rate <= 65535:
        return dict(sr_code=13, sr_value=rate)
    return dict(sr_code=0)


def expected(case, number, rate=44100):
    """The frame, by flac_write alone."""
    return fw.frame(case.x, case.tag, case.bps, case.subs, number=number, **rate_header(rate))


def expected_body(case):
    """The subframes' bytes from the first subframe bit to the padding (the frame without header and CRC-16); the
    subframes start on a byte, so this is independent of the header."""
    bw = fw.BitWriter()
    for c in range(case.channels):
        bw.bits.extend(subframe_bit_list(case, c))
    bw.align()
    return bw.bytes()


# ---------------------------------------------------------------- the packer's inputs
def _params_record(case, c):
    sf = case.subs[c]
    p = np.zeros((), _capi.PARAMS_DTYPE)
    if sf["kind"] not in ("fixed", "lpc"):
        return p
    _, w = coded_signals(case)[c]
    w -= sf["wasted"]
    order = sf["order"]
    if sf["kind"] == "fixed":
        p["coefs"][:4] = FIXED_LPC_COEFS[order]
        head = 8 + order * w
    else:
        p["coefs"][:order] = sf["coefs"]
        p["shift"], p["precision"] = sf["shift"], sf["precision"]
        head = 8 + order * w + 9 + order * sf["precision"]
    p["order"], p["rice_order"] = order, sf["porder"]
    p["rice_params"][:1 << sf["porder"]] = sf["params"]
    bits = len(subframe_bit_list(case, c)) - sf["wasted"]
    p["subframe_bits"], p["code_bits"] = bits, bits - head
    e = shifted_residual(case, c)
    u = np.where(e < 0, -2 * e - 1, 2 * e)
    per = np.repeat(np.asarray(sf["params"], np.int64), case.n >> sf["porder"])
    p["sum_quotients"] = int((u >> per)[order:].sum())
    return p


def record(case):
    """FRAME_RESULT_DTYPE [] for a stereo case, CHANNEL_RESULT_DTYPE [channels] otherwise."""
    sigs = coded_signals(case)
    if case.stereo:
        r = np.zeros((), _capi.FRAME_RESULT_DTYPE)
        r["channel_assignment"] = case.assignment
        for c, sf in enumerate(case.subs):
            r["role"][c] = roles(case)[c]
            r["kind"][c] = KIND[sf["kind"]]
            r["pad"][c] = sf["wasted"]
            r["dc_offset"][c] = int(sigs[c][0][0]) >> sf["wasted"] if sf["kind"] == "constant" else 0
            r["bits"][roles(case)[c]] = len(subframe_bit_list(case, c))
            r["lpc"][c] = _params_record(case, c)
        return r
    r = np.zeros(case.channels, _capi.CHANNEL_RESULT_DTYPE)
    for c, sf in enumerate(case.subs):
        r[c]["kind"] = KIND[sf["kind"]]
        r[c]["pad"][0] = sf["wasted"]
        r[c]["dc_offset"] = int(sigs[c][0][0]) >> sf["wasted"] if sf["kind"] == "constant" else 0
        r[c]["bits"] = len(subframe_bit_list(case, c))
        r[c]["params"] = _params_record(case, c)
    return r


def residual_rows(case):
    e = np.stack([shifted_residual(case, c) for c in range(case.channels)])
    assert e.min() >= -(1 << 31) and e.max() < (1 << 31)
    return e.astype(np.int32)


def samples(case):
    return case.x.astype(np.int32)


def lds_bytes(case):
    """The LDS image enqueue_pack asks for: the entry point's bytes bound (a multiple of 16) + 4 words."""
    n, bps = case.n, case.bps
    bits = 2 * 8 + n * (2 * bps + 1) if case.stereo else case.channels * (8 + n * bps)
    bound = 15 + (bits + 7) // 8 + 2
    return (bound + 15) // 16 * 16 + 16


def check_domain(case):
    """Every condition of the module docstring, on the CPU."""
    n, total = case.n, 0
    assert 1 <= n <= 32768 and 8 <= case.bps <= 24 and 1 <= case.channels <= 8, case
    assert lds_bytes(case) <= LDS_LIMIT, case
    for c, sf in enumerate(case.subs):
        sig, w = coded_signals(case)[c]
        k = sf["wasted"]
        assert 0 <= k < w and not (sig & ((1 << k) - 1)).any(), (case, c)
        w -= k
        assert (sig >> k).min() >= -(1 << (w - 1)) and (sig >> k).max() < (1 << (w - 1)), (case, c, w)
        assert sf["kind"] in KIND, case
        if sf["kind"] == "constant":
            assert (sig == sig[0]).all(), (case, c)
        if sf["kind"] in ("fixed", "lpc"):
            order, porder, params = sf["order"], sf["porder"], sf["params"]
            assert 0 <= porder <= 8 and n % (1 << porder) == 0 and order <= n >> porder, (case, c)
            assert len(params) == 1 << porder and all(isinstance(p, int) and 0 <= p <= 30 for p in params), (case, c)
            assert sf["method"] == (1 if max(params) > 14 else 0), (case, c)
            if sf["kind"] == "fixed":
                assert 0 <= order <= 4 and sf["shift"] == 0 and sf["precision"] == 0
            else:
                assert 1 <= order <= 32 and 0 <= sf["shift"] <= 15 and 1 <= sf["precision"] <= 15, (case, c)
                lim = 1 << (sf["precision"] - 1)
                assert len(sf["coefs"]) == order and all(-lim <= v < lim for v in sf["coefs"]), (case, c)
            e = shifted_residual(case, c)
            assert e.min() >= -(1 << 31) and e.max() < (1 << 31), (case, c)
        total += len(subframe_bit_list(case, c))
    assert total <= case.channels * (8 + n * case.bps), (case, total, case.channels * (8 + n * case.bps))


# ---------------------------------------------------------------- signals and parameters
def tone(rng, n, bps, amp=0.5, noise=0.002):
    """A sine with a little noise: every predictor here leaves a residual well below the sample width."""
    hi = (1 << (bps - 1)) - 1
    t = np.arange(n)
    x = amp * np.sin(2 * np.pi * t / rng.uniform(40, 200) + rng.uniform(0, 6)) + noise * rng.standard_normal(n)
    return np.clip(np.round(x * hi), -hi - 1, hi).astype(np.int64)


def partition_slices(n, order, porder):
    psize = n >> porder
    return [slice(max(order, q * psize), (q + 1) * psize) for q in range(1 << porder)]


def choose_params(e, n, order, porder, limit=14, perturb=True):
    """flac_write.best_param per partition, then deliberately off the optimum: + 1 on partitions 1 mod 3, - 1 on
    partitions 2 mod 3 (so the packer is not only shown the parameters a search would pick)."""
    out = []
    for q, s in enumerate(partition_slices(n, order, porder)):
        p = min(limit, fw.best_param(e[s], 1))
        if perturb:
            p = min(limit, p + 1) if q % 3 == 1 else max(0, p - 1) if q % 3 == 2 else p
        out.append(int(p))
    return out


def coded(sig, kind, order=0, porder=0, wasted=0, coefs=None, precision=0, shift=0, params=None, limit=14,
          perturb=True):
    """A complete subframe description of `sig` (the role's signal); parameters chosen from its residual unless
    given."""
    if kind in ("constant", "verbatim"):
        return dict(kind=kind, wasted=wasted)
    c = fw.FIXED_COEFS[order] if kind == "fixed" else coefs
    if params is None:
        e = fw.residuals(np.asarray(sig, np.int64) >> wasted, c, shift, order)
        params = choose_params(e, len(sig), order, porder, limit, perturb)
        if order == len(sig) >> porder:
            params[0] = 5                   # an empty first partition still has a parameter: one that shows
    sf = dict(kind=kind, order=order, porder=porder, wasted=wasted, params=[int(p) for p in params],
              method=1 if max(params) > 14 else 0)
    if kind == "lpc":
        sf.update(coefs=[int(v) for v in coefs], precision=precision, shift=shift)
    return sf


def small_lpc(rng, order, precision=12):
    """A decaying first coefficient, the rest small (test_decode_core_cpu.lpc_coefs)."""
    coefs, shift = dc.corpora.lpc_coefs(rng, order, precision)
    return dict(coefs=[int(v) for v in coefs], precision=precision, shift=int(shift))


def stereo_pair(rng, n, bps, assignment=0):
    """Two tones a little apart; with a side role the pair keeps l - r small.  Above 16 bits the tones keep their 16-bit
    size (times 5: 19 bits with every low bit in use), so that the residuals stay below the sample width."""
    scale = 5 if bps > 16 else 1
    bps = min(bps, 16)
    l = tone(rng, n, bps, amp=0.45)
    r = l // 2 + tone(rng, n, bps, amp=0.2) if assignment else tone(rng, n, bps, amp=0.45)
    return np.stack([l, r]) * scale


def stereo_case(name, family, rng, n, bps, assignment, spec0, spec1, edges=(), x=None):
    """spec = dict(kind, order, porder, ...) without parameters: they are chosen from the role's residual."""
    x = stereo_pair(rng, n, bps, assignment) if x is None else np.asarray(x, np.int64)
    tmp = PackCase(name, family, x, bps, [dict(kind="verbatim")] * 2, assignment)
    subs = []
    for (sig, _), spec in zip(coded_signals(tmp), (spec0, spec1)):
        spec = dict(spec)
        if spec["kind"] == "lpc" and "coefs" not in spec:
            spec.update(small_lpc(rng, spec["order"], spec.pop("precision", 12)))
        subs.append(coded(sig, **spec))
    return PackCase(name, family, x, bps, subs, assignment, edges=edges)


# ---------------------------------------------------------------- the families
@functools.lru_cache(None)
def family_a():
    """The ALIGNED instance: n = 4096 (16 bits) and 8192 (24 bits)."""
    rng = np.random.default_rng(0xA11)
    out = []
    for p in range(9):
        s0 = dict(kind="lpc", order=8, porder=p) if p % 2 else dict(kind="fixed", order=2, porder=p)
        s1 = dict(kind="fixed", order=3, porder=8 - p) if p % 2 else dict(kind="lpc", order=6, porder=8 - p)
        out.append(stereo_case("A 4096 porder %d/%d" % (p, 8 - p), "A", rng, 4096, 16, p % 4, s0, s1,
                               edges={"A slot0 porder %d" % p, "A slot1 porder %d" % (8 - p)}))
    for i, (porder, order) in enumerate([(8, 1), (8, 15), (8, 16), (7, 17), (7, 31), (7, 32)]):
        s = dict(kind="lpc", order=order, porder=porder)
        other = dict(kind="fixed", order=i % 5, porder=(3, 8)[i % 2])
        specs = (s, other) if i % 2 == 0 else (other, s)
        edges = {"A order %d porder %d" % (order, porder)}
        if order == 4096 >> porder:
            edges.add("order == part_len aligned")
        if order == (4096 >> porder) - 1:
            edges.add("order == part_len - 1 aligned")
        out.append(stereo_case("A 4096 order %d porder %d" % (order, porder), "A", rng, 4096, 16, i % 4, *specs,
                               edges=edges))
    for i, (p0, p1) in enumerate([(0, 1), (1, 8), (8, 0)]):
        out.append(stereo_case("A 8192 porder %d/%d" % (p0, p1), "A", rng, 8192, 24, (0, 3, 1)[i],
                               dict(kind="lpc", order=12, porder=p0, precision=15), dict(kind="fixed", order=4, porder=p1),
                               edges={"A 8192 porder %d" % p0, "A 8192 porder %d" % p1}))
    return out


@functools.lru_cache(None)
def family_b():
    """Aligned runs inside the general instance: n and n >> porder multiples of 16, n no multiple of 4096."""
    rng = np.random.default_rng(0xB22)
    out = []
    for n, top in ((4608, 6), (1152, 4)):
        for p in range(top):
            q = (p + top // 2) % top
            out.append(stereo_case("B %d porder %d/%d" % (n, p, q), "B", rng, n, 16, p % 4,
                                   dict(kind="lpc", order=4 + 3 * p, porder=p), dict(kind="fixed", order=p % 5, porder=q),
                                   edges={"B %d porder %d" % (n, p)}))
    out.append(stereo_case("B 48 porder 0", "B", rng, 48, 16, 1, dict(kind="lpc", order=3, porder=0),
                           dict(kind="fixed", order=4, porder=0), edges={"B 48 porder 0"}))
    out.append(stereo_case("B 32 porder 1 order 16", "B", rng, 32, 16, 0, dict(kind="lpc", order=16, porder=1, precision=6),
                           dict(kind="fixed", order=1, porder=1), edges={"B 32 order 16", "order == part_len runs"}))
    for order in (15, 16):
        x = stereo_pair(rng, 16, 16)
        x[order % 2] = int(x[0, 3])         # the channel of the Constant subframe
        specs = [dict(kind="lpc", order=order, porder=0, precision=5), dict(kind="constant")]
        edges = {"B 16 order %d" % order} | ({"order == part_len runs", "order == n"} if order == 16 else
                                             {"order == part_len - 1 runs"})
        out.append(stereo_case("B 16 order %d" % order, "B", rng, 16, 16, 0, *(specs if order % 2 else specs[::-1]),
                               edges=edges, x=x))
    return out


@functools.lru_cache(None)
def family_c():
    """The per-sample walk on blocks up to 4096 samples (zig-zag codes cached in registers), and 4608 with partitions
    that are no multiple of 16 (18 samples per thread: the walk re-reads the residual row)."""
    rng = np.random.default_rng(0xC33)
    out = []
    for i, p in enumerate((6, 7, 8)):
        out.append(stereo_case("C 4608 porder %d" % p, "C", rng, 4608, 16, i, dict(kind="lpc", order=5 + i, porder=p),
                               dict(kind="fixed", order=2 + i, porder=p), edges={"C 4608 porder %d" % p}))
    for p in range(4):
        out.append(stereo_case("C 1000 porder %d" % p, "C", rng, 1000, 16, 3 - p, dict(kind="fixed", order=p + 1, porder=p),
                               dict(kind="lpc", order=9 + p, porder=3 - p), edges={"C 1000 porder %d" % p}))
    for i, order in enumerate((1, 24, 25)):
        edges = {"C 100 order %d" % order} | ({"order == part_len walk"} if order == 25 else
                                              {"order == part_len - 1 walk"} if order == 24 else set())
        s = dict(kind="lpc", order=order, porder=2, precision=8)
        other = dict(kind="fixed", order=i + 1, porder=2)
        out.append(stereo_case("C 100 porder 2 order %d" % order, "C", rng, 100, 16, i,
                               *((s, other) if i % 2 == 0 else (other, s)), edges=edges))
    out.append(stereo_case("C 40 porder 1 order 20", "C", rng, 40, 16, 0, dict(kind="lpc", order=20, porder=1, precision=3),
                           dict(kind="fixed", order=1, porder=1),
                           edges={"C 40 order 20", "order == part_len walk"}))
    x = stereo_pair(rng, 25, 16)
    x[1] = -1234
    out.append(stereo_case("C 25 porder 0 order 25", "C", rng, 25, 16, 0, dict(kind="lpc", order=25, porder=0, precision=2),
                           dict(kind="constant"), edges={"order == part_len walk", "order == n"}, x=x))
    out.append(stereo_case("C 4095 porder 0", "C", rng, 4095, 16, 2, dict(kind="lpc", order=32, porder=0),
                           dict(kind="fixed", order=4, porder=0), edges={"C 4095 porder 0"}))
    return out


@functools.lru_cache(None)
def family_d():
    """The walk on blocks above 4096 samples (more than 16 samples per thread)."""
    rng = np.random.default_rng(0xD44)
    out = []
    for i, (n, p) in enumerate([(4097, 0), (6000, 4), (20000, 5), (32767, 0)]):
        out.append(stereo_case("D %d porder %d" % (n, p), "D", rng, n, 16, i, dict(kind="lpc", order=7 + 8 * i, porder=p),
                               dict(kind="fixed", order=i + 1, porder=p), edges={"D %d porder %d" % (n, p)}))
    return out


E_KINDS = ("constant", "verbatim", "fixed", "lpc")


@functools.lru_cache(None)
def family_e():
    """Frames whose two subframes take different paths; every assignment with every pair of kinds (Fixed orders cycle
    through 0..4); the corner25 construction of decode_cases (25-bit side, order 32, precision 15, shifts 0..15, the three
    coefficient sign patterns) with a silent tail that brings the frame inside the bit bound."""
    rng = np.random.default_rng(0xE55)
    out = []
    for i, (n, p0, p1) in enumerate([(4608, 6, 2), (4608, 2, 6), (192, 3, 1), (192, 1, 3)]):   # 72 / 1152, 24 / 96
        out.append(stereo_case("E %d porder %d/%d" % (n, p0, p1), "E", rng, n, 16, 1 + i % 2,
                               dict(kind="lpc", order=10, porder=p0), dict(kind="lpc", order=3, porder=p1),
                               edges={"E %d %s" % (n, "walk then runs" if p0 > p1 else "runs then walk")}))
    k = 0
    for assignment in range(4):
        for k0 in E_KINDS:
            for k1 in E_KINDS:
                n = (192, 100)[k % 2]
                x = stereo_pair(rng, n, 16, assignment)
                # a Constant subframe needs a constant role signal
                if assignment:
                    x >>= 4            # next to a Verbatim side role of bps + 1 bits the other subframe must be short
                const = [k0 == "constant", k1 == "constant"]
                if any(const):
                    x = _with_constant_roles(x, assignment, const, rng)
                specs = []
                for c, kind in enumerate((k0, k1)):
                    porder = (k + c) % 4 if n == 192 else (k + c) % 3
                    specs.append(dict(kind=kind, order=(k + c) % 5 if kind == "fixed" else 1 + (3 * k + c) % 12,
                                      porder=porder) if kind in ("fixed", "lpc") else dict(kind=kind))
                if assignment and k0 == k1 == "verbatim":
                    x = x >> 3 << 3    # two Verbatim subframes and a side role: the other one drops two wasted bits
                    specs[1 if assignment == 2 else 0]["wasted"] = 2
                out.append(stereo_case("E a%d %s/%s" % (assignment, k0, k1), "E", rng, n, 16, assignment, *specs,
                                       edges={"E a%d %s/%s" % (assignment, k0, k1)}, x=x))
                k += 1
    for shift in range(16):
        pat = ("alt", "pos", "neg")[shift % 3]
        n = 256
        left = np.zeros(n, np.int64)
        left[:64] = dc.full_scale(rng, 64, 24, pat)
        right = np.zeros(n, np.int64)
        right[:64] = -1 - left[:64]
        right[:64:7] = left[:64:7]
        side = left - right
        assert side.max() == (1 << 24) - 1 and side.min() == -(1 << 24) + 1
        subs = []
        for sig in (left, side):
            sf, _ = dc.corner_subframe(sig, pat, shift)
            sf.pop("method")
            subs.append(coded(sig, porder=2, limit=30, perturb=False, **sf))
        out.append(PackCase("E corner25 %s shift %d" % (pat, shift), "E", np.stack([left, right]), 24, subs, 1,
                            edges={"E corner25 shift %d" % shift, "E corner25 %s" % pat}))
    return out


def _with_constant_roles(x, assignment, const, rng):
    """Stereo channels whose output channel c codes a constant signal wherever const[c]."""
    l, r = x[0].copy(), x[1].copy()
    v0, v1 = (int(v) for v in rng.integers(-900, 900, 2))
    odd = np.arange(len(l)) & 1
    if assignment == 0:                       # (L, R)
        l = np.full_like(l, v0) if const[0] else l
        r = np.full_like(r, v1) if const[1] else r
    elif assignment == 1:                     # (L, S): S = l - r
        l = np.full_like(l, v0) if const[0] else l
        r = l - v1 if const[1] else r
    elif assignment == 2:                     # (S, R)
        r = np.full_like(r, v1) if const[1] else r
        l = r + v0 if const[0] else l
    elif all(const):                          # (M, S)
        l, r = np.full_like(l, v0), np.full_like(r, v1)
    elif const[0]:                            # M = (l + r) >> 1 = v0 whatever the side's low bit
        r = 2 * v0 - l + odd
    else:
        r = l - v1
    return np.stack([l, r])


F_SHAPES = ((4096, 8), (1152, 3), (1000, 3), (6000, 4))    # aligned, runs, cached walk, uncached walk


@functools.lru_cache(None)
def family_f():
    """Parameters: all <= 14 with a 14; RICE2 by one partition (first, middle, last); parameter 30; parameter 0 under
    quotients of several hundred; residuals INT32_MIN and INT32_MAX at parameter 30; precision 1.  24-bit stereo."""
    rng = np.random.default_rng(0xF66)
    out = []
    for n, porder in F_SHAPES:
        nparts, psize = 1 << porder, n >> porder
        where = path(n, porder)

        def fixed2(x):
            return fw.residuals(x, fw.FIXED_COEFS[2], 0, 2)

        def quiet_pair():                                   # residuals of some 9 bits: every parameter far below 14
            return np.stack([tone(rng, n, 24, amp=0.002, noise=0.00002) for _ in range(2)])

        # -- all <= 14, one partition at 14 (a burst of 15-bit residuals), method 0
        x = quiet_pair()
        x[0, 3 * psize + 2:4 * psize:2] += 1 << 13
        p0 = choose_params(fixed2(x[0]), n, 2, porder)
        p0[3] = 14
        s0 = coded(x[0], "fixed", 2, porder, params=p0)
        s1 = coded(x[1], "fixed", 1, porder)
        assert s0["method"] == 0 and s1["method"] == 0
        out.append(PackCase("F %d max 14" % n, "F", x, 24, [s0, s1], edges={"F all <= 14 %s" % where}))
        # -- RICE2 because of one partition: the first and the middle one (slot 0, slot 1), then the last one
        for tag, qs in (("first/middle", (0, nparts // 2)), ("last", (nparts - 1, nparts - 1))):
            x = quiet_pair()
            subs = []
            for c, q in enumerate(qs):
                ps = choose_params(fixed2(x[c]), n, 2, porder)
                assert max(ps) <= 14
                ps[q] = 15
                subs.append(coded(x[c], "fixed", 2, porder, params=ps))
            out.append(PackCase("F %d rice2 %s" % (n, tag), "F", x, 24, subs,
                                edges={"F rice2 by one partition %s" % where} |
                                ({"F rice2 by the last of 256"} if nparts == 256 and tag == "last" else set())))
        # -- parameter 30 on one partition, parameter 0 under quotients of several hundred on another
        x = quiet_pair()
        ps = choose_params(fixed2(x[0]), n, 2, porder, perturb=False)
        ps[1] = 30
        s0 = coded(x[0], "fixed", 2, porder, params=ps)
        x[1] = rng.integers(-3, 4, n)                       # Fixed order 0: the residual is the signal
        lo, burst = 2 * psize, min(psize, 24)
        x[1, lo:lo + burst] = rng.integers(150, 400, burst) * rng.choice([-1, 1], burst)
        ps = choose_params(x[1], n, 0, porder, perturb=False)
        ps[2] = 0
        assert int(np.abs(x[1, lo:lo + psize]).max()) >= 300
        s1 = coded(x[1], "fixed", 0, porder, params=ps)
        out.append(PackCase("F %d param 30 and long unary" % n, "F", x, 24, [s0, s1],
                            edges={"F parameter 30 %s" % where, "F long unary %s" % where}))
        # -- the ends of the int32 range at parameter 30: e = x[t] + 16384 x[t-1] (order 1, precision 15, shift 0)
        x = np.zeros((2, n), np.int64)
        t0 = psize + 3
        x[0, t0 - 1], x[0, t0] = 1 << 17, -1                   # e[t0] = 2^31 - 1
        x[0, t0 + 4], x[0, t0 + 5] = -(1 << 17), 0             # e[t0 + 5] = -2^31
        x[1] = tone(rng, n, 24, amp=0.002, noise=0.00002) * (1 - 2 * (np.arange(n) & 1))
        e0 = fw.residuals(x[0], [-16384], 0, 1)
        assert e0.max() == (1 << 31) - 1 and e0.min() == -(1 << 31)
        ps = choose_params(e0, n, 1, porder, perturb=False)
        ps[1] = 30
        s0 = coded(x[0], "lpc", 1, porder, coefs=[-16384], precision=15, shift=0, params=ps)
        # -- precision 1: coefficients -1 and 0, a signal that alternates in sign
        s1 = coded(x[1], "lpc", 2, porder, coefs=[-1, 0], precision=1, shift=0)
        out.append(PackCase("F %d int32 ends and precision 1" % n, "F", x, 24, [s0, s1],
                            edges={"F int32 ends %s" % where, "F precision 1 %s" % where}))
    return out


@functools.lru_cache(None)
def family_g():
    """Wasted bits k = 1, 8 and w - 2 next to each kind, and on the side role (w = bps + 1)."""
    rng = np.random.default_rng(0x677)
    out = []
    i = 0
    for kind in E_KINDS:
        for k in (1, 8, 14):
            n = (192, 100, 4096)[i % 3]
            x = stereo_pair(rng, n, 16)
            x[0] = x[0] >> k << k
            if kind == "constant":
                x[0] = (-3 if k < 14 else -1) << k
            spec = dict(kind=kind, wasted=k)
            if kind in ("fixed", "lpc"):
                spec.update(order=(i % 4 + 1) if kind == "fixed" else 6, porder=i % 3)
            other = dict(kind="verbatim") if i % 4 < 2 else dict(kind="fixed", order=2, porder=1)
            specs = (spec, other)
            if i % 2:
                x, specs = x[::-1].copy(), specs[::-1]
            out.append(stereo_case("G %s wasted %d" % (kind, k), "G", rng, n, 16, 0, *specs,
                                   edges={"G %s wasted %d" % (kind, k)}, x=x))
            i += 1
    for j, k in enumerate((1, 8, 15)):                  # the side role: w = 17
        n = (100, 192, 4096)[j]
        l = tone(rng, n, 16, amp=0.4)
        if k < 15:
            s = tone(rng, n, 17, amp=0.2) >> k << k
        else:                                               # side values -1, 0, 1 at two bits: r = l - s stays in range
            s = np.where(l < 0, -1, rng.integers(0, 2, n)) << 15
        r = l - s
        assert r.min() >= -(1 << 15) and r.max() < (1 << 15)
        kind = ("lpc", "fixed", "verbatim")[j]
        spec = dict(kind=kind, wasted=k)
        if kind != "verbatim":
            spec.update(order=3, porder=2)
        out.append(stereo_case("G side wasted %d" % k, "G", rng, n, 16, 1, dict(kind="lpc", order=4, porder=1), spec,
                               edges={"G side wasted %d" % k}, x=np.stack([l, r])))
    return out


@functools.lru_cache(None)
def family_h():
    """Independent frames (CHANNEL_RESULT records, flacenc_hip_pack_frames): 1, 3 and 8 channels."""
    rng = np.random.default_rng(0x488)
    out = []
    i = 0
    for channels in (1, 3, 8):
        for n in (4096, 576, 97):
            for rep in range(2):
                x = np.stack([tone(rng, n, 16, amp=0.12) for _ in range(channels)])
                subs = []
                for c in range(channels):
                    kind = E_KINDS[(i + c + rep) % 4] if channels > 1 else ("lpc", "fixed")[rep]
                    top = 8 if n == 4096 else 6 if n == 576 else 0
                    porder = (3 * i + 5 * c + rep) % (top + 1)
                    wasted = 3 if (c == 1 and kind != "constant") else 0
                    if wasted:
                        x[c] = x[c] >> wasted << wasted
                    if kind == "constant":
                        x[c] = int(x[c, 0])
                    order = min(1 + (7 * i + 3 * c) % 32, n >> porder)
                    if kind == "fixed":
                        subs.append(coded(x[c], "fixed", (i + c) % 5, porder, wasted))
                    elif kind == "lpc":
                        subs.append(coded(x[c], "lpc", order, porder, wasted, **small_lpc(rng, order, 8)))
                    else:
                        subs.append(dict(kind=kind, wasted=wasted))
                out.append(PackCase("H %dch %d #%d" % (channels, n, rep), "H", x, 16, subs, stereo=False,
                                    edges={"H %dch %d" % (channels, n)}))
                i += 1
    return out


# every tabulated block size that the entry points take (FLACENC_HIP_MAX_BLOCK_SIZE is 32767: 32768 is refused)
I_BLOCK_SIZES = sorted(set(fw.BS_CODES) - {32768}) + [1, 2, 255, 257, 4095, 32767]
I_RATES = sorted(KNOWN_RATES) + [255000, 256000, 65535, 65536, 655350, 655360, 1]
I_DEPTHS = [8, 12, 16, 20, 24, 14]
I_BOUNDARIES = [128, 2048, 65536, 1 << 21, 1 << 26]
# (first, step, frames): three frames around each boundary, a step that jumps it, a launch that ends at 2^31 - 1
I_NUMBERS = [(b - 1, 1, 3) for b in I_BOUNDARIES] + [(b - 5, 9, 2) for b in I_BOUNDARIES] + [((1 << 31) - 3, 1, 3)]

Launch = collections.namedtuple("Launch", "name stereo channels n bps rate first step cases")


@functools.lru_cache(None)
def family_i():
    """Constant-only frames for the header: every block-size code and the uncoded sizes around them, every sample-rate
    code and the rates around the explicit forms' limits, every bit depth, and frame numbers across the UTF-8 lengths
    inside one launch.  -> launches (the other families' cases get theirs from groups())."""
    rng = np.random.default_rng(0x199)
    out = []
    count = max(len(I_BLOCK_SIZES), len(I_RATES), len(I_NUMBERS))
    for i in range(count):
        n = I_BLOCK_SIZES[i % len(I_BLOCK_SIZES)]
        rate = I_RATES[i % len(I_RATES)]
        bps = I_DEPTHS[i % len(I_DEPTHS)]
        first, step, frames = I_NUMBERS[i % len(I_NUMBERS)]
        stereo = i % 2 == 0
        channels = 2 if stereo else (1, 3)[i // 2 % 2]
        probe = PackCase("probe", "I", np.zeros((channels, n), np.int64), bps, [dict(kind="constant")] * channels,
                         stereo=stereo)
        if lds_bytes(probe) > LDS_LIMIT:
            bps = 8                                # a block this long fits the LDS image at fewer bits only
        cases = []
        for f in range(frames):
            assignment = (i + f) % 4 if stereo and n > 1 else 0   # (one sample: a 9-bit side role breaks the bit bound)
            lo = -(1 << (bps - 1))
            v = [int(rng.integers(lo // 2, -lo // 2)) for _ in range(channels)]
            if f == 0:
                v[0] = lo                                    # the lowest value of the width
            x = np.repeat(np.array(v, np.int64)[:, None], n, axis=1)
            cases.append(PackCase("I %d n=%d rate=%d bps=%d #%d" % (i, n, rate, bps, first + f * step), "I", x, bps,
                                  [dict(kind="constant")] * channels, assignment, stereo))
        out.append(Launch("I %d" % i, stereo, channels, n, bps, rate, first, step, cases))
    return out


FAMILIES = collections.OrderedDict([("A", family_a), ("B", family_b), ("C", family_c), ("D", family_d), ("E", family_e),
                                    ("F", family_f), ("G", family_g), ("H", family_h)])


@functools.lru_cache(None)
def groups():
    """The launches: families A..H grouped by (entry point, channels, n, bps) at 44100 Hz with frame numbers from 0,
    then family I's launches."""
    by = collections.OrderedDict()
    for make in FAMILIES.values():
        for c in make():
            by.setdefault((c.stereo, c.channels, c.n, c.bps), []).append(c)
    out = [Launch("%s %dch n=%d %d bit" % ("stereo" if k[0] else "channels", k[1], k[2], k[3]), k[0], k[1], k[2], k[3],
                  44100, 0, 1, cases) for k, cases in by.items()]
    return out + family_i()


N_GROUPS = 49   # len(groups()), stated so that the GPU file can be collected without building a case


def all_cases():
    return [c for g in groups() for c in g.cases]


@functools.lru_cache(None)
def launch_expected(index):
    """The expected frames of launch `index`, in order."""
    g = groups()[index]
    return [expected(c, g.first + f * g.step, g.rate) for f, c in enumerate(g.cases)]


def launch_inputs(g):
    """-> (samples int32 [F, channels, n], records, residual int32 [F, channels, n])."""
    x = np.stack([samples(c) for c in g.cases])
    rec = np.stack([record(c) for c in g.cases])
    res = np.stack([residual_rows(c) for c in g.cases])
    return x, rec, res


def body_of(frame_bytes):
    """A frame without its header and CRC-16."""
    return frame_bytes[dc.header_bytes(frame_bytes):-2]

