"""The rule of the wide encode path (flacenc_hip_encode_pack_frames_wide) in exact
integers, producing frames through flac_write.frame.  It is the statement the host core (wide_encode_core.h) and the
kernels (wide_encode.cpp) are held to, byte for byte.

Arithmetic: samples are at most 33 bits wide, a fixed predictor's coefficients sum to at most 16 in magnitude, so every
difference is below 2^37 and numpy's int64 is exact; a zigzagged residual is below 2^32 and a block has fewer than 2^15
samples, so every sum of u >> p is below 2^47.  The decisions themselves (keys, bit counts) are Python integers."""
import numpy as np

import flac_write as fw

CONSTANT, VERBATIM, FIXED = "constant", "verbatim", "fixed"
KNOWN_RATES = {88200: 1, 176400: 2, 192000: 3, 8000: 4, 16000: 5, 22050: 6, 24000: 7, 32000: 8, 44100: 9, 48000: 10,
               96000: 11}
SS_CODES = dict(fw.SS_CODES)
SS_CODES[32] = 7


def make_cfg(use_constant=True, use_fixed=True, fixed_max_order=4, max_rice_parameter=30, use_leftside=True,
             use_rightside=True, use_midside=True, wasted_bits=False):
    return dict(use_constant=use_constant, use_fixed=use_fixed, fixed_max_order=fixed_max_order,
                max_rice_parameter=max_rice_parameter, use_leftside=use_leftside, use_rightside=use_rightside,
                use_midside=use_midside, wasted_bits=wasted_bits)


def finest_order(n, o):
    splits = n // max(64, o)
    if splits == 0:
        return 0
    tz = (n & -n).bit_length() - 1
    return min(15, splits.bit_length() - 1, tz)


def rice_search(e, o, max_p):
    """rice.rs:246-298 on exact sums.  e: the error signal of the whole block (its first o entries are not coded).
    -> (partition order, parameters, code_bits)."""
    e = np.asarray(e, np.int64)
    n = len(e)
    u = np.where(e < 0, -2 * e - 1, 2 * e)
    order = finest_order(n, o)
    u[:o] = 0  # the warm-up adds nothing to a sum; the counts below leave it out
    # sums[j][p] = sum of u >> p over finest partition j; a coarser level's sums are sums of these (exact integers)
    sums = np.stack([(u >> p).reshape(1 << order, -1).sum(axis=1) for p in range(max_p + 1)], axis=1)
    best = None
    for level in range(order, -1, -1):
        size = n >> level
        params, total = [], 0
        for j in range(1 << level):
            count = size - (o if j == 0 else 0)
            cand = [(4 + count * (p + 1) + int(sums[j][p]), p) for p in range(max_p + 1)]
            bits, p = min(cand)  # the smallest, ties to the lowest p
            params.append(p)
            total += bits
        if best is None or total < best[2]:
            best = (level, params, total)
        if level:
            sums = sums.reshape(-1, 2, max_p + 1).sum(axis=1)
    return best


def fixed_errors(x, o):
    """The o-th difference of x (int64, exact, see the module's note); entries below o are zero."""
    d = np.asarray(x, np.int64).copy()
    for _ in range(o):
        d[1:] = d[1:] - d[:-1]
    d[:o] = 0
    return d


def wasted_bits(x, cfg):
    """k of a role as the 24-bit path counts it (wasted_bits.cpp): 0 without the flag, for silence, and for a constant
    role under use_constant."""
    if not cfg["wasted_bits"]:
        return 0
    acc = 0
    for v in x:
        acc |= int(v)
    if acc == 0 or (cfg["use_constant"] and all(int(v) == int(x[0]) for v in x)):
        return 0
    return (acc & -acc).bit_length() - 1


def encode_subframe(x, width, cfg):
    """-> dict(kind, k, bits, and for FIXED order, porder, params, code_bits; bits include k)."""
    x = [int(v) for v in x]
    n = len(x)
    if cfg["use_constant"] and all(v == x[0] for v in x):
        return dict(kind=CONSTANT, k=0, bits=8 + width)
    k = wasted_bits(x, cfg)
    w = width - k
    y = np.array([v >> k for v in x], np.int64)
    verbatim_bits = 8 + n * w
    out = dict(kind=VERBATIM, k=k, bits=verbatim_bits + k)
    if n < 64 or not cfg["use_fixed"]:
        return out
    best = None
    for o in range(min(cfg["fixed_max_order"], 4) + 1):
        e = fixed_errors(y, o)
        coded = e[o:]
        if int(coded.min()) <= -(1 << 31) or int(coded.max()) >= (1 << 31):
            continue  # RFC 9639 section 9.2.7.3
        porder, params, code_bits = rice_search(e, o, cfg["max_rice_parameter"])
        key = w * o + code_bits
        if best is None or key < best[0]:
            best = (key, o, porder, params, code_bits)
    out["eligible"] = best is not None
    if best is None or best[0] >= verbatim_bits:
        return out
    key, o, porder, params, code_bits = best
    five = max(params) > 14
    count_bits = 8 + w * o + 2 + 4 + code_bits + (len(params) if five else 0)
    if count_bits >= verbatim_bits:
        return out
    return dict(kind=FIXED, k=k, bits=count_bits + k, order=o, porder=porder, params=params, code_bits=code_bits,
                eligible=True)


def roles_of(x, bps):
    """The roles of a frame [(signal, width)]: L, R, M, S for two channels, else the channels."""
    x = [[int(v) for v in row] for row in x]
    if len(x) != 2:
        return [(row, bps) for row in x]
    left, right = x
    return [(left, bps), (right, bps), ([(a + b) >> 1 for a, b in zip(left, right)], bps),
            ([a - b for a, b in zip(left, right)], bps + 1)]


def stereo_choice(bits, cfg):
    """try_stereo_coding, coding.rs:493-522 -> (channel tag, the two roles)."""
    bl, br, bm, bs = bits
    best, tag, roles = bl + br, 1, (0, 1)
    if cfg["use_leftside"] and bl + bs < best:
        best, tag, roles = bl + bs, 8, (0, 3)
    if cfg["use_rightside"] and br + bs < best:
        best, tag, roles = br + bs, 9, (3, 1)
    if cfg["use_midside"] and bm + bs < best:
        best, tag, roles = bm + bs, 10, (2, 3)
    return tag, roles


def _keywords(sf):
    if sf["kind"] != FIXED:
        return dict(kind=sf["kind"], wasted=sf["k"])
    return dict(kind=FIXED, order=sf["order"], wasted=sf["k"], method=1 if max(sf["params"]) > 14 else 0,
                porder=sf["porder"], params=list(sf["params"]))


def rate_code(rate):
    """(sample-rate code, the value that follows the frame number) as fill_header_specs chooses them."""
    if rate in KNOWN_RATES:
        return KNOWN_RATES[rate], 0
    if rate and rate % 1000 == 0 and rate // 1000 <= 255:
        return 12, rate // 1000
    if rate and rate % 10 == 0 and rate // 10 <= 65535:
        return 14, rate // 10
    if rate and rate <= 65535:
        return 13, rate
    return 0, 0


def encode_frame(x, bps, cfg, number=0, rate=44100):
    """x: [channels, n] integers at bps bits.  -> (frame bytes, dict(tag, roles, subframes [per role]))."""
    x = np.asarray(x, np.int64)
    roles = roles_of(x, bps)
    subs = [encode_subframe(sig, width, cfg) for sig, width in roles]
    if len(roles) == 4 and x.shape[0] == 2:
        tag, chosen = stereo_choice([s["bits"] for s in subs], cfg)
    else:
        tag, chosen = x.shape[0] - 1, tuple(range(x.shape[0]))
    sr_code, sr_value = rate_code(rate)
    data = fw.frame(x, tag, bps, [_keywords(subs[r]) for r in chosen], number=number, ss_code=SS_CODES.get(bps, 0),
                    sr_code=sr_code, sr_value=sr_value)
    header = len(fw.header(x.shape[1], tag, bps, number, ss_code=SS_CODES.get(bps, 0), sr_code=sr_code, sr_value=sr_value))
    body_bits = sum(subs[r]["bits"] for r in chosen)
    assert len(data) == header + (body_bits + 7) // 8 + 2, "the counted bits are the written bits"
    return data, dict(tag=tag, roles=chosen, subframes=subs)
