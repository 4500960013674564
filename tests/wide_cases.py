"""The frames of the wide encode path's tests, CPU and GPU: signals at 25, 28 and 32 bits (and 16 / 24 for the checks
against the oracle and the existing path), blocks 17, 64, 192, 1000 and 4096, 1, 2, 3 and 8 channels.  A case is
dict(name, x int64 [channels, n], bps, cfg); wide_model encodes it without and with wasted bits, and the builder asserts
that the list covers what the path can do."""
import functools
import struct

import numpy as np

import depth32_cases as d32
import wide_model as wm

HI, LO = (1 << 31) - 1, -(1 << 31)


def sinusoid(rng, n, bps, scale=1.0, noise_bits=3):
    return d32.sinusoid(rng, n, scale=scale, noise_bits=noise_bits, bps=bps)


@functools.lru_cache(maxsize=None)
def cases():
    rng = np.random.default_rng(0x3217)
    out = []

    def add(name, x, bps, **cfg):
        x = np.asarray(x, np.int64)
        assert x.ndim == 2 and int(x.min()) >= -(1 << (bps - 1)) and int(x.max()) < (1 << (bps - 1)), name
        out.append(dict(name=name, x=x, bps=bps, cfg=wm.make_cfg(**cfg)))

    # ---- 32 bits, two channels: the 33-bit side ----
    add("opposed pair n=192", d32.opposed_pair(rng, 192), 32)
    add("opposed pair n=4096", d32.opposed_pair(rng, 4096), 32)
    add("skewed pair n=1000", d32.skewed_pair(rng, 1000), 32)
    add("skewed pair n=64", d32.skewed_pair(rng, 64), 32)
    add("quiet pair n=192", np.stack([sinusoid(rng, 192, 32, 1e-6), sinusoid(rng, 192, 32, 2e-6)]), 32)
    add("white noise pair n=192", rng.integers(LO, HI + 1, (2, 192)), 32)
    add("white noise mono n=64", rng.integers(LO, HI + 1, (1, 64)), 32)
    alt = np.where(np.arange(64) % 2 == 0, HI, LO)
    add("alternating extremes n=64", np.stack([alt, -alt - 1]), 32)  # the side has no eligible order
    # a constant side of 33 bits next to channels that are not constant
    low = LO + rng.integers(0, 1000, 192)
    add("constant side 2^31 + 5", np.stack([low + (1 << 31) + 5, low]), 32)
    add("constant side, n=17", np.stack([low[:17] + (1 << 31) + 5, low[:17]]), 32)
    # right + small side: the left channel is the noisier one
    right = sinusoid(rng, 192, 32, 0.5)
    add("right/side n=192", np.stack([right + rng.integers(-300, 301, 192), right]), 32)
    left = sinusoid(rng, 1000, 32, 0.5)
    add("left/side n=1000", np.stack([left, left + rng.integers(-300, 301, 1000)]), 32)
    add("both constant, extremes n=64", np.stack([np.full(64, HI), np.full(64, LO)]), 32)
    add("both constant, use_constant off", np.stack([np.full(64, HI), np.full(64, LO)]), 32, use_constant=False)
    add("silence n=192", np.zeros((2, 192), np.int64), 32, use_constant=False)
    # ---- 24-bit content in 32 bits: k = 8 ----
    add("24 in 32 pair n=192", np.stack([sinusoid(rng, 192, 24), sinusoid(rng, 192, 24, 0.3)]) << 8, 32)
    add("24 in 32 mono n=4096", sinusoid(rng, 4096, 24)[None] << 8, 32)
    add("16 in 25, 3 ch n=64", np.stack([sinusoid(rng, 64, 16, s) for s in (1.0, 0.1, 0.01)]) << 9, 25)
    # ---- other counts, depths and blocks ----
    add("3 ch 25 bits n=17", np.stack([sinusoid(rng, 17, 25) for _ in range(3)]), 25)
    add("mono 28 bits n=1000", sinusoid(rng, 1000, 28)[None], 28)
    add("pair 28 bits n=4096", np.stack([sinusoid(rng, 4096, 28), sinusoid(rng, 4096, 28, 0.7)]), 28)
    add("pair 25 bits n=1000", np.stack([sinusoid(rng, 1000, 25, 0.5), sinusoid(rng, 1000, 25, 0.5)]), 25)
    add("8 ch 32 bits n=64", np.stack([sinusoid(rng, 64, 32, 2.0 ** -c) for c in range(8)]), 32)
    add("8 ch 28 bits n=192", np.stack([sinusoid(rng, 192, 28, 2.0 ** -(2 * c)) for c in range(8)]), 28)
    add("3 ch 32 bits n=4096", np.stack([sinusoid(rng, 4096, 32, s) for s in (1.0, 1e-3, 1e-7)]), 32)
    # ---- the config is read ----
    pair = d32.skewed_pair(rng, 192)
    add("fixed_max_order 1", pair, 32, fixed_max_order=1)
    add("max_rice_parameter 14", pair, 32, max_rice_parameter=14)
    add("use_fixed off", pair, 32, use_fixed=False)
    add("no side codes", d32.opposed_pair(rng, 192), 32, use_leftside=False, use_rightside=False, use_midside=False)
    add("mid/side off", d32.opposed_pair(rng, 192), 32, use_midside=False)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def _modelled_both():
    both = {w: tuple(wm.encode_frame(c["x"], c["bps"], dict(c["cfg"], wasted_bits=w)) for c in cases())
            for w in (False, True)}
    _assert_coverage(cases(), both)
    return both


def modelled(wasted):
    """Per case (frame bytes, info) of the model, without or with wasted bits; the list's coverage is asserted."""
    return _modelled_both()[bool(wasted)]


def _assert_coverage(out, both):
    tags, chosen = set(), []
    for i, c in enumerate(out):
        for wasted in (False, True):
            info = both[wasted][i][1]
            tags.add(info["tag"])
            chosen += [(c, wasted, r, info["subframes"][r]) for r in info["roles"]]
    assert {1, 8, 9, 10} <= tags, tags  # all four channel assignments of two channels
    side = [(c, sf) for c, _, r, sf in chosen if c["x"].shape[0] == 2 and r == 3]
    assert any(sf["kind"] == wm.CONSTANT and abs(int(c["x"][0, 0] - c["x"][1, 0])) >= 1 << 31 for c, sf in side)

    def order0_fits(c, r, sf):
        sig, _ = wm.roles_of(c["x"], c["bps"])[r]
        return max(abs(v >> sf["k"]) for v in sig) < 1 << 31

    assert any(sf["kind"] == wm.FIXED and sf["order"] > 0 and not order0_fits(c, r, sf) for c, _, r, sf in chosen)
    assert any(sf.get("eligible") is False for _, info in both[False] for sf in info["subframes"])
    assert any(sf["kind"] == wm.FIXED and max(sf["params"]) > 14 for _, _, _, sf in chosen)
    assert any(sf["kind"] == wm.FIXED and max(sf["params"]) <= 14 for _, _, _, sf in chosen)
    assert any(sf["k"] == 8 and c["bps"] == 32 for c, _, _, sf in chosen)
    assert any(c["x"].shape[1] == 17 for c in out)
    assert {c["x"].shape[1] for c in out} == {17, 64, 192, 1000, 4096}
    assert {c["x"].shape[0] for c in out} == {1, 2, 3, 8} and {c["bps"] for c in out} == {25, 28, 32}
    assert {sf["kind"] for _, _, _, sf in chosen} == {wm.CONSTANT, wm.VERBATIM, wm.FIXED}


def case_file(case_list, wasted, rate=44100, number=0):
    """The input of tests/host/wide_encode_core_test.cpp."""
    blob = [struct.pack("<I", len(case_list))]
    for c in case_list:
        cfg = c["cfg"]
        blob.append(struct.pack("<13I", c["x"].shape[0], c["x"].shape[1], c["bps"], rate, number, cfg["use_constant"],
                                cfg["use_fixed"], cfg["fixed_max_order"], cfg["max_rice_parameter"], cfg["use_leftside"],
                                cfg["use_rightside"], cfg["use_midside"], int(wasted)))
        blob.append(np.ascontiguousarray(c["x"], "<i4").tobytes())
    return b"".join(blob)


def read_frames(blob, count):
    """-> [(frame bytes, bytes bound)] of the program's output."""
    out, at = [], 0
    for _ in range(count):
        length, bound = struct.unpack_from("<II", blob, at)
        out.append((blob[at + 8:at + 8 + length], bound))
        at += 8 + length
    assert at == len(blob)
    return out
