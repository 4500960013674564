"""tests/wide_model.py, the rule of the wide encode path in exact integers: on 16- and 24-bit signals it is the oracle's
fixed_lpc under OrderSel::BitCount and its encode_subframe without the LPC candidate; every frame it writes at 25, 28 and
32 bits parses back to its input with the RFC-derived parser and decodes with the library's CPU decoder at limit 32.
The coverage of the case list is asserted by wide_cases itself.  No GPU."""
import shutil

import numpy as np
import pytest

import flac_parse
import wide_cases as wc
import wide_model as wm
from flacenc_rs_amd import decode_cpu
from oracle import oracle as orc

AMPLITUDES = (300, 20000, 3000000)
BLOCKS = (64, 192, 256, 1000, 1152, 4096, 4608)


def signals():
    """(name, int32 signal, bits): sinusoids of three amplitudes plus noise at 16 and 24 bits, every block size."""
    rng = np.random.default_rng(0xF17ED)
    out = []
    for n in BLOCKS:
        for amp in AMPLITUDES:
            for bps in (16, 24):
                if amp >= 1 << (bps - 1):
                    continue
                t = np.arange(n) + rng.uniform(0, 100)
                x = np.round(amp * np.sin(2 * np.pi * t / rng.uniform(20, 300))).astype(np.int64)
                x += rng.integers(-(amp >> 5) - 2, (amp >> 5) + 3, n)
                hi = (1 << (bps - 1)) - 1
                out.append(("n=%d amp=%d bps=%d" % (n, amp, bps), np.clip(x, -hi, hi).astype(np.int32), bps))
    return out


def test_the_rule_is_the_oracles_fixed_lpc_under_bitcount():
    fixed = orc.make_fixed_config(order_sel=orc.ORDERSEL_BITCOUNT)
    seen = 0
    for name, x, bps in signals():
        n = len(x)
        verbatim_bits = 8 + n * bps
        want = orc.fixed_lpc(x, bps, verbatim_bits, fixed, max_p=30)
        got = wm.encode_subframe(x, bps, wm.make_cfg(use_constant=False))
        assert got.get("eligible") is True, name
        # the candidate itself, whether or not it beats Verbatim
        best = None
        for o in range(5):
            porder, params, code_bits = wm.rice_search(wm.fixed_errors(x, o), o, 30)
            key = bps * o + code_bits
            if best is None or key < best[0]:
                best = (key, o, porder, params, code_bits)
        assert want["selected"] == (best[0] < verbatim_bits), name
        if want["selected"]:
            seen += 1
            assert (best[1], best[2], best[4]) == (want["order"], want["rice_order"], want["code_bits"]), name
            assert list(best[3]) == want["rice_params"].tolist(), name
            if got["kind"] == wm.FIXED:
                assert got["bits"] == want["subframe_bits"] and got["order"] == want["order"], name
    assert seen >= 30


def test_the_rule_is_the_oracles_encode_subframe_without_lpc():
    fc = orc.make_frame_config(use_lpc=False, fixed=orc.make_fixed_config(order_sel=orc.ORDERSEL_BITCOUNT))
    kinds = set()
    extra = [("constant", np.full(192, -77, np.int32), 16), ("short", np.arange(17, dtype=np.int32), 16),
             ("noise", np.random.default_rng(5).integers(-(1 << 23), 1 << 23, 192).astype(np.int32), 24)]
    for name, x, bps in signals() + extra:
        want = orc.encode_subframe(x, bps, fc)
        got = wm.encode_subframe(x, bps, wm.make_cfg())
        kind = {wm.CONSTANT: 0, wm.VERBATIM: 1, wm.FIXED: 2}[got["kind"]]
        assert (kind, got["bits"]) == (want["kind"], want["bits"]), name
        kinds.add(kind)
        if kind == 2:
            assert got["order"] == int(want["fixed"].order) and got["porder"] == int(want["fixed"].rice_order), name
            assert list(got["params"]) == want["rice_params"][: 1 << got["porder"]].tolist(), name
    assert kinds == {0, 1, 2}


@pytest.mark.parametrize("wasted", (False, True))
def test_every_frame_parses_back_to_its_input(wasted):
    for c, (data, info) in zip(wc.cases(), wc.modelled(wasted)):
        back = flac_parse.parse_frame(data, stream_bps=c["bps"], wasted_ok=True)  # asserts both CRCs
        assert back["bps"] == c["bps"] and back["length"] == len(data), c["name"]
        assert np.array_equal(back["channels"], c["x"]), c["name"]
        # Verbatim is never beaten by more than it costs: no frame exceeds its bound
        body = sum(8 + c["x"].shape[1] * width for _, width in wm.roles_of(c["x"], c["bps"])[:c["x"].shape[0]])
        assert len(data) <= 16 + (body + c["x"].shape[1] + 7) // 8 + 2, c["name"]


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
@pytest.mark.parametrize("wasted", (False, True))
def test_every_frame_decodes_with_the_cpu_decoder_at_limit_32(wasted):
    dec = decode_cpu.DecoderCpu(decode_cpu.build())
    for c, (data, _) in zip(wc.cases(), wc.modelled(wasted)):
        channels, n = c["x"].shape
        out, bs, num, st = dec.decode_frames(data, [0], [len(data)], channels, c["bps"], n, max_bits_per_sample=32)
        assert st[0] == 0 and bs[0] == n and num[0] == 0, c["name"]
        assert np.array_equal(out[0], c["x"]), c["name"]
