"""tests/pack_cases.py proves its claims without a GPU, before a record reaches a packer: every expected frame (written
by tests/flac_write.py) parses back to the case's samples with tests/flac_parse.py and through the host build of the
project's decoder; the oracle's restatement of Frame::write, fed the record and the residual rows the packer will get,
writes the same bytes (two writers that share no code); the records' bit counts are the oracle's; every case lies in
the packer's domain; and the case list reaches every residual path and every listed edge by name."""
import shutil

import numpy as np
import pytest

import decode_cases as dc
import flac_parse
import flac_write as fw
import pack_cases as pc
from flacenc_rs_amd import _capi, decode_cpu
from oracle import oracle as orc

GROUPS = range(pc.N_GROUPS)


def test_the_stated_group_count_is_the_corpus():
    assert len(pc.groups()) == pc.N_GROUPS
    names = [c.name for c in pc.all_cases()]
    assert len(set(names)) == len(names)


def test_vectorised_residuals_equal_the_plain_loop():
    """flac_write.residuals against its definition in Python integers, at the extremes of its stated range (|c| < 2^15,
    |x| < 2^25, 32 terms) and on short and empty tails."""
    rng = np.random.default_rng(0x2E5)
    for n, order, shift in [(97, 32, 0), (64, 32, 15), (40, 1, 3), (33, 32, 7), (32, 32, 0), (5, 0, 0), (3, 4, 0)]:
        x = rng.integers(-(1 << 25) + 1, 1 << 25, n)
        x[::3] = (1 << 25) - 1
        coefs = [int(v) for v in rng.choice([-(1 << 15) + 1, (1 << 15) - 1], order)]
        want = np.zeros(n, np.int64)
        for t in range(order, n):
            want[t] = int(x[t]) - (sum(c * int(x[t - 1 - j]) for j, c in enumerate(coefs)) >> shift)
        assert np.array_equal(fw.residuals(x, coefs, shift, order), want), (n, order, shift)


@pytest.mark.parametrize("g", GROUPS)
def test_expected_frames_parse_back_to_the_samples(g):
    group = pc.groups()[g]
    for f, (case, data) in enumerate(zip(group.cases, pc.launch_expected(g))):
        got = flac_parse.parse_frame(data, stream_bps=group.bps, stream_rate=group.rate, wasted_ok=True)
        assert np.array_equal(got["channels"], case.x), case
        assert got["number"] == group.first + f * group.step and got["length"] == len(data), case
        assert got["block_size"] == case.n and got["bps"] == group.bps and got["sample_rate"] == group.rate, case
        assert got["channel_tag"] == case.tag and got["variable"] == 0, case
        assert got["kinds"] == [sf["kind"] for sf in case.subs], case
        assert got["orders"] == [sf["order"] for sf in case.subs], case
        assert pc.body_of(data) == pc.expected_body(case), case


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_the_projects_decoder_reads_every_expected_frame():
    """The domain's first line: the host build of flac_decode_core.h gives status 0 and the samples, the frames with an
    empty first partition included."""
    dec = decode_cpu.DecoderCpu(decode_cpu.build())
    for g, group in enumerate(pc.groups()):
        frames = pc.launch_expected(g)
        lengths = np.array([len(b) for b in frames], np.uint32)
        offsets = np.concatenate([[0], np.cumsum(lengths[:-1])]).astype(np.uint64)
        out, bs, num, st = dec.decode_frames(b"".join(frames), offsets, lengths, group.channels, group.bps, group.n,
                                             threads=4)
        assert not st.any(), [(group.cases[f].name, int(st[f])) for f in np.flatnonzero(st)]
        assert (bs == group.n).all()
        assert np.array_equal(num, group.first + np.arange(len(frames), dtype=np.uint64) * group.step)
        assert np.array_equal(out, np.stack([c.x for c in group.cases])), group.name


def _oracle_subframes(case, rec, rows):
    """orc.write_frame's description of the subframes, from the packer's own inputs."""
    out = []
    for c in range(case.channels):
        r = rec[c]
        sig, w = pc.coded_signals(case)[c]
        p = r["params"]
        out.append(dict(kind=int(r["kind"]), bps=w, samples=sig, dc_offset=int(r["dc_offset"]), order=int(p["order"]),
                        shift=int(p["shift"]), precision=int(p["precision"]), coefs=p["coefs"].copy(),
                        rice_order=int(p["rice_order"]), rice_params=p["rice_params"].copy(), residual=rows[c]))
    return out


@pytest.mark.parametrize("g", GROUPS)
def test_the_oracle_writes_the_same_bytes_from_the_records(g):
    """Frame::write as the oracle restates it, on the record and the residual rows the packer gets, against flac_write on
    the description: the same bytes (cases without wasted bits, which the oracle's writer cannot express), and the
    record's bit counts are the oracle's SubFrame::count_bits."""
    group = pc.groups()[g]
    compared = 0
    for f, (case, want) in enumerate(zip(group.cases, pc.launch_expected(g))):
        number = group.first + f * group.step
        rec, rows = pc.record(case), pc.residual_rows(case)
        hdr = orc.write_frame_header(case.n, case.tag, group.bps, group.rate, False, number)
        assert want[:len(hdr)] == hdr, case
        if any(sf["wasted"] for sf in case.subs):
            continue
        if case.stereo:
            got = orc.write_stereo_frame(rec, case.x[0], case.x[1], group.bps, group.rate, number, rows[0], rows[1])
            subs = [dict(kind=int(rec["kind"][c]), bps=pc.coded_signals(case)[c][1], samples=pc.coded_signals(case)[c][0],
                         dc_offset=int(rec["dc_offset"][c]), order=int(rec["lpc"][c]["order"]),
                         shift=int(rec["lpc"][c]["shift"]), precision=int(rec["lpc"][c]["precision"]),
                         coefs=rec["lpc"][c]["coefs"].copy(), rice_order=int(rec["lpc"][c]["rice_order"]),
                         rice_params=rec["lpc"][c]["rice_params"].copy(), residual=rows[c]) for c in range(2)]
            bits = [int(rec["bits"][role]) for role in pc.roles(case)]
            assert sorted(np.flatnonzero(rec["bits"])) == sorted(set(pc.roles(case))), case
        else:
            subs = _oracle_subframes(case, rec, rows)
            got = orc.write_frame(case.n, 0, group.bps, group.rate, number, subs)
            bits = [int(rec[c]["bits"]) for c in range(case.channels)]
        assert got == want, (case, len(got), len(want))
        for c, sf in enumerate(subs):
            assert orc.write_subframe(n=case.n, **sf)[1] == bits[c], (case, c)
        compared += 1
    assert compared or all(any(sf["wasted"] for sf in c.subs) for c in group.cases)


def test_every_case_lies_in_the_packers_domain_and_its_record_is_consistent():
    for case in pc.all_cases():
        pc.check_domain(case)
        rec, rows = pc.record(case), pc.residual_rows(case)
        assert rows.dtype == np.int32 and rows.shape == case.x.shape
        total = 0
        for c, sf in enumerate(case.subs):
            p = rec["lpc"][c] if case.stereo else rec[c]["params"]
            bits = int(rec["bits"][pc.roles(case)[c]]) if case.stereo else int(rec[c]["bits"])
            pad = int(rec["pad"][c]) if case.stereo else int(rec[c]["pad"][0])
            assert pad == sf["wasted"] and int(p["status"]) == 0, case
            assert bits == len(pc.subframe_bit_list(case, c)), case
            total += bits
            if sf["kind"] in ("fixed", "lpc"):
                assert not rows[c, :sf["order"]].any(), case
                assert int(p["subframe_bits"]) == bits - sf["wasted"], case
                assert p["rice_params"][:1 << sf["porder"]].tolist() == sf["params"], case
                assert not p["rice_params"][1 << sf["porder"]:].any(), case
                if sf["kind"] == "fixed":
                    assert p["coefs"][:4].tolist() == pc.FIXED_LPC_COEFS[sf["order"]], case
                    assert int(p["shift"]) == 0 and int(p["precision"]) == 0, case
                # Residual::count_bits from the record's own sums: header, parameters, stop bits + remainders, quotients
                pbits = 5 if sf["method"] else 4
                psize = case.n >> sf["porder"]
                coded = [psize - (sf["order"] if q == 0 else 0) for q in range(1 << sf["porder"])]
                want = 6 + pbits * len(coded) + sum(k * (1 + q) for k, q in zip(coded, sf["params"])) + \
                    int(p["sum_quotients"])
                assert int(p["code_bits"]) == want, (case, c)
            else:
                assert not rows[c].any() and not np.frombuffer(p.tobytes(), np.uint8).any(), case
        # the launch's frame is what the records' bits say
        assert 8 * len(pc.expected_body(case)) == (total + 7) // 8 * 8, case
    # and the domain check does reject what it must: the corner25 frames of decode_cases as they stand
    c25 = [c for c in dc.corner_cases() if c.name.startswith("corner25")][0]
    bits = 8 * (len(c25.data) - dc.header_bytes(c25.data) - 2)
    assert bits > 2 * (8 + c25.x.shape[1] * 24)


# ---------------------------------------------------------------- the family list is complete
PATHS = ("aligned", "runs", "walk cached", "walk uncached")

EDGES = (
    ["A slot%d porder %d" % (s, p) for s in (0, 1) for p in range(9)] +
    ["A order %d porder %d" % (o, p) for p, o in [(8, 1), (8, 15), (8, 16), (7, 17), (7, 31), (7, 32)]] +
    ["A 8192 porder %d" % p for p in (0, 1, 8)] +
    ["B 4608 porder %d" % p for p in range(6)] + ["B 1152 porder %d" % p for p in range(4)] +
    ["B 48 porder 0", "B 32 order 16", "B 16 order 15", "B 16 order 16"] +
    ["C 4608 porder %d" % p for p in (6, 7, 8)] + ["C 1000 porder %d" % p for p in range(4)] +
    ["C 100 order %d" % o for o in (1, 24, 25)] + ["C 40 order 20", "C 4095 porder 0"] +
    ["D 4097 porder 0", "D 6000 porder 4", "D 20000 porder 5", "D 32767 porder 0"] +
    ["E %d %s" % (n, o) for n in (4608, 192) for o in ("walk then runs", "runs then walk")] +
    ["E a%d %s/%s" % (a, k0, k1) for a in range(4) for k0 in pc.E_KINDS for k1 in pc.E_KINDS] +
    ["E corner25 shift %d" % s for s in range(16)] + ["E corner25 %s" % p for p in ("pos", "neg", "alt")] +
    ["F %s %s" % (e, w) for e in ("all <= 14", "rice2 by one partition", "parameter 30", "long unary", "int32 ends",
                                   "precision 1") for w in PATHS] + ["F rice2 by the last of 256"] +
    ["G %s wasted %d" % (k, w) for k in pc.E_KINDS + ("side",) for w in ((1, 8, 15) if k == "side" else (1, 8, 14))] +
    ["H %dch %d" % (c, n) for c in (1, 3, 8) for n in (4096, 576, 97)] +
    ["order == part_len %s" % w for w in ("aligned", "runs", "walk")] +
    ["order == part_len - 1 %s" % w for w in ("aligned", "runs", "walk")] + ["order == n"])


def test_every_path_and_every_listed_edge_is_reached_by_a_named_case():
    cases = pc.all_cases()
    reached = set().union(*(c.edges for c in cases))
    assert not [e for e in EDGES if e not in reached]
    # the path each family is there for, computed from n and porder as the kernel computes them
    by_family = {fam: {p for c in cases if c.family == fam for p in pc.paths(c) if p} for fam in "ABCDEFGH"}
    assert by_family["A"] == {"aligned"} and by_family["B"] == {"runs"} and by_family["D"] == {"walk uncached"}
    # (4608 samples are 18 per thread: the walk on them runs uncached, next to the cached blocks of family C)
    assert by_family["C"] == {"walk cached", "walk uncached"}
    assert by_family["F"] == set(PATHS) and by_family["E"] >= {"runs", "walk cached", "walk uncached"}
    assert pc.path(4096, 8) == "aligned" and pc.path(8192, 0) == "aligned" and pc.path(4608, 5) == "runs"
    assert pc.path(4608, 6) == "walk uncached" and pc.path(4095, 0) == "walk cached" and pc.path(4097, 0) == "walk uncached"
    assert pc.path(16, 0) == "runs" and pc.path(48, 0) == "runs" and pc.path(40, 1) == "walk cached"
    # the edges mean what they say
    for c in cases:
        for where in ("aligned", "runs", "walk"):
            for edge, gap in (("order == part_len %s" % where, 0), ("order == part_len - 1 %s" % where, 1)):
                if edge in c.edges:   # an empty first partition carries parameter 5: dropped or misplaced, it shows
                    assert any(p and p.startswith(where) and sf["order"] == (c.n >> sf["porder"]) - gap and
                               (gap or sf["params"][0] == 5) for sf, p in zip(c.subs, pc.paths(c))), (c, edge)
    assert any(c.n == 4096 and sf["porder"] == 8 and sf["order"] == 16 for c in cases for sf in c.subs)
    # frames whose two subframes take different paths, in both orders
    mixed = {tuple(pc.paths(c)) for c in cases if c.stereo and None not in pc.paths(c)}
    assert ("walk uncached", "runs") in mixed and ("runs", "walk uncached") in mixed
    assert ("walk cached", "runs") in mixed and ("runs", "walk cached") in mixed
    # parameters
    subs = [(c, sf) for c in cases for sf in c.subs if sf["kind"] in ("fixed", "lpc")]
    assert any(sf["method"] == 0 and max(sf["params"]) == 14 for _, sf in subs)
    assert any(sf["params"][-1] == 15 and max(sf["params"][:-1]) <= 14 and len(sf["params"]) == 256 for _, sf in subs)
    assert any(sf["params"][0] == 15 and max(sf["params"][1:]) <= 14 for _, sf in subs)
    assert any(30 in sf["params"] for _, sf in subs) and any(sf.get("precision") == 1 for _, sf in subs)
    for where in PATHS:
        ends = [c for c in cases if "F int32 ends %s" % where in c.edges]
        rows = pc.residual_rows(ends[0])
        assert rows.max() == 2 ** 31 - 1 and rows.min() == -2 ** 31 and pc.paths(ends[0])[0] == where
        unary = [c for c in cases if "F long unary %s" % where in c.edges][0]
        sf = unary.subs[1]
        lo = 2 * (unary.n >> sf["porder"])
        assert sf["params"][2] == 0 and np.abs(unary.x[1, lo:lo + 16]).max() >= 300 and pc.paths(unary)[1] == where
    # the corner25 construction: a 25-bit side role, order 32, precision 15, every shift, the three sign patterns
    corner = [c for c in cases if c.name.startswith("E corner25")]
    assert sorted(sf["shift"] for c in corner for sf in c.subs[:1]) == list(range(16))
    for c in corner:
        side = c.x[0] - c.x[1]
        assert c.assignment == 1 and side.max() == 2 ** 24 - 1 and side.min() == -2 ** 24 + 1
        assert all(sf["order"] == 32 and sf["precision"] == 15 for sf in c.subs)
    # wasted bits k = 1, 8, w - 2 beside each kind, the side role at w = bps + 1
    for kind in pc.E_KINDS:
        ks = {sf["wasted"] for c in cases if c.family == "G" and c.assignment == 0 for sf in c.subs
              if sf["kind"] == kind}
        assert ks >= {1, 8, 14}, kind
    assert {c.subs[1]["wasted"] for c in cases if c.family == "G" and c.assignment == 1} == {1, 8, 15}
    # family H: 1, 3 and 8 channels through the channel records
    assert {(c.channels, c.n) for c in cases if not c.stereo and c.family == "H"} == \
        {(ch, n) for ch in (1, 3, 8) for n in (4096, 576, 97)}


def test_the_header_sweep_holds_every_listed_value():
    launches = pc.family_i()
    assert {g.n for g in launches} == set(pc.I_BLOCK_SIZES) == set(fw.BS_CODES) - {32768} | {1, 2, 255, 257, 4095, 32767}
    assert {g.rate for g in launches} == set(pc.I_RATES) >= set(flac_parse.SAMPLE_RATES.values()) | {
        255000, 256000, 65535, 65536, 655350, 655360, 1}
    assert {g.bps for g in launches} >= {8, 12, 16, 20, 24, 14}
    assert {pc.rate_header(g.rate)["sr_code"] for g in launches} == set(range(15))
    numbers = [[g.first + f * g.step for f in range(len(g.cases))] for g in launches]
    for b in (128, 2048, 65536, 1 << 21, 1 << 26):
        assert any(seq[:3] == [b - 1, b, b + 1] for seq in numbers), b           # across the boundary, one by one
        assert any(len(seq) == 2 and seq[0] < b <= seq[1] and seq[1] - seq[0] > 1 for seq in numbers), b   # by a step
    assert any(seq[-1] == 2 ** 31 - 1 for seq in numbers)
    assert {g.stereo for g in launches} == {True, False}
    assert all(sf["kind"] == "constant" for g in launches for c in g.cases for sf in c.subs)
    assert _capi.FRAME_RESULT_DTYPE.itemsize == 752 and _capi.CHANNEL_RESULT_DTYPE.itemsize == 368
