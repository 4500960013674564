"""CPU: FLACENC_HIP_FLAG_RICE_ESCAPE's definition as tests/escape_model.py states it.

  * with escapes disabled the model is the reference's search: orc_find_partitioned_rice_parameter's order, parameters
    and code_bits, and the oracle's Residual::count_bits, on every signal of tests/escape_cases.py;
  * on seeded random rows a flagged record is never longer than the unflagged one, identical to it when nothing escapes,
    and tests/flac_parse.py reads the model's bytes back to the residual;
  * flacenc_rs_amd/csrc/rice_escape_core.h, compiled for the host from its own text, equals the model on random and
    constructed partitions (cnt = 0, widths 0 / 1 / 31 / 32, the tie E == R), once optimised and once as a stand-alone
    program under AddressSanitizer + UBSan;
  * the corpus has teeth: every escaping family escapes somewhere at every block size, the silence-then-signal case
    changes rice_order, and the benchmark's material at fixed orders 1 and 2 escapes nowhere."""
import os
import subprocess

import numpy as np
import pytest

import escape_cases as ec
import escape_model as em
import flac_parse
from oracle import oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU_SIZES = (192, 256, 1000, 4095, 4096, 4608)


def corpus():
    """(name, residual row, warm-up length) over the families, the block sizes and two fixed orders."""
    for name, fam in ec.FAMILIES.items():
        for n in CPU_SIZES:
            x, _ = fam(n)
            for order in (1, 2):
                yield "%s/%d/fixed%d" % (name, n, order), ec.fixed_residual(x, order), order


def random_rows():
    rng = np.random.default_rng(0xE5CA9E)
    for i in range(40):
        n = int(rng.choice([64, 192, 256, 1000, 1152, 4095, 4096]))
        order = int(rng.integers(0, 33))
        scale = int(rng.choice([1, 3, 40, 3000, 1 << 20]))
        e = np.rint(rng.standard_normal(n) * scale).astype(np.int64)
        for _ in range(int(rng.integers(0, 4))):                  # silent and loud stretches
            a = int(rng.integers(0, n))
            b = min(n, a + int(rng.integers(1, n // 2 + 2)))
            e[a:b] = 0 if rng.integers(0, 2) else rng.integers(-(1 << 23), 1 << 23, b - a)
        e[:order] = 0
        yield n, order, e, int(rng.choice([14, 30, 30, 4]))


def test_without_escapes_the_model_is_the_reference_search():
    for name, e, order in corpus():
        m = em.search(e, order, 30, escape=False)
        ro, ps, code_bits, _ = orc.find_partitioned_rice_parameter(e.astype(np.int32), order, 30)
        assert (m["rice_order"], m["params"], m["code_bits"]) == (ro, [int(p) for p in ps], code_bits), name
        res = orc.encode_residual(e.astype(np.int32), order, 30)
        assert (m["sum_quotients"], m["residual_bits"]) == (res["sum_quotients"], res["count_bits"]), name
        f = em.search(e, order, 30, escape=False, finest_only=True)
        assert f["rice_order"] == orc.finest_partition_order(len(e), max(64, order)), name


def test_flagged_rows_are_never_longer_identical_without_escapes_and_decode_back():
    escaped_rows = 0
    for n, order, e, max_p in random_rows():
        plain = em.search(e, order, max_p, escape=False)
        for finest in (False, True):
            m = em.search(e, order, max_p, escape=True, finest_only=finest)
            base = em.search(e, order, max_p, escape=False, finest_only=finest)
            assert m["residual_bits"] <= base["residual_bits"] and m["code_bits"] <= base["code_bits"]
            if not m["escaped"]:
                assert m == base
            else:
                escaped_rows += 1
            raw, nbits = em.residual_bytes(e, order, m["rice_order"], m["params"])
            assert nbits == m["residual_bits"]
            r = flac_parse.Bits(raw)
            got = flac_parse._residual(r, n, order)
            assert r.pos == nbits and np.array_equal(got[order:], e[order:])
        assert plain["residual_bits"] == orc.encode_residual(e.astype(np.int32), order, max_p)["count_bits"]
    assert escaped_rows > 15


def constructed_partitions():
    """(lo, hi, cnt, rice_cost, rice_param): the edges by hand, then random ones."""
    rows = [(0, 0, 0, 4, 0),                                      # cnt = 0: width 0, E = 9 > R = 4
            (0, 0, 64, 68, 0),                                    # width 0: E = 9
            (-1, -1, 64, 4 + 64 + 64, 0),                         # e = -1 only: width 1
            (-1, 0, 100, 200, 0),
            (-(1 << 30), (1 << 30) - 1, 64, (1 << 27) - 1, 30),   # width 31
            (-(1 << 30) - 1, 0, 64, (1 << 27) - 1, 30),           # width 32: cannot be escaped
            (0, 1 << 30, 64, (1 << 27) - 1, 30),                  # width 32 from the top
            (-(1 << 31), (1 << 31) - 1, 32767, (1 << 27) - 1, 30),
            (-4, 3, 64, 9 + 64 * 3, 2),                           # the tie E == R stays Rice
            (-4, 3, 64, 9 + 64 * 3 + 1, 2),                       # one bit above the tie escapes
            (-4, 3, 64, 9 + 64 * 3 - 1, 2)]
    rng = np.random.default_rng(0xC02E)
    for _ in range(4000):
        w = int(rng.integers(0, 33))
        lim = 1 << max(w - 1, 0)
        lo, hi = sorted(int(v) for v in rng.integers(-lim, lim, 2)) if w else (0, 0)
        cnt = int(rng.integers(0, 32768))
        k = int(rng.integers(0, 31))
        base = 4 + cnt * (k + 1)
        cost = min((1 << 27) - 1, base + int(rng.integers(0, 1 << int(rng.integers(1, 26)))))
        if rng.integers(0, 4) == 0:                               # around the tie
            cost = max(base, min((1 << 27) - 1, 9 + cnt * em.raw_width(np.array([lo, hi])) + int(rng.integers(-1, 2))))
        rows.append((lo, hi, cnt, cost, k))
    return rows


def model_line(lo, hi, cnt, rice_cost, k):
    w = em.raw_width(np.array([lo, hi]))
    e = em.escape_cost(cnt, w)
    esc = e is not None and e < rice_cost
    sq = rice_cost - 4 - cnt * (k + 1)
    return (w, -1 if e is None else e, (em.MARK | w) if esc else k, e if esc else rice_cost,
            5 + cnt * w if esc else sq + cnt * (k + 1), 0 if esc else int(k > 14))


@pytest.mark.parametrize("name,flags", [("rice_escape_core_test", ["-O2"]),
                                        ("rice_escape_core_test_san", ["-O1", "-g", "-fsanitize=address,undefined",
                                                                       "-fno-sanitize-recover=undefined"])])
def test_the_shared_header_equals_the_model(tmp_path, name, flags):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-I",
                           os.path.join(ROOT, "flacenc_rs_amd", "csrc"),
                           os.path.join(ROOT, "tests", "host", "rice_escape_core_test.cpp"), "-o", exe])
    rows = constructed_partitions()
    text = "".join("%d %d %d %d %d\n" % r for r in rows)
    res = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    got = [tuple(int(v) for v in line.split()) for line in res.stdout.splitlines()]
    assert len(got) == len(rows)
    bad = [(r, g, model_line(*r)) for r, g in zip(rows, got) if g != model_line(*r)]
    assert not bad, bad[:5]
    widths = {g[0] for g in got}
    assert widths == set(range(33)) and any(g[2] & em.MARK for g in got) and any(not g[2] & em.MARK for g in got)


def test_the_corpus_has_teeth():
    seen = {name: 0 for name in ec.FAMILIES}
    for name, fam in ec.FAMILIES.items():
        for n in CPU_SIZES:
            x, _ = fam(n)
            for order in (0, 1, 2):
                want = ec.must_escape(name, n, order)
                if want is None:
                    continue
                m = em.search(ec.fixed_residual(x, order), order)
                assert (m["escaped"] > 0) == want, (name, n, order, m["escaped"])
                seen[name] += m["escaped"] > 0
    assert all(seen[name] >= 2 for name in ec.ESCAPING) and seen["bench_like"] == 0, seen
    # the ramp: 9 bits of residual code at every block size, against n - 2 + 4 without the flag
    for n in (256, 1000, 4096, 4608):
        e = ec.fixed_residual(ec.ramp(n)[0], 2)
        assert not e.any()
        assert em.search(e, 2)["code_bits"] == 9 and em.search(e, 2, escape=False)["code_bits"] == n + 2
    # silence, then signal: the chosen partition order changes
    e = ec.fixed_residual(ec.silence_then_tone(4096)[0], 1)
    assert em.search(e, 1)["rice_order"] != em.search(e, 1, escape=False)["rice_order"]
