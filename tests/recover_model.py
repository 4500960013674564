"""What flacenc_hip_recover_streams must give for one stream, from pieces none of which is code under test: the host
build of the decoder core (flacenc_rs_amd/decode_cpu.py) says which byte positions hold a verified frame and what each
decodes to, tests/pcm_pack_model.py packs, and rules 2 to 9 of the call's contract (include/flacenc_hip.h) are the plain
loops below."""
import functools

import numpy as np

import pcm_pack_model
from flacenc_rs_amd import _capi, decode_cpu


@functools.lru_cache(None)
def decoder():
    return decode_cpu.DecoderCpu(decode_cpu.build())


class Frame:
    def __init__(self, pos, length, block, number, variable, rows):
        self.pos, self.len, self.block, self.number, self.variable, self.rows = pos, length, block, number, variable, rows

    @property
    def end(self):
        return self.pos + self.len


def verified(data, channels, bps):
    """Rule 1: every verified candidate of the span `data`, in ascending position.  (Kept per span: batches repeat their
    streams, and the corpus tests walk the chains the expectations were made from.)"""
    return list(_verified(np.ascontiguousarray(data, np.uint8).tobytes(), channels, bps))


@functools.lru_cache(None)
def _verified(raw, channels, bps):
    data = np.frombuffer(raw, np.uint8)
    dec = decoder()
    out = []
    sync = np.flatnonzero((data[:-1] == 0xFF) & ((data[1:] & 0xFE) == 0xF8)) if len(data) > 1 else []
    for p in sync:
        p = int(p)
        off, ln, _ = dec.index_frames(data[p:], channels, bps, 1)
        if len(off) == 0:
            continue
        n = int(ln[0])
        for bound in (4096, 65536):
            rows, bs, num, st = dec.decode_frames(data[p:p + n], [0], [n], channels, bps, bound)
            if st[0] == 0:
                break
        assert st[0] == 0, (p, st)
        out.append(Frame(p, n, int(bs[0]), int(num[0]), int(data[p + 1]) & 1, rows[0][:, :int(bs[0])].copy()))
    return out


def chain(cands):
    """Rule 2: the resynchronising chain over the verified candidates."""
    out, at = [], 0
    for c in cands:
        if c.pos >= at:
            out.append(c)
            at = c.end
    return out


def expected(data, channels, bps, mbs, width, capacity, origin=0):
    """-> (the L * W bytes the slot's front must hold, totals [8], gaps [(first_sample, n_samples)])."""
    n_bytes = len(data)
    if n_bytes == 0:
        return np.zeros(0, np.uint8), [0] * 8, []
    frames = chain(verified(data, channels, bps))
    W = channels * width
    breaks, at, covered = 0, 0, 0
    for f in frames:
        breaks += f.pos != at
        at = f.end
        covered += f.len
    breaks += at != n_bytes
    # rules 3 and 4
    placed, top, dropped = [], origin, 0
    for f in frames:
        P = f.number if f.variable else f.number * mbs
        E = P + f.block
        if f.block <= mbs and P >= origin and P >= top:
            placed.append((P, E, f))
        else:
            dropped += 1
        top = max(top, E)
    # rule 5
    written, why = [], 0
    for P, E, f in placed:
        if (E - origin) * W > capacity:
            why = _capi.DECODE_NO_ROOM
            break
        written.append((P, E, f))
    L = written[-1][1] - origin if written else 0
    slot = np.zeros(L * W, np.uint8)
    gaps, at, silence = [], origin, 0
    for P, E, f in written:
        if P > at:
            gaps.append((at - origin, P - at))
            silence += P - at
        pcm, _, _ = pcm_pack_model.pack_le_bytes(f.rows[None], [f.block], width)
        slot[(P - origin) * W:(E - origin) * W] = pcm
        at = E
    return slot, [len(written), L, silence, dropped, n_bytes - covered, breaks, why, 0], gaps


def expected_batch(batch, origins=None):
    origins = origins if origins is not None else [0] * len(batch.streams)
    return [expected(s.data, s.channels, s.bps, s.mbs, s.width, cap, int(o))
            for s, cap, o in zip(batch.streams, batch.capacities, origins)]


def gap_records(want):
    """The call's gap table for a batch's expectations: (stream, first_sample, n_samples) by stream, then position."""
    return [(i, a, n) for i, (_, _, gaps) in enumerate(want) for a, n in gaps]


def check_batch(batch, out, totals, gaps, call, want, max_gaps=None):
    """One call's output buffer, totals, gap records and call totals against the model; FILL wherever the rule says
    untouched."""
    written = []
    for i, (slot, tot, _) in enumerate(want):
        got = [int(v) for v in totals[i]]
        assert got == tot, (batch.streams[i].name, got, tot)
        assert np.array_equal(batch.slot(out, i)[:len(slot)], slot), batch.streams[i].name
        written.append(len(slot))
    assert batch.outside_slots_untouched(out, written), "bytes outside the defined prefixes were written"
    records = gap_records(want)
    keep = len(records) if max_gaps is None else min(max_gaps, len(records))
    assert [tuple(int(v) for v in g) for g in np.asarray(gaps).reshape(-1, 3)[:keep]] == records[:keep]
    assert [int(v) for v in call] == [sum(t[0] for _, t, _ in want), sum(t[1] for _, t, _ in want), len(records),
                                       sum(t[3] for _, t, _ in want)]
