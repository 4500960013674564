"""flacenc_hip_recover_streams and flacenc_hip_decode_streams past the seams of their scans, on the GPU: every batch of
tests/recover_long_cases.py against the model of tests/recover_model.py, in host and in device memory -- chains of more
than 1024 frames, heads on the edges of the max-scan's workgroups, dropped runs across whole workgroups, more than 1024
streams, gaps of several zero-pass pieces at every residue mod 16, 3- and 8-channel decode workgroups with idle frames
--, the undamaged long batch against tests/streams_model.py and against recovery, and the plan.  What each batch is
there for is proved on the model in tests/test_recover_long_cpu.py.  Every comparison is exact."""
import numpy as np
import pytest

import recover_long_cases as lc
import recover_model as model
import streams_cases as cases
import streams_model
from test_gpu_recover_streams import GAP_FILL, RUNS, run_device, run_host

pytestmark = pytest.mark.gpu
ROUND = 1024


@pytest.mark.parametrize("memory", ["host", "device"])
@pytest.mark.parametrize("name", lc.NAMES)
def test_every_long_batch_equals_the_model(hooks_handle, name, memory):
    batch, origins = lc.all_batches()[name]
    want = lc.wanted(name)
    n_gaps = len(model.gap_records(want))
    out, totals, gaps, call = RUNS[memory](hooks_handle, batch, origins, n_gaps)
    model.check_batch(batch, out, totals, gaps, call, want)


@pytest.mark.parametrize("memory", ["host", "device"])
def test_many_streams_fill_a_short_gap_table_in_order(hooks_handle, memory):
    batch, origins = lc.all_batches()["many"]
    want = lc.wanted("many")
    total = len(model.gap_records(want))
    sizes = lc.many_max_gaps()
    assert 0 < sizes[2] < len(model.gap_records(want[:ROUND])) < total
    for max_gaps in sizes:
        out, totals, table, call = RUNS[memory](hooks_handle, batch, origins, max_gaps)
        assert call[2] == total
        model.check_batch(batch, out, totals, table[:max_gaps], call, want, max_gaps=max_gaps)
        assert (table[min(total, max_gaps):] == GAP_FILL).all()


def test_long_undamaged_streams_give_what_decode_streams_gives(hooks_handle):
    """The only place the chain from a span's first byte passes depth 64 and the scans over streams 1024 of them."""
    h = hooks_handle
    batch = lc.undamaged_batch()
    assert len(batch.streams) >= 1100
    ref = batch.fresh_out()
    ref_totals, ref_call, _ = h.decode_streams(batch.data, batch.table, batch.max_frames(), ref)
    want = streams_model.check_batch(batch, ref, ref_totals)
    assert ref_call == [sum(t[0] for _, t in want), sum(t[1] for _, t in want)] and not ref_totals[:, 3].any()
    out, totals, gaps, call = run_host(h, batch, None, 4)
    assert np.array_equal(out, ref)
    assert np.array_equal(totals[:, :2], ref_totals[:, :2]) and not totals[:, 2:].any()
    assert call == [ref_call[0], ref_call[1], 0, 0] and (gaps == GAP_FILL).all()
    out_d, totals_d, _, call_d = run_device(h, batch, [0] * len(batch.streams), 0, None)
    assert np.array_equal(out_d, ref) and np.array_equal(totals_d, totals) and call_d == call
    # decode_streams on device pointers: the same bytes and totals
    import torch
    dev = torch.device("cuda:0")
    d_in = torch.from_numpy(batch.data).to(dev)
    d_out = torch.full((batch.out_bytes,), cases.FILL, dtype=torch.uint8, device=dev)
    d_tot = torch.full((len(batch.streams), 4), -1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    call_s, _ = h.decode_streams_device(d_in.data_ptr(), len(batch.data), batch.table.copy(), batch.max_frames(),
                                        d_out.data_ptr(), d_out.numel(), d_tot.data_ptr())
    assert call_s == ref_call and np.array_equal(d_out.cpu().numpy(), ref)
    assert np.array_equal(d_tot.cpu().numpy().astype(np.uint64), ref_totals)


def test_the_plan_of_a_long_batch_is_the_plan_of_four_streams(hooks_handle):
    """Launches, synchronisations and transfers of `seams` (6000 chain frames) and of `many` (1200 streams) are those of
    four short streams of the same channel class under the same max_frames (which sizes the candidate table and with
    it the jump levels, one launch each)."""
    h = hooks_handle
    four = lc.many_streams(damaged=False)[1:5]
    small = lc.Batch(four, capacities=[4 * lc.BLOCK] * 4, spacing=2)
    for name in ("seams", "many"):
        batch, origins = lc.all_batches()[name]
        n_gaps = len(model.gap_records(lc.wanted(name)))
        for memory, transfers in (("host", 6), ("device", 3)):
            RUNS[memory](h, small, [0] * 4, 4, max_frames=batch.max_frames())
            plan4 = h.debug_last_recover_plan()
            assert plan4[3] == 1 and plan4[1] == 2 and plan4[2] <= transfers
            RUNS[memory](h, batch, origins, n_gaps)
            assert h.debug_last_recover_plan() == plan4, (name, memory)
