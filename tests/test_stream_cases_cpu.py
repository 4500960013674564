"""The stream-contract case table (tests/stream_cases.py) covers every `*_async` export of include/flacenc_hip.h: an
async export that ships without a case fails here, on a box without a GPU."""
import stream_cases
from flacenc_rs_amd import _capi


def test_every_async_export_has_a_stream_case():
    exports = stream_cases.header_async_exports()
    assert len(exports) >= 20 and "flacenc_hip_qlpc_batch_async" in exports, exports
    covered = {c.export for c in stream_cases.all_cases()}
    assert not set(exports) - covered, "async exports without a stream case: %s" % sorted(set(exports) - covered)
    assert not covered - set(exports), "cases of exports the header does not declare: %s" % sorted(covered - set(exports))
    # the binding knows the same exports, and has a device wrapper's argtypes for each
    assert sorted(n for n in _capi.EXPORTED_SYMBOLS if n.endswith("_async")) == exports
    lib = _capi.load()
    for name in exports:
        assert getattr(lib, name).argtypes, name


def test_case_names_are_unique_and_the_flags_the_header_excludes_from_capture_are_marked():
    cases = stream_cases.all_cases()
    assert len({c.name for c in cases}) == len(cases)
    # FLACENC_HIP_FLAG_WASTED_BITS "SYNCHRONISES the stream once": the one family that is not capturable
    assert [c.name for c in cases if c.syncs] == ["WASTED_BITS"]
    assert all(not c.capturable for c in cases if c.syncs or c.comm)
    assert sum(c.capturable for c in cases) >= len(cases) - 3
