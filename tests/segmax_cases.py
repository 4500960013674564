"""The inputs of the segmented max-scan on its own (flacenc_hip_debug_segmax_scan; tests/test_gpu_segmax_scan.py) and
its reference: a plain loop over segments, np.maximum.accumulate on uint64 per segment.  The sizes lie around the scan's
seams: 256 elements per workgroup of the reduce and apply kernels, 1024 aggregates per round of the one-workgroup carry
kernel, so that its second round starts at element 1024 * 256 = 262 144.  No GPU is needed to build any of it:
tests/test_recover_long_cpu.py shows on the reference that these cases tell a carry lost at 262 144 from a kept one."""
import numpy as np

WG = 256
ROUND = 1024 * WG
SIZES = (1, 255, 256, 257, ROUND - 1, ROUND, ROUND + 1, 2 * ROUND + 300)
TOP = (1 << 64) - 1


def reference(values, heads):
    """out[m] = the unsigned maximum of values from the head of m's segment up to m."""
    values = np.asarray(values, np.uint64)
    out = np.empty_like(values)
    starts = np.flatnonzero(heads)
    assert len(values) == 0 or (len(starts) and starts[0] == 0)
    for a, b in zip(starts, list(starts[1:]) + [len(values)]):
        out[a:b] = np.maximum.accumulate(values[a:b])
    return out


def descending(n):
    """n strictly descending values from 2^64 - 1 down through 2^63: an element never exceeds one in front of it, so
    every output is its segment's first value -- and a signed comparison orders the two halves the wrong way round."""
    step = TOP // (n + 1)
    return np.uint64(TOP) - np.arange(n, dtype=np.uint64) * np.uint64(step)


def random64(rng, n):
    return rng.integers(0, 1 << 64, n, dtype=np.uint64)


def heads_at(n, positions):
    h = np.zeros(n, np.uint8)
    h[[p for p in positions if 0 <= p < n]] = 1
    if n:
        h[0] = 1   # the contract: element 0 is a head
    return h


def sparse_heads(rng, n):
    h = (rng.integers(0, 3000, n) == 0).astype(np.uint8)
    if n:
        h[0] = 1
    return h


def one_segment(n, rng):
    """Element 0 is the maximum; the others are random below 2^63."""
    v = random64(rng, n) >> np.uint64(1)
    v[0] = TOP - 5
    return v, heads_at(n, [0])


# name -> (the smallest n that reaches the pattern, (n, rng) -> (values, heads))
PATTERNS = {
    "one segment, element 0 its maximum": (1, one_segment),
    "heads at 256k": (1, lambda n, rng: (random64(rng, n), heads_at(n, range(0, n, WG)))),
    "heads at 256k - 1": (WG, lambda n, rng: (random64(rng, n), heads_at(n, range(WG - 1, n, WG)))),
    "heads at 256k + 1": (2, lambda n, rng: (random64(rng, n), heads_at(n, range(1, n, WG)))),
    "heads at 256k - 1, descending": (WG, lambda n, rng: (descending(n), heads_at(n, range(WG - 1, n, WG)))),
    "heads at 256k + 1, descending": (2, lambda n, rng: (descending(n), heads_at(n, range(1, n, WG)))),
    "a head at 262143": (ROUND, lambda n, rng: (descending(n), heads_at(n, [ROUND - 1]))),
    "a head at 262144": (ROUND + 1, lambda n, rng: (descending(n), heads_at(n, [ROUND]))),
    "a head at 262145": (ROUND + 2, lambda n, rng: (descending(n), heads_at(n, [ROUND + 1]))),
    "sparse heads, descending": (2, lambda n, rng: (descending(n), sparse_heads(rng, n))),
    "sparse heads, 64 random bits": (1, lambda n, rng: (random64(rng, n), sparse_heads(rng, n))),
}


def case(pattern, n):
    """-> (values uint64 [n], heads uint8 [n])."""
    least, make = PATTERNS[pattern]
    assert n >= least
    return make(n, np.random.default_rng([n, sorted(PATTERNS).index(pattern)]))


def all_cases():
    """(pattern, n) for every size of SIZES that reaches the pattern."""
    return [(p, n) for p, (least, _) in PATTERNS.items() for n in SIZES if n >= least]
