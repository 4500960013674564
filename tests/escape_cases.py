"""The signals of the FLACENC_HIP_FLAG_RICE_ESCAPE tests (tests/test_rice_escape_cpu.py asserts from the model alone that
they do what they are here for; tests/test_gpu_rice_escape.py runs them on the device).  Every signal is a function of
the block size n and a seed; ESCAPING names the families in which some partition must escape."""
import numpy as np

import flac_write as fw
import util

BLOCK_SIZES = (192, 256, 1000, 4095, 4096, 4608, 16384)
ESCAPING = ("ramp", "tone_then_silence", "silence_then_tone", "burst24", "fullscale24")


def _rng(n, seed):
    return np.random.default_rng(0xE5C0000 + 131 * n + seed)


def ramp(n, seed=0):
    """x[t] = 3t - 1000: the fixed predictor of order 2 leaves an all-zero residual (24-bit container)."""
    return (3 * np.arange(n, dtype=np.int64) - 1000).astype(np.int32), 24


def tone_then_silence(n, seed=0):
    """Tone + noise, digital silence from sample 2085 of 4096 on (the same share of any block; below 256 samples from
    three samples before the middle, so that the second of two partitions is silent behind the predictor's tail)."""
    x = util.sine_noise(n, 16, 97.0, 0.3, 0.01, 11 + seed).copy()
    x[(n * 2085 // 4096 if n >= 256 else n // 2 - 3):] = 0
    return x, 16


def silence_then_tone(n, seed=0):
    """Digital silence for the first 700 samples of 4096 (the same share of any block), then tone + noise."""
    x = util.sine_noise(n, 16, 61.0, 0.25, 0.02, 25 + seed).copy()
    x[:n * 700 // 4096] = 0
    return x, 16


def burst24(n, seed=0):
    """Quiet 24-bit noise with one 64-sample full-scale burst."""
    rng = _rng(n, seed)
    x = rng.integers(-40, 41, n).astype(np.int64)
    at = (n // 3) & ~63
    x[at:at + 64] = rng.integers(-(1 << 23), 1 << 23, min(64, n - at))
    return x.astype(np.int32), 24


def fullscale24(n, seed=0):
    """Full-scale 24-bit noise: Rice codes it above the container."""
    return _rng(n, seed).integers(-(1 << 23), 1 << 23, n).astype(np.int32), 24


def bench_like(n, seed=0):
    """The benchmark's material: Sine(200, 0.4) + Noise(0.4) at 16 bits -- nothing escapes."""
    return util.sine_noise(n, 16, 200.0, 0.4, 0.4, 0xF1AC + seed), 16


FAMILIES = dict(ramp=ramp, tone_then_silence=tone_then_silence, silence_then_tone=silence_then_tone, burst24=burst24,
                fullscale24=fullscale24, bench_like=bench_like)


def must_escape(name, n, order):
    """Does the family's block of n samples, coded by the fixed predictor of `order` (0..2), have an escaped partition?
    True / False where the construction says so, None where it is left to the noise."""
    one_partition = n == 4095                                     # an odd block: the finest level is the whole block
    if name == "ramp":                                            # an all-zero residual at order 2
        return True if order == 2 else None
    if name == "tone_then_silence":                               # whole partitions of zeros behind the tone
        return not one_partition
    if name == "silence_then_tone":                               # ... in front of it, where the silence holds one
        return False if one_partition else (True if n >= 1000 else None)
    if name == "burst24":                                         # the burst's partition, where it is 64 samples long
        return True if order == 2 and n in (4096, 4608, 16384) else None
    if name == "fullscale24":                                     # 24 bits raw against 24.5 of Rice code at order 0;
        return order == 0                                         # a difference signal is a bit wider and stays Rice
    return False                                                  # bench_like


def fixed_residual(x, order):
    """The fixed predictor's error signal, warm-up slots zero (int64)."""
    return fw.residuals(np.asarray(x, np.int64), fw.FIXED_COEFS[order], 0, order)


def stereo_frames(n, frames=4):
    """[frames, 2, n] int32 at 16 bits: one frame per 16-bit family, left and right a little apart (a side role stays
    small), the silences in the same places in both."""
    out = []
    for f in range(frames):
        fam = (tone_then_silence, silence_then_tone, bench_like)[f % 3]
        l, _ = fam(n, f)
        r, _ = fam(n, f + 100)
        out.append(np.stack([l, (l.astype(np.int64) // 2 + r // 2).astype(np.int32)]))
    return np.stack(out).astype(np.int32)
