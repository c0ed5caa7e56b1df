"""The captures of the synchroniser's tests, shared by tests/test_sync_cpu.py (which checks on the oracle's chains and the
float64 model that every one of them is found, with every integer decision far from going the other way) and
tests/test_sync_gpu.py (which asserts equal integers on the device)."""
import functools

import numpy as np

from tests import demod_cases as DC
from tests.sync_model import geometry

MAX_SHIFT = 31
NTAPS = 45
CFG2, CFG3 = 0, DC.GAIN | DC.FIR

# name -> (mode, stages, oracle keywords, start, cfo in carrier spacings, phase, noise_db or None, seed, s16)
# Every case met the conditions of tests/test_sync_cpu.py with the seed and offset it was first written with: none was changed.
CASES = {
    "m1_cfg2": (1, CFG2, {}, 1234, 3.37, 0.7, 20.0, 11, False),
    "m2_cfg2": (2, CFG2, {}, 1234, -7.31, -2.1, 20.0, 12, False),
    "m3_cfg2": (3, CFG2, {}, 333, 12.2, 1.3, 20.0, 13, False),
    "m4_cfg2": (4, CFG2, {}, 1234, -0.25, 3.0, 20.0, 14, False),
    "m1_cfg3": (1, CFG3, dict(gain_mode=2, normalise=DC.NORMALISE), 70001, -20.4, 0.4, None, 15, False),
    "m1_cfg3_tii": (1, CFG3, dict(gain_mode=2, normalise=DC.NORMALISE, tii=DC.TII), 70001, -20.4, 0.4, None, 16, False),
    "m2_clean": (2, CFG2, {}, 0, 0.0, 0.0, None, 17, False),
    "m1_s16": (1, CFG3, dict(gain_mode=2, normalise=1.0), 1234, 3.37, 0.7, 20.0, 18, True),
}
CFG3_CASES = ("m1_cfg3", "m1_cfg3_tii", "m1_s16")


def case_bits(mode, n_frames=2):
    """The coded bits of the case's chain: n_frames + 1 frames (the last one only lends its ends to the capture)."""
    import oracle as O
    return DC.case_bits(mode, n_frames + 1, O.tf_input_bytes(mode))


def capture_of(y, mode, start, cfo, phase, noise_db, seed, n_frames=2, s16=False, tail=None):
    """y: (n_frames + 1, tf) chain output.  -> the capture: the last `start` samples of the extra frame, n_frames frames, and
    a tail from the head of the extra frame (at least 2 B + N samples, and what the shortest capture the library takes needs);
    times exp(j (2 pi cfo i / N + phase)), plus complex Gaussian noise noise_db below the data symbols; complex64, or int16
    pairs through the oracle's FormatConverter."""
    g = geometry(mode)
    N, B, null, tf = g["N"], g["B"], g["null"], g["tf"]
    y = np.asarray(y).reshape(n_frames + 1, tf).astype(np.complex128)
    if tail is None:
        tail = max(2 * B + N, null - start)
    x = np.concatenate([y[n_frames][tf - start:], y[:n_frames].reshape(-1), y[n_frames][:tail]])
    i = np.arange(x.size, dtype=np.float64)
    x = x * np.exp(1j * (2.0 * np.pi * cfo * i / N + phase))
    if noise_db is not None:
        rs = np.random.RandomState(seed)
        p = float(np.mean(np.abs(y[:n_frames, null:]) ** 2))
        sigma = np.sqrt(p / 10.0 ** (noise_db / 10.0) / 2.0)
        x = x + sigma * (rs.randn(x.size) + 1j * rs.randn(x.size))
    x = x.astype(np.complex64)
    if s16:
        import oracle as O
        q, _ = O.format_convert(x, "s16")
        return np.asarray(q, np.int16)
    return x


def capture(mode, stages, start, cfo, phase, noise_db, seed, n_frames=2, s16=False, tail=None, **kw):
    """The oracle's chain on case_bits(mode, n_frames), as a capture (capture_of)."""
    import oracle as O
    y = O.Chain(mode=mode, stages=stages, **kw).process(case_bits(mode, n_frames))
    return capture_of(y, mode, start, cfo, phase, noise_db, seed, n_frames, s16, tail)


@functools.lru_cache(maxsize=None)
def named(name, tail=None):
    """-> (capture, mode, bits of the frames inside it, true start, cfo).  Computed once per process; do not write to it."""
    mode, stages, kw, start, cfo, phase, noise_db, seed, s16 = CASES[name]
    x = capture(mode, stages, start, cfo, phase, noise_db, seed, 2, s16, tail, **kw)
    x.setflags(write=False)
    return x, mode, case_bits(mode, 2)[:2], start, cfo


def n_samples(x):
    return x.size // 2 if x.dtype == np.int16 else x.size
