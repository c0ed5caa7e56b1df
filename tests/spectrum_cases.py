"""The synthetic signal of the spectrum monitor's tests, shared by tests/test_spectrum_cpu.py and tests/test_spectrum_gpu.py:
four tones spread over 80 dB -- one between two bins, one half-way -- on a floor of white noise at -100 dB, 40 segments long."""
import numpy as np

N_SAMPLES = 40 * 2048
TONES = [(100.0, 0.0, 0.3), (-300.37, -40.0, 1.0), (700.5, -80.0, 2.0), (-900.0, -60.0, 0.1)]     # bin, level in dB, phase
NOISE_DB = -100.0
S16_SCALE, BYTE_SCALE = 3000.0, 100.0
FORMATS = ("cf32", "s16", "u8", "s8")
WINDOWS = (0, 1, 2)
_cache = {}


def signal():
    """complex64, read-only; computed once."""
    if "cf32" not in _cache:
        rng = np.random.default_rng(1)
        n = np.arange(N_SAMPLES, dtype=np.float64)
        x = np.zeros(N_SAMPLES, np.complex128)
        for b, db, phi in TONES:
            x += 10.0 ** (db / 20.0) * np.exp(2j * np.pi * (b / 2048.0) * n + 1j * phi)
        sigma = 10.0 ** (NOISE_DB / 20.0) / np.sqrt(2.0)
        x += sigma * (rng.standard_normal(N_SAMPLES) + 1j * rng.standard_normal(N_SAMPLES))
        y = x.astype(np.complex64)
        y.setflags(write=False)
        _cache["cf32"] = y
    return _cache["cf32"]


def samples(fmt):
    """The signal in one of the four input formats: complex64, or interleaved (re, im) int16 (x 3000, rounded), uint8 / int8
    (x 100, rounded and clipped; uint8 + 128)."""
    if fmt == "cf32":
        return signal()
    if fmt not in _cache:
        x = signal().astype(np.complex128)
        pairs = np.empty((x.size, 2), np.float64)
        if fmt == "s16":
            pairs[:, 0], pairs[:, 1] = x.real * S16_SCALE, x.imag * S16_SCALE
            y = np.clip(np.rint(pairs), -32768, 32767).astype(np.int16).reshape(-1)
        elif fmt == "s8":
            pairs[:, 0], pairs[:, 1] = x.real * BYTE_SCALE, x.imag * BYTE_SCALE
            y = np.clip(np.rint(pairs), -128, 127).astype(np.int8).reshape(-1)
        elif fmt == "u8":
            pairs[:, 0], pairs[:, 1] = x.real * BYTE_SCALE, x.imag * BYTE_SCALE
            y = (np.clip(np.rint(pairs), -128, 127) + 128).astype(np.uint8).reshape(-1)
        else:
            raise ValueError(fmt)
        y.setflags(write=False)
        _cache[fmt] = y
    return _cache[fmt]


def truncated(fmt, n_samples):
    """The first n_samples samples of a format's buffer."""
    y = samples(fmt)
    return y[:n_samples] if fmt == "cf32" else y[:2 * n_samples]
