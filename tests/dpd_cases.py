"""The inputs of the DPD measurement's tests, shared by tests/test_dpd_cpu.py and tests/test_dpd_gpu.py: a band-limited
noise block with delayed, scaled and noisy captures of it (alignment, statistics), and the amplifier model of the closed loop.
Everything is computed once and handed out read-only."""
import numpy as np

N_SAMPLES = 43008                      # 21 x 2048
BAND_BINS = 768                        # +-768 of 2048 bins occupied
RMS = 0.25
GAIN0 = 0.8 * np.exp(0.4j)             # the capture's gain
NOISE_DB = -60.0
DELAYS = (0.0, 0.37, -300.5, 511.25, -1000.3, 1020.6)
S16_SCALE = 20000.0
PEAK = 1.0                             # the statistics' tests bin up to this amplitude (the block's largest |x| is near 0.9)
N_BINS = 64
# the statistics' cases: alignment (lag, tau) handed to the device; the capture is the block delayed by lag + tau
STATS_LAGS = (0, 7, -300, 1000)
STATS_TAUS = (0.0, 0.37)
_cache = {}


def _ro(a):
    a.setflags(write=False)
    return a


def block():
    """complex64: white noise on the bins |k| <= 768 of 2048 (in the 43 008-point transform: |k| <= 768 x 21), rms 0.25."""
    if "x" not in _cache:
        rng = np.random.default_rng(7)
        n = N_SAMPLES
        k = np.fft.fftfreq(n) * 2048.0
        X = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * (np.abs(k) <= BAND_BINS)
        x = np.fft.ifft(X)
        x *= RMS / np.sqrt(np.mean(np.abs(x) ** 2))
        _cache["x"] = _ro(x.astype(np.complex64))
    return _cache["x"]


def block_s16():
    """The block as interleaved int16 (x 20 000, rounded)."""
    if "s16" not in _cache:
        x = block().astype(np.complex128) * S16_SCALE
        p = np.empty((x.size, 2), np.float64)
        p[:, 0], p[:, 1] = x.real, x.imag
        _cache["s16"] = _ro(np.rint(p).astype(np.int16).reshape(-1))
    return _cache["s16"]


def delayed(x, d):
    """x delayed by d samples (float64, a phase ramp on the whole block's transform: circular)."""
    x = np.asarray(x, np.complex128)
    f = np.fft.fftfreq(x.size)
    return np.fft.ifft(np.fft.fft(x) * np.exp(-2j * np.pi * f * d))


def capture(d, gain=GAIN0, noise_db=NOISE_DB, seed=11):
    """complex64: the block delayed by d samples, times `gain`, plus white noise at noise_db relative to the capture."""
    key = ("rx", float(d), complex(gain), float(noise_db), seed)
    if key not in _cache:
        rng = np.random.default_rng(seed)
        y = delayed(block(), d) * gain
        sigma = np.sqrt(np.mean(np.abs(y) ** 2)) * 10.0 ** (noise_db / 20.0) / np.sqrt(2.0)
        y = y + sigma * (rng.standard_normal(y.size) + 1j * rng.standard_normal(y.size))
        _cache[key] = _ro(y.astype(np.complex64))
    return _cache[key]


# ---- the closed loop.  The amplifier: 0.9 e^{0.3j} x (1 - 0.15 a^2 + 0.02 a^4) e^{j 0.1 a^2}, a = |x|, on a signal of rms
# 0.25 whose peak is near 0.9.  The mild model on purpose: with 24 % compression at the peak a one-iteration loop blew up, by
# extrapolation beyond the measured amplitudes.  The AM/PM term stayed at 0.1 a^2: with the oracle's predistorter (the
# reference's phasor approximation) the model loop of tests/test_dpd_cpu.py goes from PA_RESIDUAL_BEFORE_DB to
# PA_RESIDUAL_AFTER_DB (filled in from that test's printout), more than the 10 dB asked for.
PA_GAIN = 0.9 * np.exp(0.3j)
PA_AM = (1.0, -0.15, 0.02)
PA_PM = 0.1


def pa(x):
    """The amplifier model in float64; returns complex128."""
    x = np.asarray(x).astype(np.complex128)
    a2 = x.real ** 2 + x.imag ** 2
    return PA_GAIN * x * (PA_AM[0] + PA_AM[1] * a2 + PA_AM[2] * a2 * a2) * np.exp(1j * PA_PM * a2)


def residual_db(y, x):
    """The residual of y against the clean x after the least-squares complex gain, in dB relative to x."""
    y, x = np.asarray(y, np.complex128), np.asarray(x, np.complex128)
    g = np.vdot(y, x) / np.vdot(y, y)
    return 10.0 * np.log10(np.sum(np.abs(g * y - x) ** 2) / np.sum(np.abs(x) ** 2))


# ---- the pair that tests/golden/make_dpd_golden.py runs through the reference's ExtractStatistic and Model_Poly
GOLDEN = {"seed": 23, "n": 20000, "rms": 0.25, "peak": float(np.float32(0.8)), "n_bins": 64, "min_count": 10, "tx_min": 0.1,
          "am3": -0.2, "pm2": 0.15}


def golden_pair(p=GOLDEN):
    """(peak is an fp32 value -- the library takes it as one -- so that both sides form the same bin edges and centres; one
    with a full mantissa, so that no power of a bin centre is an exact tie between two fp32 values.)
    (tx, rx) complex64: white noise of the given rms, and a mildly compressed, phase-rotated copy of it, scaled so that the
    medians of |tx| and |rx| agree (the reference's ExtractStatistic asserts that)."""
    rng = np.random.default_rng(p["seed"])
    x = (rng.standard_normal(p["n"]) + 1j * rng.standard_normal(p["n"])) * (p["rms"] / np.sqrt(2.0))
    tx = x.astype(np.complex64)
    t = tx.astype(np.complex128)
    a2 = np.abs(t) ** 2
    y = t * (1.0 + p["am3"] * a2) * np.exp(1j * p["pm2"] * a2)
    y *= np.median(np.abs(t)) / np.median(np.abs(y))
    return _ro(tx), _ro(y.astype(np.complex64))
