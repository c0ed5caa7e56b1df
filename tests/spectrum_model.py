"""The yardstick of the spectrum monitor: the Welch sums of include/dabgpu.h ("the spectrum monitor") and its mask rule in
float64 numpy.  Independent of the device code: the only thing taken from the library is the fp32 window table, which is the
input both sides multiply by (and which tests/test_spectrum_cpu.py holds to the formulas)."""
import numpy as np

NFFT = 2048
HOP = 1024
BAND_HZ = 768e3


def as_complex(x):
    """The samples the device gets as complex128: complex64 as it is, int16 / int8 pairs as they are, uint8 pairs - 128."""
    x = np.asarray(x).reshape(-1)
    if x.dtype == np.uint8:
        p = x.reshape(-1, 2).astype(np.float64) - 128.0
        return p[:, 0] + 1j * p[:, 1]
    if x.dtype in (np.int16, np.int8):
        p = x.reshape(-1, 2).astype(np.float64)
        return p[:, 0] + 1j * p[:, 1]
    return x.astype(np.complex128)


def n_segments(n_samples):
    return (n_samples - NFFT) // HOP + 1 if n_samples >= NFFT else 0


def welch_raw(x, window):
    """(raw, segments): raw[k] = sum over the segments of |FFT(w x_seg)[k]|^2, segment i = samples 1024 i ... 1024 i + 2047;
    window: the fp32 table, taken to float64."""
    x = as_complex(x)
    w = np.asarray(window, np.float32).astype(np.float64)
    assert w.size == NFFT
    n = n_segments(x.size)
    raw = np.zeros(NFFT, np.float64)
    for i in range(n):
        X = np.fft.fft(x[i * HOP: i * HOP + NFFT] * w)
        raw += X.real ** 2 + X.imag ** 2
    return raw, n


def window_formula(window):
    """Periodic form in float64: 0 rectangular, 1 Hann, 2 four-term Blackman-Harris."""
    x = 2.0 * np.pi * np.arange(NFFT) / NFFT
    if window == 0:
        return np.ones(NFFT)
    if window == 1:
        return 0.5 - 0.5 * np.cos(x)
    if window == 2:
        return 0.35875 - 0.48829 * np.cos(x) + 0.14128 * np.cos(2 * x) - 0.01168 * np.cos(3 * x)
    raise ValueError(window)


def bin_freqs(nfft, rate_hz):
    k = np.arange(nfft)
    return np.where(k < nfft // 2, k, k - nfft) * (rate_hz / nfft)


def check_mask_model(raw, rate_hz, mask=(), oob_from_hz=970e3):
    """The mask rule restated: ref = mean of raw over 0 < |f| <= 768 kHz, level = 10 log10(raw / ref), limit piecewise linear
    in dB between the points (held beyond the last, unchecked below the first)."""
    raw = np.asarray(raw, np.float64)
    f = bin_freqs(raw.size, rate_hz)
    af = np.abs(f)
    band = (af > 0) & (af <= BAND_HZ)
    ref = raw[band].mean()
    with np.errstate(divide="ignore"):
        level = 10.0 * np.log10(raw / ref)
    out = {"ref": float(ref), "level": level, "freqs": f, "worst_margin_db": 0.0, "worst_freq_hz": 0.0, "n_violations": 0,
           "n_checked": 0}
    oob = af >= oob_from_hz
    if oob.any():
        k = int(np.flatnonzero(oob)[np.argmax(level[oob])])
        out["oob_max_db"], out["oob_freq_hz"] = float(level[k]), float(f[k])
    else:
        out["oob_max_db"], out["oob_freq_hz"] = -np.inf, 0.0
    pts = np.asarray(mask, np.float64).reshape(-1, 2)
    if pts.shape[0]:
        sel = af >= pts[0, 0]
        limit = np.interp(af[sel], pts[:, 0], pts[:, 1])      # (np.interp holds the end values)
        margin = limit - level[sel]
        k = int(np.argmin(margin))
        out.update(worst_margin_db=float(margin[k]), worst_freq_hz=float(f[sel][k]),
                   n_violations=int(np.sum(level[sel] > limit)), n_checked=int(sel.sum()))
    return out
