"""The yardstick of the DPD measurement (include/dabgpu.h, "DPD measurement") in float64 numpy: cross-spectrum, alignment
solve, delay taps, amplitude-bin statistics and both polynomial fits.  Independent of the device code.  What both sides must
share is shared on purpose: the fp32 squared magnitude of a tx sample (two products and a sum, each rounded) and the fp32
table of squared bin edges decide the bin, so the counts can be compared exactly; the statistics take the fp32 taps and the
fp32 gain as inputs, because that is what the device is handed."""
import numpy as np

NFFT, HOP = 2048, 1024
TAPS, CENTRE = 32, 15
KAISER_BETA, KAISER_HALF = 10.0, 16.0


def tx_complex(tx):
    """complex64 as it is, int16 pairs as they are -- as complex128."""
    tx = np.asarray(tx).reshape(-1)
    if tx.dtype == np.int16:
        p = tx.reshape(-1, 2).astype(np.float64)
        return p[:, 0] + 1j * p[:, 1]
    return tx.astype(np.complex128)


def segments(n, rx_offset):
    """The segments i whose rx range 1024 i + rx_offset ... + 2047 lies inside the n samples."""
    n_seg = (n - NFFT) // HOP + 1 if n >= NFFT else 0
    return [i for i in range(n_seg) if HOP * i + rx_offset >= 0 and HOP * i + rx_offset + NFFT <= n]


def xspectrum(tx, rx, rx_offset=0):
    """(S, p_tx, p_rx, segments): S[k] = sum TX[k] conj(RX[k]) over the segments, rectangular window."""
    t, r = tx_complex(tx), np.asarray(rx).reshape(-1).astype(np.complex128)
    S, pt, pr = np.zeros(NFFT, np.complex128), np.zeros(NFFT), np.zeros(NFFT)
    segs = segments(t.size, rx_offset)
    for i in segs:
        T = np.fft.fft(t[HOP * i: HOP * i + NFFT])
        R = np.fft.fft(r[HOP * i + rx_offset: HOP * i + rx_offset + NFFT])
        S += T * np.conj(R)
        pt += np.abs(T) ** 2
        pr += np.abs(R) ** 2
    return S, pt, pr, len(segs)


def _omega():
    k = np.arange(NFFT)
    return 2.0 * np.pi * np.where(k < NFFT // 2, k, k - NFFT) / NFFT


def solve_alignment(S, p_tx, p_rx):
    """lag, tau, gain, coherence by the rule of the header: the largest |IDFT(conj S)|, a scan at 1/32 sample and bisection
    on the derivative of |sum conj(S) e^{j w d}|^2."""
    S = np.asarray(S, np.complex128)
    c = np.fft.ifft(np.conj(S))
    l = int(np.argmax(np.abs(c)))
    lag = l if l < NFFT // 2 else l - NFFT
    w, cs = _omega(), np.conj(S)

    def corr(d):
        return np.sum(cs * np.exp(1j * w * d))

    def slope(d):
        e = cs * np.exp(1j * w * d)
        a, b = np.sum(e), np.sum(1j * w * e)
        return 2.0 * (a.real * b.real + a.imag * b.imag)

    step = 1.0 / 32.0
    grid = np.arange(-31, 32)
    bi = int(grid[np.argmax([abs(corr(lag + step * i)) for i in grid])])
    lo, hi = step * (bi - 1), step * (bi + 1)
    if not slope(lag + lo) > 0:
        tau = lo
    elif not slope(lag + hi) < 0:
        tau = hi
    else:
        while hi - lo > 1e-13:
            mid = 0.5 * (lo + hi)
            if slope(lag + mid) > 0:
                lo = mid
            else:
                hi = mid
        tau = 0.5 * (lo + hi)
    a = np.conj(corr(lag + tau))                    # sum S e^{-j w d}
    return {"lag": lag, "tau": float(tau), "gain": complex(a / np.sum(p_rx)),
            "coherence": float(abs(a) ** 2 / (np.sum(p_tx) * np.sum(p_rx)))}


def delay_taps(tau):
    """float64: sinc(m - tau) kaiser(m - tau), m = j - 15, beta 10 over +-16 samples around the sinc's peak."""
    m = np.arange(TAPS) - CENTRE
    x = m - tau
    u = x / KAISER_HALF
    win = np.where(np.abs(u) < 1.0, np.i0(KAISER_BETA * np.sqrt(np.clip(1.0 - u * u, 0.0, None))) / np.i0(KAISER_BETA), 0.0)
    return np.sinc(x) * win


def edges2(peak, n_bins):
    """The fp32 table of squared bin edges, formed in float64."""
    e = np.arange(n_bins + 1, dtype=np.float64) * float(np.float32(peak)) / n_bins
    return (e * e).astype(np.float32)


def magsq_fp32(t):
    """re re + im im of complex128 values that are exact fp32 pairs, every operation rounded to fp32."""
    re, im = t.real.astype(np.float32), t.imag.astype(np.float32)
    return re * re + im * im


def stats(tx, rx, lag=0, tau=0.0, gain=1.0, peak=1.0, n_bins=64, taps=None):
    """The statistics of the header in float64.  taps: the fp32 taps the device runs (default: delay_taps(tau) rounded to
    fp32); gain is rounded to fp32 as the device's argument is.  Returns counts, sums, overflow and samples used."""
    t, r = tx_complex(tx), np.asarray(rx).reshape(-1).astype(np.complex128)
    n = t.size
    h = (delay_taps(tau).astype(np.float32) if taps is None else np.asarray(taps, np.float32)).astype(np.float64)
    g = complex(np.complex64(gain))
    i0, i1 = max(0, CENTRE - lag), min(n, n - (TAPS - 1 - CENTRE) - lag)
    out = {"n_bins": n_bins, "peak": float(np.float32(peak)), "count": np.zeros(n_bins, np.int64), "overflow": 0, "samples_used": 0}
    for name in ("sum_tx", "sum_rx", "sum_phase", "sum_rx2", "sum_phase2"):
        out[name] = np.zeros(n_bins, np.float64)
    if i1 <= i0:
        return out
    # aligned[i - i0] = sum_j h[j] rx[i + lag + j - 15]
    first = i0 + lag - CENTRE
    aligned = g * np.correlate(r[first: first + (i1 - i0) + TAPS - 1], h, mode="valid")
    tt = t[i0:i1]
    a2 = magsq_fp32(tt)
    b = np.searchsorted(edges2(peak, n_bins)[1:], a2, side="right")       # #{ j >= 1 : edge2[j] <= a2 }
    over = b >= n_bins
    out["overflow"], out["samples_used"] = int(over.sum()), int(tt.size)
    keep = ~over
    b, tt, rr = b[keep], tt[keep], aligned[keep]
    at = np.abs(tt)
    ar = np.minimum(np.abs(rr), 16.0 * out["peak"])
    phi = np.angle(rr * np.conj(tt))
    out["count"] = np.bincount(b, minlength=n_bins).astype(np.int64)
    for name, v in (("sum_tx", at), ("sum_rx", ar), ("sum_phase", phi), ("sum_rx2", ar * ar), ("sum_phase2", phi * phi)):
        out[name] = np.bincount(b, weights=v, minlength=n_bins)
    return out


def fit_poly(st, basis="magsq", min_count=1, weighted=True, tx_min=0.0):
    """(am, pm) in float64 by numpy's least squares; the two bases of the header."""
    n_bins, peak = st["n_bins"], float(np.float32(st["peak"]))
    cnt = np.asarray(st["count"][:n_bins], np.float64)
    ok = cnt >= max(1, min_count)
    if basis == "reference":
        run = int(np.argmin(ok)) if not ok.all() else n_bins
        ok = np.arange(n_bins) < run
    idx = np.flatnonzero(ok)
    n = cnt[idx]
    t, r, p = st["sum_tx"][idx] / n, st["sum_rx"][idx] / n, st["sum_phase"][idx] / n
    w = np.sqrt(n) if weighted else np.ones_like(n)
    if basis == "reference":
        t = ((idx + 0.5) * peak / n_bins).astype(np.float32)
        r, p = r.astype(np.float32), p.astype(np.float32)
        p = np.where(t < tx_min, np.float32(0), p)
        t, r, p = t.astype(np.float64), r.astype(np.float64), p.astype(np.float64)
        # (fp32 values; their powers rounded once to fp32, as Model_Poly's `sig ** i` on float32 arrays gives them where the
        # float32 power is the correctly rounded one)
        A = np.array([(r ** i).astype(np.float32) for i in range(1, 6)]).T.astype(np.float64)
        B = np.array([(t ** i).astype(np.float32) for i in range(0, 5)]).T.astype(np.float64)
    else:
        A = np.array([r ** (2 * i + 1) for i in range(5)]).T
        B = np.array([r ** (2 * i) for i in range(5)]).T
    # (columns scaled by the largest abscissa: numpy's SVD does not need it, the condition number it reports does)
    am = np.linalg.lstsq(A * w[:, None], t * w, rcond=None)[0]
    pm = np.linalg.lstsq(B * w[:, None], p * w, rcond=None)[0]
    return am, pm
