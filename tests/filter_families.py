"""A deterministic table of FIRFilter tap sets around the gate of the frame kernel's equalised-boundary form (helper: no tests
here).  design_inverse_filter (csrc/api_context.hip) admits taps whose 160-tap inverse on the occupied carriers fits to
fit < 1e-7 with a noise gain sum(g^2) < 4; everything else keeps the packed dual transform.  The families below move the
filter's SHAPE across both thresholds -- cutoff, window, length, delay, tilt / droop, scale -- and add the shapes the gate
refuses outright.  Built with scipy.signal and numpy alone; every member is float32 with at most 45 taps, but for the one
46-tap member that the kernel's tap count refuses.

VERDICTS is tabulated from the library (pkg.fir_inverse_design on every member; `python -m tests.filter_families` prints
the table in this form), not from a model of it:
    "eq"    admitted: the equalised-boundary form runs
    "fit"   refused on the fit alone        (fit >= 1e-7, sum(g^2) < 4)
    "norm"  refused on the noise gain alone (fit < 1e-7, sum(g^2) >= 4)
    "both"  refused on both
    "none"  refused before a fit exists (a zero of H on an occupied bin, or more than 45 taps)
tests/test_cabi_cpu.py holds the table to the library and to the conditions that keep it from going soft."""
import numpy as np

FS = 2.048e6
FIT_LIMIT, NORM2_LIMIT = 1e-7, 4.0          # the gate's two constants (design_inverse_filter's return statement)
N, K = 2048, 1536                           # Mode I: FFT size, occupied carriers
OCC = np.r_[1:K // 2 + 1, N - K // 2:N]
EQ_TAPS, EQ_CENTRE = 160, 56                # the inverse filter's length and its centre tap (kEqTaps, kEqCentre)


def _lp(ntaps, cutoff, window="hamming"):
    from scipy.signal import firwin
    return firwin(ntaps, cutoff, window=window, fs=FS)


def _pad45(t, at=0):
    out = np.zeros(45)
    out[at:at + len(t)] = t
    return out


def families():
    """name -> float32 taps, in a fixed order."""
    import oracle as O
    fam = {}
    fam["default"] = O.fir_default_taps().astype(np.float64)
    # cutoff sweep: 45-tap Hamming low-passes; the occupied band ends at 768 kHz
    for kHz in (765, 770, 775, 780, 785, 790, 800, 900, 1000):
        fam["cut%d" % kHz] = _lp(45, kHz * 1e3)
    # ... and the narrow ones rescaled: the fit does not move with the scale, the noise gain does, so these sit on ONE threshold
    fam["cut760x2"] = 2.0 * _lp(45, 760e3)
    fam["cut765x2"] = 2.0 * _lp(45, 765e3)
    fam["cut780x0.75"] = 0.75 * _lp(45, 780e3)
    fam["cut780x0.5"] = 0.5 * _lp(45, 780e3)
    # other windows
    fam["kaiser5_900"] = _lp(45, 900e3, ("kaiser", 5.0))
    fam["boxcar_900"] = _lp(45, 900e3, "boxcar")
    # length sweep, odd and even
    for nt in (5, 21, 30, 37, 44):
        fam["len%d" % nt] = _lp(nt, 900e3)
    # delay family: a 25-tap low-pass somewhere inside 45 taps, and unit impulses
    lp25 = _lp(25, 900e3)
    for at in (0, 13, 20):
        fam["lp25_at%d" % at] = _pad45(lp25, at)
    for at in (0, 22, 44):
        fam["impulse%d" % at] = _pad45([1.0], at)
    # tilt and droop: a 43-tap low-pass convolved with a short shaping filter, up to a zero inside the band
    lp43 = _lp(43, 900e3)
    fam["droop_m0.2"] = np.convolve(lp43, [-0.1, 1.0, -0.1])          # [-t/2, 1, -t/2], t = 0.2: rises towards the band edge
    fam["droop_p0.2"] = np.convolve(lp43, [0.2, 0.6, 0.2])            # [t, 1 - 2t, t], t = 0.2: falls towards the band edge
    fam["droop_p0.25"] = np.convolve(lp43, [0.25, 0.5, 0.25])         # ... t = 0.25: a zero at fs / 2, 17 dB down at the band edge
    fam["droop_p0.25x2"] = 2.0 * fam["droop_p0.25"]
    fam["droop_p0.38"] = np.convolve(lp43, [0.38, 0.24, 0.38])        # ... t = 0.38: the zero is inside the band (near bin 616)
    lp44 = _lp(44, 900e3)
    fam["tilt0.3"] = np.convolve(lp44, [1.0, -0.3])                   # the asymmetric [1, -t]
    fam["tilt0.7"] = np.convolve(lp44, [1.0, -0.7])
    fam["tilt1.0"] = np.convolve(lp44, [1.0, -1.0])                   # t = 1: the zero sits on DC, next to the first occupied bin
    # scale family: one good low-pass
    for sc in (0.4, 0.5, 0.7, 2.0, 10.0, -1.0):
        fam["scale%g" % sc] = sc * _lp(45, 900e3)
    # shapes the gate refuses: the notch of test_fir_inverse_design..., random taps, 46 taps
    fam["notch300"] = np.convolve(fam["default"][:43], [1, -2 * np.cos(2 * np.pi * 300 / N), 1])
    fam["random"] = np.random.RandomState(45).standard_normal(45) / 8.0
    fam["taps46"] = _lp(46, 900e3)
    return {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in fam.items()}


# tabulated from the library (python -m tests.filter_families); the figures behind each verdict ride along as comments
# (fp32: fp32_filter_error relative to the default taps')
VERDICTS = {
    "default":       "eq",    # fit 3.25e-08  sum g^2 0.9579  fp32 1.00 x default
    "cut765":        "both",  # fit 1.13e-07  sum g^2 7.393  fp32 1.01 x default
    "cut770":        "norm",  # fit 9.52e-08  sum g^2 4.527  fp32 0.99 x default
    "cut775":        "eq",    # fit 9.46e-08  sum g^2 3.021  fp32 0.88 x default
    "cut780":        "eq",    # fit 7.35e-08  sum g^2 2.186  fp32 1.00 x default
    "cut785":        "eq",    # fit 9.73e-08  sum g^2 1.7  fp32 0.92 x default
    "cut790":        "eq",    # fit 4.97e-08  sum g^2 1.405  fp32 1.13 x default
    "cut800":        "eq",    # fit 2.93e-08  sum g^2 1.096  fp32 1.21 x default
    "cut900":        "eq",    # fit 2.85e-08  sum g^2 0.8107  fp32 1.06 x default
    "cut1000":       "eq",    # fit 3.8e-08  sum g^2 0.8106  fp32 0.97 x default
    "cut760x2":      "fit",   # fit 1.8e-07  sum g^2 3.295  fp32 0.94 x default
    "cut765x2":      "fit",   # fit 1.13e-07  sum g^2 1.848  fp32 1.01 x default
    "cut780x0.75":   "eq",    # fit 5.37e-08  sum g^2 3.885  fp32 0.92 x default
    "cut780x0.5":    "norm",  # fit 7.35e-08  sum g^2 8.742  fp32 1.00 x default
    "kaiser5_900":   "eq",    # fit 2.85e-08  sum g^2 0.8117  fp32 0.85 x default
    "boxcar_900":    "eq",    # fit 4.36e-08  sum g^2 0.7851  fp32 0.98 x default
    "len5":          "eq",    # fit 4.14e-08  sum g^2 1.004  fp32 0.48 x default
    "len21":         "eq",    # fit 4.46e-08  sum g^2 0.8338  fp32 0.74 x default
    "len30":         "eq",    # fit 4.26e-08  sum g^2 0.8198  fp32 0.88 x default
    "len37":         "eq",    # fit 2.71e-08  sum g^2 0.8127  fp32 0.89 x default
    "len44":         "eq",    # fit 2.92e-08  sum g^2 0.8137  fp32 1.23 x default
    "lp25_at0":      "eq",    # fit 3.79e-08  sum g^2 0.8271  fp32 0.92 x default
    "lp25_at13":     "eq",    # fit 3.33e-08  sum g^2 0.8225  fp32 0.92 x default
    "lp25_at20":     "eq",    # fit 2.5e-08  sum g^2 0.8239  fp32 0.92 x default
    "impulse0":      "eq",    # fit 1.88e-08  sum g^2 0.8281  fp32 0.00 x default
    "impulse22":     "eq",    # fit 2.47e-08  sum g^2 0.8123  fp32 0.00 x default
    "impulse44":     "eq",    # fit 4.17e-08  sum g^2 0.8251  fp32 0.00 x default
    "droop_m0.2":    "eq",    # fit 3.21e-08  sum g^2 0.9323  fp32 1.00 x default
    "droop_p0.2":    "eq",    # fit 4.8e-08  sum g^2 2.84  fp32 1.17 x default
    "droop_p0.25":   "both",  # fit 1.2e-07  sum g^2 9.559  fp32 1.12 x default
    "droop_p0.25x2": "fit",   # fit 1.2e-07  sum g^2 2.39  fp32 1.12 x default
    "droop_p0.38":   "both",  # fit 2.49  sum g^2 6.708e+14  fp32 0.82 x default
    "tilt0.3":       "eq",    # fit 3.22e-08  sum g^2 0.9869  fp32 1.07 x default
    "tilt0.7":       "eq",    # fit 3.1e-08  sum g^2 1.896  fp32 0.87 x default
    "tilt1.0":       "both",  # fit 2.46  sum g^2 1.252e+14  fp32 0.77 x default
    "scale0.4":      "norm",  # fit 2.24e-08  sum g^2 5.067  fp32 0.98 x default
    "scale0.5":      "eq",    # fit 2.85e-08  sum g^2 3.243  fp32 1.06 x default
    "scale0.7":      "eq",    # fit 3.13e-08  sum g^2 1.654  fp32 1.04 x default
    "scale2":        "eq",    # fit 2.85e-08  sum g^2 0.2027  fp32 1.06 x default
    "scale10":       "eq",    # fit 2.8e-08  sum g^2 0.008107  fp32 1.02 x default
    "scale-1":       "eq",    # fit 2.85e-08  sum g^2 0.8107  fp32 1.06 x default
    "notch300":      "none",  # fit 0  sum g^2 0  fp32 1.19 x default
    "random":        "both",  # fit 0.816  sum g^2 1.268e+12  fp32 1.03 x default
    "taps46":        "none",  # fit 0  sum g^2 0  fp32 1.15 x default
}


# The members the other equalised forms are run on (windowed, integer stores, TII, Mode IV): the three nearest each threshold
# of the gate (by the ratio to the threshold, admitted or not; cut770 is among the three of both), one more admitted member high
# on the noise gain, one tilt, one delay and the default taps.  tests/test_cabi_cpu.py checks "nearest" on the library's figures.
NEAREST_FIT = ("cut785", "cut770", "cut775")
NEAREST_NORM = ("cut780x0.75", "cut770", "cut760x2")
SUBSET = ("cut785", "cut770", "cut775", "cut780x0.75", "cut760x2", "scale0.5", "tilt0.7", "lp25_at20", "default")


def classify(ok, fit, g):
    """The verdict string of one pkg.fir_inverse_design result, by the gate's constants."""
    norm2 = float((g.astype(np.float64) ** 2).sum())
    if ok:
        return "eq"
    if fit == 0.0 and norm2 == 0.0:
        return "none"
    bad_fit, bad_norm = not fit < FIT_LIMIT, not norm2 < NORM2_LIMIT
    return "both" if bad_fit and bad_norm else "fit" if bad_fit else "norm" if bad_norm else "none"


def response(taps, n=N):
    """H[k] = sum_j taps[j] exp(+2 pi i k j / n): the filter is out[m] = sum_j taps[j] in[m + j] (float64)."""
    t = np.asarray(taps, np.float64)
    return (t[None, :] * np.exp(2j * np.pi * np.outer(np.arange(n), np.arange(t.size)) / n)).sum(1)


def inverse_response(g, n=N):
    g = np.asarray(g, np.float64)
    return (g[None, :] * np.exp(-2j * np.pi * np.outer(np.arange(n), np.arange(g.size) - EQ_CENTRE) / n)).sum(1)


def fp32_filter_error(taps, seed=11, nsym=4):
    """What float32 filtering itself leaves on these taps: max |fp32 - float64| of out[m] = sum_j taps[j] x[m + j] over an
    OFDM-like stream (nsym Mode I symbols of unit-modulus carriers on the occupied bins, float32 samples), relative to
    the largest float64 output.  The float32 evaluation accumulates tap by tap in float32, products rounded, as a
    straightforward kernel would."""
    rs = np.random.RandomState(seed)
    x = []
    for _ in range(nsym):
        X = np.zeros(N, complex)
        X[OCC] = np.exp(1j * np.pi / 4 * (2 * rs.randint(0, 4, K) + 1))
        x.append(np.fft.ifft(X) * N)
    x = np.concatenate(x).astype(np.complex64)
    t32 = np.asarray(taps, np.float32)
    m = x.size - t32.size
    acc = np.zeros(m, np.complex64)
    for j in range(t32.size):
        seg = x[j:j + m]
        p = (seg.real * t32[j]).astype(np.float32) + 1j * (seg.imag * t32[j]).astype(np.float32)
        acc = (acc + p.astype(np.complex64)).astype(np.complex64)
    exact = np.zeros(m, np.complex128)
    for j in range(t32.size):
        exact += float(t32[j]) * x[j:j + m].astype(np.complex128)
    return float(np.abs(acc.astype(np.complex128) - exact).max() / np.abs(exact).max())


def boundary_members():
    """The members whose boundary outputs are held to the 7e-7 bar, in whichever form the chain runs them (admitted or
    refused): those for which float32 filtering itself leaves room, i.e. whose fp32_filter_error is at most 1.5 x the default
    taps' own."""
    fam = families()
    base = fp32_filter_error(fam["default"])
    return [n for n, t in fam.items() if fp32_filter_error(t) <= 1.5 * base]


if __name__ == "__main__":
    from tests.conftest import load_pkg
    pkg = load_pkg()
    fam = families()
    base = fp32_filter_error(fam["default"])
    for name, taps in fam.items():
        ok, g, fit = pkg.fir_inverse_design(taps)
        print('    %-16s %-8s # fit %.3g  sum g^2 %.4g  fp32 %.2f x default' % (
            '"%s":' % name, '"%s",' % classify(ok, fit, g), fit, float((g.astype(np.float64) ** 2).sum()),
            fp32_filter_error(taps) / base))
