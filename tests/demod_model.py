"""The yardstick of the on-device receiver: the per-frame figures of include/dabgpu.h ("the receiver") in float64 numpy, on the
steps of tests/receiver.py (dab_demodulate: window, FFT, the occupied bins in carrier order, z_s conj(z_{s-1})).  Independent
of the device code; the bits are dab_demodulate's own."""
import numpy as np

from tests.receiver import MODES, dab_demodulate


def as_complex(y):
    """One frame as complex128: complex input as it is, int16 input as interleaved (re, im) pairs."""
    y = np.asarray(y)
    if y.dtype == np.int16:
        y = y.reshape(-1, 2).astype(np.float64)
        return y[:, 0] + 1j * y[:, 1]
    return y.astype(np.complex128)


def demod_model(y, mode, early=0, ref_bits=None):
    """One frame of native-rate samples -> dict(bits, sum_signal, sum_quadrature, min_margin, bit_errors, n_bits)."""
    y = as_complex(y)
    N, K, nsym, null, sym = MODES[mode]
    z = np.empty((nsym, K), np.complex128)
    for s in range(nsym):
        seg = y[null + s * sym: null + (s + 1) * sym]
        X = np.fft.fft(seg[sym - N - early: sym - early])
        z[s, :K // 2] = X[1:K // 2 + 1]
        z[s, K // 2:] = X[N - K // 2:]
    d = z[1:] * np.conj(z[:-1])
    c = ((1.0 - 2.0 * (d.real < 0)) + 1j * (1.0 - 2.0 * (d.imag < 0))) / np.sqrt(2.0)      # the decided point
    mag = np.abs(d)
    with np.errstate(divide="ignore", invalid="ignore"):
        margin = np.where(mag > 0, np.minimum(np.abs(d.real), np.abs(d.imag)) / mag, 0.0)
    bits = dab_demodulate(y, mode, early)
    out = {"bits": bits, "sum_signal": float(np.sum(mag ** 2)),
           "sum_quadrature": float(np.sum((d * np.conj(c)).imag ** 2)), "min_margin": float(margin.min()),
           "bit_errors": 0, "n_bits": 0}
    if ref_bits is not None:
        ref = np.asarray(ref_bits, np.uint8).reshape(-1)
        out["bit_errors"] = int(np.unpackbits(bits ^ ref).sum())
        out["n_bits"] = 8 * ref.size
    return out


def mer_db(st):
    return 10.0 * np.log10(st["sum_signal"] / st["sum_quadrature"])


def auto_early(ntaps_in_mask, overlap):
    """The monitor's automatic window position: FIRFilter looks ntaps - 1 samples ahead, the guard window's overlap reaches
    as far into the symbol's end."""
    return (ntaps_in_mask - 1 if ntaps_in_mask else 0) + (overlap if overlap > 0 else 0)
