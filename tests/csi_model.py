"""Float64 / integer numpy model of the carrier state (include/dabgpu.h, "the carrier state"), written from the header alone and
independent of the device code, on the steps of tests/soft_model.py: window, FFT, the occupied bins in frequency order,
d = z_s conj(z_{s-1}), q_s = 64 sqrt(2) / sqrt(P_s / K), u = d q_s.

    A_k = sum_s rint(2^F (|Re u| + |Im u|) / 2),  V_k = sum_s rint(2^F (|Im u| - |Re u|)^2 / 2)       (int64)
    SA, SV, n the integer totals and the size of the trimmed set T (three passes: V_k n_i <= 4 SV_i); SA = 0 or SV = 0: w = 1;
    else w_k = float32(min(MAX, (A_k SV) / (SA max(V_k, SV / (64 n)))))
    soft = clamp(rint(-Re d q w_k)), clamp(rint(-Im d q w_k)); per block the I softs in interleaver-undone order, then the Q softs

Every float64 operation of the weights is a single correctly rounded IEEE operation, in the header's order: numpy gives the
device's bits where the device's operations are correctly rounded too."""
import numpy as np

from tests.demod_model import as_complex
from tests.receiver import MODES
from tests.soft_model import carrier_order

FRAC_BITS, MAX_WEIGHT, TRIM_PASSES, TRIM_FACTOR = 16, 4.0, 3, 4


def header_constants(text):
    """(FRAC_BITS, MAX_WEIGHT, TRIM_PASSES, TRIM_FACTOR) as include/dabgpu.h defines them"""
    import re
    return tuple(int(re.search(r"#define DABGPU_CSI_%s (\d+)" % k, text).group(1))
                 for k in ("FRAC_BITS", "MAX_WEIGHT", "TRIM_PASSES", "TRIM_FACTOR"))


def scaled_d(y, mode, early=0):
    """One frame -> u = d q, (nb_symbols - 1, K) complex128 by carrier position"""
    y = as_complex(y)
    N, K, nsym, null, sym = MODES[mode]
    z = np.empty((nsym, K), np.complex128)
    for s in range(nsym):
        seg = y[null + s * sym: null + (s + 1) * sym]
        X = np.fft.fft(seg[sym - N - early: sym - early])
        z[s, :K // 2] = X[1:K // 2 + 1]
        z[s, K // 2:] = X[N - K // 2:]
    d = z[1:] * np.conj(z[:-1])
    P = np.sum(np.abs(d) ** 2, axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(P > 0, 64.0 * np.sqrt(2.0) / np.sqrt(P / K), 0.0)
    return d * q[:, None]


def terms(u):
    """u -> the two terms per symbol and carrier before rint, in units of 2^-F"""
    ar, ai = np.abs(u.real), np.abs(u.imag)
    return 2.0 ** FRAC_BITS * (ar + ai) / 2.0, 2.0 ** FRAC_BITS * (ai - ar) ** 2 / 2.0


def sums(u):
    """u -> (A, V) int64 per carrier position"""
    ta, tv = terms(u)
    return np.rint(ta).astype(np.int64).sum(axis=0), np.rint(tv).astype(np.int64).sum(axis=0)


def weights(A, V):
    """(A, V) int64 -> float32 weights per carrier position"""
    A, V = np.asarray(A, np.int64), np.asarray(V, np.int64)
    K = A.size
    keep = np.ones(K, bool)
    for _ in range(TRIM_PASSES):
        n, sv = int(keep.sum()), int(V[keep].sum())
        keep = np.array([int(v) * n <= TRIM_FACTOR * sv for v in V])          # Python integers: no overflow to think about
    n, SA, SV = int(keep.sum()), int(A[keep].sum()), int(V[keep].sum())
    if SA == 0 or SV == 0:
        return np.ones(K, np.float32)
    sa, sv = np.float64(SA), np.float64(SV)
    floor = sv / np.float64(64 * n)
    r = (A.astype(np.float64) * sv) / (sa * np.maximum(V.astype(np.float64), floor))
    return np.minimum(np.float64(MAX_WEIGHT), r).astype(np.float32)


def softs_of(u, w, mode, exact=False):
    """u and per-position weights -> the frame's softs (exact=True: the float64 values before rint and clamp)"""
    v = (u * np.asarray(w, np.float64)[None, :])[:, carrier_order(mode)]
    x = np.concatenate([-v.real, -v.imag], axis=1).reshape(-1)
    if exact:
        return x
    return np.clip(np.rint(x), -127, 127).astype(np.int8)


def demod_csi_model(y, mode, early=0, exact=False):
    """One frame of native-rate samples -> dict(soft, A, V, w)"""
    u = scaled_d(y, mode, early)
    A, V = sums(u)
    w = weights(A, V)
    return {"soft": softs_of(u, w, mode, exact), "A": A, "V": V, "w": w, "u": u}


def mer_db(A, V, mode):
    """the header's per-carrier MER"""
    S = MODES[mode][2] - 1
    with np.errstate(divide="ignore", invalid="ignore"):
        return 20.0 * np.log10(np.asarray(A, np.float64) / np.sqrt(2.0 ** (FRAC_BITS - 1) * S * np.asarray(V, np.float64)))


def tone_comb(n_samples, mode, bins, power):
    """A comb of unmodulated tones over a whole stream of n_samples: tone j at `bins[j]` carrier spacings from the centre
    frequency, phase continuous over the stream, the comb's total power `power` split evenly.  -> complex128"""
    N = MODES[mode][0]
    t = np.arange(n_samples, dtype=np.float64)
    amp = np.sqrt(power / len(bins))
    y = np.zeros(n_samples, np.complex128)
    for j, b in enumerate(bins):
        y += amp * np.exp(2j * np.pi * ((b / N) * t + 0.1 * j))
    return y
