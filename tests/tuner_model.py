"""The tuner of include/dabgpu.h ("the tuner") in float64 numpy and Python integers, written from the header's text: the ratio,
the tap formula, the count of outputs and the mixer + polyphase decimator as a stream (Tuner).  The stream runs on the rows
of the tap table the library returns (host-only getter), as tests/clock_model.py does: what is modelled there is the arithmetic
built on them; the rows themselves are held to formula_taps by tests/test_tuner_cpu.py."""
import functools
import math

import numpy as np

from tests.channel_model import as_samples, to_s16  # noqa: F401  (to_s16: for the tests)

NATIVE = 2048000
MAX_L, MAX_TAPS = 512, 768
MAX_POSITION = 2 ** 50
BANDWIDTH = (2048000.0, 1712000.0)                # wide, channel: twice the -6 dB frequency


def geometry(in_rate, selectivity):
    """(L, M, P) by the header's rule; None where the rate is refused"""
    in_rate = int(in_rate)
    if in_rate < NATIVE:
        return None
    g = math.gcd(NATIVE, in_rate)
    L, M = NATIVE // g, in_rate // g
    if L > MAX_L or M > 8 * L or selectivity not in (0, 1):
        return None
    D = -(-M // L)
    return L, M, (96 if selectivity else 32) * D


def step_of(in_rate, offset_hz):
    """rint(-offset_hz / in_rate 2^64) as a Python integer (the quotient and the product in float64, from the left)"""
    v = -float(offset_hz) / float(in_rate) * 18446744073709551616.0
    return int(np.rint(v))


def bessel_i0(x):
    term, total = 1.0, 1.0
    for k in range(1, 256):
        term *= (x / (2.0 * k)) * (x / (2.0 * k))
        total += term
        if term < 1e-18 * total:
            break
    return total


def sinc_exact(x):
    """1 at 0, exactly 0 at every other integer: (-1)^n sin(pi (x - n)) / (pi x), n = x rounded to the nearest integer"""
    if x == 0.0:
        return 1.0
    n = round(x)                                   # ties to even, as nearbyint
    s = math.sin(math.pi * (x - n))
    if n % 2:
        s = -s
    return s / (math.pi * x)


def formula_taps(in_rate, selectivity, p):
    """row p in float64 before the last rounding: h_j / sum_j h_j, the sum in the order j = 0 ... P - 1"""
    L, M, P = geometry(in_rate, selectivity)
    c = min(1.0, BANDWIDTH[selectivity] / float(in_rate))
    half, i0b = float(P // 2), bessel_i0(10.0)
    h = []
    for j in range(P):
        t = float(j - (P // 2 - 1)) - float(p) / float(L)
        u = t / half
        h.append(c * sinc_exact(c * t) * bessel_i0(10.0 * math.sqrt(max(0.0, 1.0 - u * u))) / i0b if abs(t) <= half else 0.0)
    total = 0.0
    for v in h:
        total += v
    return np.array([v / total + 0.0 for v in h], np.float64)


@functools.lru_cache(maxsize=None)
def table(pkg, in_rate, selectivity):
    """the L rows the library runs on, fp32; do not write to it"""
    L, M, P = pkg.tuner_geometry(in_rate, selectivity)
    t = np.stack([pkg.tuner_taps(in_rate, selectivity, p) for p in range(L)])
    assert t.dtype == np.float32 and t.shape == (L, P)
    t.setflags(write=False)
    return t


def count(L, M, P, T):
    """M(T) by the definition: the number of m >= 0 with (m M) div L + P/2 <= T - 1, by bisection (i_m does not decrease)"""
    T = int(T)
    ok = lambda m: (m * M) // L + P // 2 <= T - 1  # noqa: E731
    if not ok(0):
        return 0
    lo, hi = 0, T + 1                              # (M >= L: i_m >= m, m = T + 1 lies behind T)
    assert not ok(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if ok(mid):
            lo = mid
        else:
            hi = mid
    return hi


def response(row_taps, L, freqs_hz, in_rate, p):
    """the frequency response of one row, float64, with the row's own fractional delay taken off: sum_j T[p][j] e^{-j w t_j}"""
    P = row_taps.size
    t = np.arange(P) - (P // 2 - 1) - p / float(L)
    w = 2.0 * np.pi * np.asarray(freqs_hz, np.float64) / float(in_rate)
    return np.exp(-1j * np.outer(w, t)) @ row_taps.astype(np.float64)


class Tuner:
    """One stream.  pkg: the package (the table comes from its host-only function)."""

    def __init__(self, pkg, in_rate, selectivity=0, offset_hz=0.0):
        self.L, self.M, self.P = pkg.tuner_geometry(in_rate, selectivity, offset_hz)
        assert (self.L, self.M, self.P) == geometry(in_rate, selectivity)
        self.t = table(pkg, int(in_rate), int(selectivity)).astype(np.float64)
        self.step = step_of(in_rate, offset_hz) % 2 ** 64
        self.reset(0)

    def reset(self, position=0):
        self.T = int(position)
        assert 0 <= self.T <= MAX_POSITION
        self.hist = np.zeros(self.P - 1, np.complex128)          # mixed already: a sample's phase is its absolute index's

    def mix(self, x, first):
        """x[k] exp(2 pi j frac((first + k) step / 2^64)), the product modulo 2^64 in exact integers"""
        if self.step == 0:
            return x
        n = (np.uint64(first % 2 ** 64) + np.arange(x.size, dtype=np.uint64))
        with np.errstate(over="ignore"):
            acc = n * np.uint64(self.step)
        return x * np.exp(2j * np.pi * (acc.astype(np.float64) / 2.0 ** 64))

    def __call__(self, x):
        """the next samples of the stream -> the outputs they complete, complex128"""
        x = as_samples(x)
        n, L, M, P = x.size, self.L, self.M, self.P
        m0, m1 = count(L, M, P, self.T), count(L, M, P, self.T + n)
        ext = np.concatenate([self.hist, self.mix(x, self.T)])      # ext[r + P - 1] = mixed input sample T + r
        y = np.zeros(m1 - m0, np.complex128)
        if m1 > m0:
            q = np.arange(m0, m1, dtype=np.int64) * M
            i, p = q // L - self.T, q % L
            assert i[0] - (P // 2 - 1) >= -(P - 1) and i[-1] + P // 2 <= n - 1
            first = i - (P // 2 - 1) + (P - 1)                       # where tap 0 of every output lies in ext
            for j in range(P):
                y += self.t[p, j] * ext[first + j]
        self.hist = ext[ext.size - (P - 1):]
        self.T += n
        return y


def run(pkg, in_rate, selectivity, offset_hz, x, lengths=None, position=0):
    """reset at `position`, the stream x in calls of these lengths -> (the outputs joined, the counts of the calls)"""
    c = Tuner(pkg, in_rate, selectivity, offset_hz)
    c.reset(position)
    xs = as_samples(x)
    n = xs.size
    out, counts, at = [], [], 0
    for m in lengths or [n]:
        y = c(xs[at:at + m])
        out.append(y)
        counts.append(y.size)
        at += m
    assert at == n
    return np.concatenate(out), counts


def receive(stream, mode, early, bits, n_frames=2):
    """a native-rate stream -> sync_model -> extract_model -> demod_model: dict(starts, shifts, valid, bit_errors, mer_db (of
    the frames together: 10 log10(sum_signal / sum_quadrature)... as demod_model reports the sums), sync)"""
    from tests.demod_model import demod_model
    from tests.sync_model import extract_model, extract_slots, sync_model
    stream = np.asarray(stream).astype(np.complex64)               # (what the device hands on is fp32)
    r = sync_model(stream, mode, 31, n_frames)
    frames = extract_model(stream, mode, r["frames"], extract_slots(stream.size, mode, n_frames)).astype(np.complex64)
    st = [demod_model(f, mode, early, b) for f, b in zip(frames, bits)]
    sig, quad = sum(s["sum_signal"] for s in st), sum(s["sum_quadrature"] for s in st)
    return dict(starts=[f["start"] for f in r["frames"]], shifts=[f["shift"] for f in r["frames"]],
                valid=[f["valid"] for f in r["frames"]], bit_errors=[s["bit_errors"] for s in st],
                mer_db=10.0 * math.log10(sig / quad) if quad > 0 else float("inf"), sync=r)
