"""The clock of include/dabgpu.h ("the clock") in float64 numpy and Python integers, written from the header's text: the
position-exact fractional resampler as a stream (Clock) and the count of outputs (count).  The step and the rows of the tap
table are the library's own (host-only getters): what is modelled here is the arithmetic built on them."""
import functools

import numpy as np

from tests.channel_model import as_samples, to_s16  # noqa: F401  (to_s16: for the tests)

TAPS, CENTRE, PHASES, HISTORY = 32, 15, 512, 31
MAX_POSITION = 2 ** 62


def formula_taps(tau):
    """float64: sinc(m - tau) kaiser(m - tau), m = j - 15, beta 10 over +-16 samples around the sinc's peak"""
    x = np.arange(TAPS) - CENTRE - float(tau)
    u = x / 16.0
    w = np.where(np.abs(u) < 1.0, np.i0(10.0 * np.sqrt(np.clip(1.0 - u * u, 0.0, None))) / np.i0(10.0), 0.0)
    return np.sinc(x) * w


@functools.lru_cache(maxsize=None)
def table(pkg):
    """the 513 rows the library runs on, fp32; do not write to it"""
    t = np.stack([pkg.clock_phase_taps(p) for p in range(PHASES + 1)])
    assert t.dtype == np.float32 and t.shape == (PHASES + 1, TAPS)
    t.setflags(write=False)
    return t


def position(m, step):
    """output m -> (i_m, F): D = m step as an exact integer, i_m = m + floor(D / 2^64), F = the upper 32 bits of D mod 2^64"""
    d = int(m) * int(step)
    return int(m) + (d >> 64), (d & (2 ** 64 - 1)) >> 32


def count(step, T):
    """M(T): the number of m >= 0 with i_m + 16 <= T - 1, counted without the closed form: i_m does not decrease with m, so it
    is the first m whose last tap has not arrived, found by bisection on the definition"""
    T = int(T)
    if position(0, step)[0] + 16 > T - 1:
        return 0
    lo, hi = 0, 2 * T + 64                      # (i_m >= 0.999 m: m = 2 T + 64 lies behind T)
    assert position(hi, step)[0] + 16 > T - 1
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if position(mid, step)[0] + 16 <= T - 1:
            lo = mid
        else:
            hi = mid
    return hi


class Clock:
    """One stream.  pkg: the package (step and table come from its host-only functions)."""

    def __init__(self, pkg, ppm, exact_taps=False):
        self.step = pkg.clock_step(ppm)
        self.t = table(pkg).astype(np.float64)
        self.d = (table(pkg)[1:] - table(pkg)[:-1]).astype(np.float64)      # the fp32 subtraction of the definition
        self.exact_taps = exact_taps               # the formula at mu itself instead of the table's blend (CPU test 5)
        self.reset(0)

    def reset(self, position=0):
        self.T = int(position)
        assert 0 <= self.T <= MAX_POSITION
        self.hist = np.zeros(HISTORY, np.complex128)

    def __call__(self, x):
        """the next samples of the stream -> the outputs they complete, complex128"""
        x = as_samples(x)
        n = x.size
        m0, m1 = count(self.step, self.T), count(self.step, self.T + n)
        ext = np.concatenate([self.hist, x])        # ext[r + 31] = input sample T + r
        y = np.zeros(m1 - m0, np.complex128)
        if m1 > m0:
            pos = [position(m, self.step) for m in range(m0, m1)]
            i = np.array([p[0] - self.T for p in pos], np.int64)
            F = np.array([p[1] for p in pos], np.int64)
            assert i[0] - CENTRE >= -HISTORY and i[-1] + 16 <= n - 1
            p, f = F >> 23, (F & 0x7fffff).astype(np.float64) * 2.0 ** -23
            if self.exact_taps:
                h = np.stack([formula_taps(mu) for mu in F.astype(np.float64) / 2.0 ** 32])
            else:
                h = self.t[p] + f[:, None] * self.d[p]
            idx = i[:, None] + np.arange(TAPS)[None, :] - CENTRE + HISTORY
            y = (h * ext[idx]).sum(axis=1)
        self.hist = ext[ext.size - HISTORY:]
        self.T += n
        return y


def run(pkg, ppm, x, lengths=None, position=0, exact_taps=False):
    """reset at `position`, the stream x in calls of these lengths -> (the outputs joined, the counts of the calls)"""
    c = Clock(pkg, ppm, exact_taps)
    c.reset(position)
    n = x.size // 2 if np.asarray(x).dtype == np.int16 else x.size
    xs = as_samples(x)
    out, counts, at = [], [], 0
    for m in lengths or [n]:
        y = c(xs[at:at + m])
        out.append(y)
        counts.append(y.size)
        at += m
    assert at == n
    return np.concatenate(out), counts


# ---- the estimator
def sco_sums(y, mode, early=0):
    """One frame of native-rate samples -> (A_hi, A_lo, S) in float64: e = d conj(c) over the data blocks, d the receiver's
    product on the steps of tests/demod_model.py, the carriers 1 ... K/2 first in z."""
    from tests.demod_model import as_complex
    from tests.receiver import MODES
    y = as_complex(y)
    N, K, nsym, null, sym = MODES[mode]
    z = np.empty((nsym, K), np.complex128)
    for s in range(nsym):
        seg = y[null + s * sym: null + (s + 1) * sym]
        X = np.fft.fft(seg[sym - N - early: sym - early])
        z[s, :K // 2] = X[1:K // 2 + 1]
        z[s, K // 2:] = X[N - K // 2:]
    d = z[1:] * np.conj(z[:-1])
    c = ((1.0 - 2.0 * (d.real < 0)) + 1j * (1.0 - 2.0 * (d.imag < 0))) / np.sqrt(2.0)
    e = d * np.conj(c)
    return complex(e[:, :K // 2].sum()), complex(e[:, K // 2:].sum()), float(np.abs(e).sum())


def sco_figures(a_hi, a_lo, s, mode):
    """the derived figures of a set of sums -> dict(a_hi, a_lo, s, ppm, residual_cfo, quality, valid)"""
    from tests.receiver import MODES
    N, K, _, _, sym = MODES[mode]
    out = dict(a_hi=complex(a_hi), a_lo=complex(a_lo), s=float(s), ppm=0.0, residual_cfo=0.0, quality=0.0, valid=0)
    if s > 0:
        turn = 2.0 * np.pi * sym / N
        out.update(ppm=1e6 * float(np.angle(a_hi * np.conj(a_lo))) / (turn * (K // 2 + 1)),
                   residual_cfo=float(np.angle(a_hi + a_lo)) / turn, quality=abs(a_hi + a_lo) / s, valid=1)
    return out


def sco_model(frames, mode, early=0):
    """whole frames (n, tf) -> (the figures of every frame, the figures from the sums over all valid frames)"""
    per = [sco_figures(*sco_sums(f, mode, early), mode) for f in frames]
    valid = [p for p in per if p["valid"]]
    total = sco_figures(sum(p["a_hi"] for p in valid), sum(p["a_lo"] for p in valid), sum(p["s"] for p in valid), mode)
    return per, total


def loop_model(pkg, x, mode, ppm, early, bits, channel=None):
    """The loop of the tests on the models: [channel ->] clock(+ppm) -> sync -> extract -> sco; then clock(inverse of the
    estimate) on the capture -> sync -> extract -> demod and sco.  -> dict(first, second: per pass starts, shifts, bit_errors,
    ratio (sum_quadrature / sum_signal over the frames), estimate)"""
    from tests.demod_model import demod_model
    from tests.sync_model import extract_model, extract_slots, sync_model
    if channel is not None:
        x = channel(x)
    out, capture = {}, run(pkg, ppm, np.asarray(x).astype(np.complex64))[0]
    stream, name = capture, "first"
    for _ in range(2):
        stream = stream.astype(np.complex64)            # (what the device hands on is fp32)
        r = sync_model(stream, mode, 31, 2)
        frames = extract_model(stream, mode, r["frames"], extract_slots(stream.size, mode, 2)).astype(np.complex64)
        st = [demod_model(f, mode, early, b) for f, b in zip(frames, bits)]
        out[name] = dict(starts=[f["start"] for f in r["frames"]], shifts=[f["shift"] for f in r["frames"]],
                         valid=[f["valid"] for f in r["frames"]], bit_errors=[s["bit_errors"] for s in st],
                         ratio=sum(s["sum_quadrature"] for s in st) / sum(s["sum_signal"] for s in st),
                         estimate=sco_model(frames, mode, early)[1]["ppm"], sync=r)
        if name == "first":
            stream, name = run(pkg, pkg.clock_inverse_ppm(out["first"]["estimate"]), capture.astype(np.complex64))[0], "second"
    return out
