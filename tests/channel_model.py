"""Float64 numpy model of the channel emulator, written from the text of include/dabgpu.h ("the channel") alone: Philox4x32-10
in uint64 arithmetic, the cut-off Gaussian, the paths with their integer Doppler phase, the history of 2047 samples."""
import numpy as np

MAX_PATHS, MAX_DELAY = 64, 2047
M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)


def philox4x32_10(counter, key):
    """counter: four arrays (or scalars) of 32-bit words, key: two words -> four uint64 arrays holding 32-bit words"""
    x = [np.atleast_1d(np.asarray(c, np.uint64)) & MASK32 for c in counter]
    x = list(np.broadcast_arrays(*x))
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = M0 * x[0], M1 * x[2]                     # 32 x 32 -> 64 bits: no overflow in uint64
        x = [(p1 >> S32) ^ x[1] ^ np.uint64(k0), p1 & MASK32, (p0 >> S32) ^ x[3] ^ np.uint64(k1), p0 & MASK32]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return x


def absolute_index(position, n):
    """a = position + i mod 2^64, uint64"""
    return np.uint64(int(position) & (2 ** 64 - 1)) + np.arange(n, dtype=np.uint64)


def unit_noise(seed, position, n):
    """n_re + j n_im for the samples position ... position + n - 1: complex128, unit variance per component"""
    a = absolute_index(position, n)
    c = a >> np.uint64(1)
    w = philox4x32_10((c & MASK32, c >> S32, 0, 0), (int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF))
    odd = (a & np.uint64(1)) != 0
    wa, wb = np.where(odd, w[2], w[0]), np.where(odd, w[3], w[1])
    u = ((wa >> np.uint64(9)).astype(np.float64) + 0.5) * 2.0 ** -23
    r = np.sqrt(-2.0 * np.log(u))
    ang = 2.0 * np.pi * wb.astype(np.float64) / 2.0 ** 32
    return r * np.cos(ang) + 1j * r * np.sin(ang)


def doppler_step(doppler_hz, rate_hz):
    """rint(doppler_hz / rate_hz 2^64) as a two's-complement 64-bit integer (a Python int in 0 ... 2^64 - 1)"""
    return int(np.rint(np.float64(doppler_hz) / np.float64(rate_hz) * 2.0 ** 64)) & (2 ** 64 - 1)


def theta(position, n, step):
    """the upper 32 bits of a step mod 2^64, over 2^32"""
    a = absolute_index(position, n)
    return ((a * np.uint64(step)) >> S32).astype(np.float64) / 2.0 ** 32


def as_samples(x):
    """complex input, or int16 interleaved (re, im) -> complex128"""
    x = np.asarray(x)
    if x.dtype == np.int16:
        v = x.reshape(-1, 2).astype(np.float64)
        return v[:, 0] + 1j * v[:, 1]
    return x.astype(np.complex128).reshape(-1)


class Channel:
    """One stream: paths are (delay, gain, doppler_hz); gains and sigma are taken at fp32 precision, as the interface does."""

    def __init__(self, paths, sigma=0.0, seed=0, rate_hz=2048000.0):
        self.set(paths, sigma, seed, rate_hz)
        self.reset(0)

    def set(self, paths, sigma=0.0, seed=0, rate_hz=2048000.0):
        paths = list(paths)
        assert len(paths) <= MAX_PATHS and all(0 <= d <= MAX_DELAY for d, _, _ in paths)
        self.paths = [(int(d), complex(np.complex64(g)), doppler_step(f, rate_hz)) for d, g, f in paths]
        self.sigma, self.seed = float(np.float32(sigma)), int(seed)

    def reset(self, position=0):
        self.position = int(position) & (2 ** 64 - 1)
        self.hist = np.zeros(MAX_DELAY, np.complex128)

    def __call__(self, x):
        x = as_samples(x)
        n = x.size
        ext = np.concatenate([self.hist, x])
        y = np.zeros(n, np.complex128)
        for d, g, step in self.paths:
            seg = ext[MAX_DELAY - d:MAX_DELAY - d + n]
            if step == 0:
                y += g * seg
            else:
                y += g * np.exp(2j * np.pi * theta(self.position, n, step)) * seg
        if self.sigma > 0.0:
            y += self.sigma * unit_noise(self.seed, self.position, n)
        self.hist = ext[ext.size - MAX_DELAY:]
        self.position = (self.position + n) & (2 ** 64 - 1)
        return y


def to_s16(y):
    """dabgpu_format_process's s16 conversion of complex samples: saturating, toward zero -> int16 interleaved"""
    v = np.stack([y.real, y.imag], axis=1).reshape(-1)
    return np.clip(np.trunc(v), -32768, 32767).astype(np.int16)
