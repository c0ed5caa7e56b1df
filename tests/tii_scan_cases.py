"""The signals of the TII analyser's tests, shared by tests/test_tii_scan_cpu.py (which checks on the oracle's chains and the
float64 model that every case reads as expected, with every integer decision far from going the other way) and
tests/test_tii_scan_gpu.py (which asserts the model's integers on the device).

Every chain is the oracle's on sync_cases.case_bits: cfg 3 = GAIN | FIR with 45 taps, gain_mode 2, normalise DC.NORMALISE,
five frames (frames 0, 2 and 4 carry TII), unless the case says otherwise.  A "two" case is A (comb 3, pattern 5) +
0.5 e^{j 1.0} B (comb 7, pattern 5) on the same bits, B delayed by d whole samples along the stream (its first d samples are the
last d of the fifth frame: the stream is rolled), plus complex Gaussian noise cn_db below the power of A's data symbols, RandomState(seed).

Seeds and levels are the issue's; none needed changing: every case met the conditions of tests/test_tii_scan_cpu.py as first
written (seeds 6 and 7 were tried beside 5 on the two "two" cases and qualify as well)."""
import functools

import numpy as np

from tests import demod_cases as DC
from tests import sync_cases as SY
from tests.sync_model import geometry

CFG2, CFG3 = 0, DC.GAIN | DC.FIR
EARLY = {1: 252, 2: 63}
MIN_RATIO, MIN_REL = 12.0, 1e-3
A, B = (3, 5), (7, 5)                               # (comb, pattern) of the two transmitters
B_GAIN = 0.5 * np.exp(1j * 1.0)
S16_SCALE = 1.0 / DC.NORMALISE                      # m1_s16: the level of a chain at normalise 1.0, in front of the FormatConverter

# name -> dict(mode, stages, tii (of A; None: off), old, d (None: A alone), cn_db, seed, frames (slice of the five), s16)
CASES = {
    "m1_single": dict(mode=1),
    "m1_old": dict(mode=1, old=True),
    "m1_odd": dict(mode=1, frames=(1, 5)),
    "m1_two": dict(mode=1, d=37, cn_db=20.0, seed=5),
    "m1_s16": dict(mode=1, d=37, cn_db=20.0, seed=5, s16=True),
    "m1_none": dict(mode=1, tii=None, cn_db=20.0, seed=5, frames=(0, 4)),
    "m1_zero": dict(mode=1, stages=CFG2, tii=None),
    "m2_single": dict(mode=2),
    "m2_two": dict(mode=2, d=11, cn_db=30.0, seed=5),
}
# what each case must read as: [(comb, pattern by the standard, delay in samples)], and the parity where it is asserted
EXPECT = {
    "m1_single": ([(3, 5, -22.0)], 0),
    "m1_old": ([(3, 5, -22.0)], 0),
    "m1_odd": ([(3, 5, -22.0)], 1),
    "m1_two": ([(3, 5, -22.0), (7, 5, 15.0)], 0),
    "m1_s16": ([(3, 5, -22.0), (7, 5, 15.0)], 0),
    "m1_none": ([], None),
    "m1_zero": ([], None),
    "m2_single": ([(3, 32, -22.0)], 0),
    "m2_two": ([(3, 32, -22.0), (7, 32, -11.0)], 0),
}
TWO_CASES = ("m1_two", "m1_s16", "m2_two")
LEVEL_DB, LEVEL_TOL_DB = 6.02, 0.5                  # A over B: 20 log10(1 / 0.5)


def case(name):
    c = dict(stages=CFG3, tii=A, old=False, d=None, cn_db=None, seed=None, frames=(0, 5), s16=False)
    c.update(CASES[name])
    return c


def chain(mode, stages, tii, old, n_frames=5):
    """The oracle's chain on case_bits: (n_frames, tf) complex64."""
    import oracle as O
    kw = dict(gain_mode=2, normalise=DC.NORMALISE) if stages else {}
    if tii is not None:
        kw["tii"] = (tii[0], tii[1], bool(old))
    y = O.Chain(mode=mode, stages=stages, **kw).process(SY.case_bits(mode, n_frames - 1))
    return np.asarray(y).reshape(n_frames, geometry(mode)["tf"]).astype(np.complex64)


def data_power(y, mode):
    g = geometry(mode)
    return float(np.mean(np.abs(np.asarray(y).reshape(-1, g["tf"])[:, g["null"]:].astype(np.complex128)) ** 2))


def build(name, seed=None, cn_db=None):
    """-> (frames: (n, tf) complex64 or (n, 2 tf) int16, mode).  seed / cn_db: another operating point of the same case."""
    c = case(name)
    mode, tf = c["mode"], geometry(c["mode"])["tf"]
    ya = chain(mode, c["stages"], c["tii"], c["old"])
    x = ya.astype(np.complex128).reshape(-1)
    if c["d"] is not None:
        yb = chain(mode, c["stages"], B, c["old"]).astype(np.complex128).reshape(-1)
        x = x + B_GAIN * np.roll(yb, c["d"])
    cn_db = c["cn_db"] if cn_db is None else cn_db
    if cn_db is not None:
        rs = np.random.RandomState(c["seed"] if seed is None else seed)
        sigma = np.sqrt(data_power(ya, mode) / 10.0 ** (cn_db / 10.0) / 2.0)
        x = x + sigma * (rs.randn(x.size) + 1j * rs.randn(x.size))
    f0, f1 = c["frames"]
    x = x.reshape(5, tf)[f0:f1]
    if c["s16"]:
        import oracle as O
        q, _ = O.format_convert((x.reshape(-1) * S16_SCALE).astype(np.complex64), "s16")
        return np.asarray(q, np.int16).reshape(f1 - f0, 2 * tf), mode
    return x.astype(np.complex64), mode


@functools.lru_cache(maxsize=None)
def named(name):
    """-> (frames, mode, early, old_variant).  Computed once per process; do not write to it."""
    x, mode = build(name)
    x.setflags(write=False)
    return x, mode, EARLY[mode], case(name)["old"]


@functools.lru_cache(maxsize=None)
def model(name):
    """The float64 model's verdict on a named case, once per process."""
    from tests.tii_scan_model import tii_scan_model
    x, mode, early, old = named(name)
    return tii_scan_model(x, mode, early, old, MIN_RATIO, MIN_REL)
