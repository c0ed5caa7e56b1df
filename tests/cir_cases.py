"""The signals of the channel estimator's tests, shared by tests/test_cir_cpu.py (which checks on the oracle's chains and the
float64 model that every case reads as expected, with every integer decision far from going the other way) and
tests/test_cir_gpu.py (which asserts the model's integers on the device).

Every chain is the oracle's on sync_cases.case_bits: cfg 3 = GAIN | FIR with 45 taps, gain_mode 2, normalise DC.NORMALISE,
three frames, unless the case says otherwise.  A path (d, g) is g np.roll(stream, d) in complex128 along the three frames (its
first d samples are the last d of the third frame); the signal is the sum of the case's paths plus complex Gaussian noise cn_db
below the power of the chain's data symbols, RandomState(seed).  early = CP // 2, min_rel 1e-3, min_ratio 20, Hann weights
unless stated.

Seeds, paths and levels are the issue's; none needed changing: every case met the conditions of tests/test_cir_cpu.py with
seed 5 as first written."""
import functools

import numpy as np

from tests import demod_cases as DC
from tests import sync_cases as SY
from tests.sync_model import geometry

CFG2, CFG3 = 0, DC.GAIN | DC.FIR
N_FRAMES = 3
MIN_RATIO, MIN_REL = 20.0, 1e-3
SEED = 5
S16_SCALE = 1.0 / DC.NORMALISE                      # m1_s16: the level of a chain at normalise 1.0, in front of the FormatConverter
FOUR1 = ((0, 1.0), (37, 0.5 * np.exp(1j * 1.0)), (200, 0.25), (600, 0.1j))
FOUR2 = ((0, 1.0), (11, 0.5 * np.exp(1j * 1.0)), (60, -0.25), (150, 0.1j))
LOOKAHEAD = 22                                      # FIRFilter's, in samples: what a cfg 3 chain's direct path reads as -22

# name -> dict(mode, stages, paths (None: the chain alone), cn_db, window, min_ratio, frames (slice of the three), s16, zero)
CASES = {
    "m1_clean": dict(mode=1),
    "m1_cfg2": dict(mode=1, stages=CFG2),
    "m1_cfg2_rect": dict(mode=1, stages=CFG2, window=0),
    "m1_four": dict(mode=1, paths=FOUR1, cn_db=20.0),
    "m1_four_rect": dict(mode=1, paths=FOUR1, cn_db=20.0, window=0),
    "m1_s16": dict(mode=1, paths=FOUR1, cn_db=20.0, s16=True),
    "m1_one_frame": dict(mode=1, paths=FOUR1, cn_db=20.0, frames=(0, 1), min_ratio=30.0),
    "m1_low_cn": dict(mode=1, paths=FOUR1, cn_db=5.0),
    "m1_close": dict(mode=1, paths=((0, 1.0), (6, 0.9)), cn_db=20.0),
    "m2_four": dict(mode=2, paths=FOUR2, cn_db=20.0),
    "m3_two": dict(mode=3, paths=((0, 1.0), (20, 0.5 * np.exp(1j * 1.0))), cn_db=20.0),
    "m4_two": dict(mode=4, paths=((0, 1.0), (100, 0.5 * np.exp(1j * 1.0))), cn_db=20.0),
    "m1_zero": dict(mode=1, zero=True),
}
# what each case must read as, the issue's table: the paths in descending power as (delay, level in dB below the strongest) --
# for the rectangular cases the first entries of the list, the side lobes follow -- and n_peaks
EXPECT = {
    "m1_clean": ([(-22, 0.0)], 1),
    "m1_cfg2": ([(0, 0.0)], 1),
    "m1_cfg2_rect": ([(0, 0.0), (-6, -23.1), (6, -23.1), (-10, -27.3), (10, -27.3)], 5),
    "m1_four": ([(-22, 0.0), (15, -6.02), (178, -11.98), (578, -21.61)], 4),
    "m1_four_rect": ([(-22, 0.0), (15, -6.02), (178, -11.98), (578, -21.61)], 10),
    "m1_s16": ([(-22, 0.0), (15, -6.02), (178, -11.98), (578, -21.61)], 4),
    "m1_one_frame": ([(-22, 0.0), (15, -6.02), (178, -11.98), (578, -21.61)], 4),
    "m1_low_cn": ([(-22, 0.0), (15, -6.02), (178, -11.98), (578, -21.04)], 4),
    "m1_close": ([(-22, 0.0), (-16, -0.92)], 2),
    "m2_four": ([(-22, 0.0), (-11, -6.01), (38, -12.01), (128, -21.81)], 4),
    "m3_two": ([(-22, 0.0), (-2, -6.12)], 2),
    "m4_two": ([(-22, 0.0), (78, -6.01)], 2),
    "m1_zero": ([], 0),
}
LEVEL_TOL_DB = 0.5
OUTSIDE_GUARD_M1_FOUR = 0.0052                      # the 578-sample path's share of the four paths' power
RESP_DIP_M1_CLOSE = 1.6e-3                          # resp_min / resp_mean: two paths of 1 and 0.9 cancel on some carriers


def case(name):
    c = dict(stages=CFG3, paths=None, cn_db=None, window=1, min_ratio=MIN_RATIO, frames=(0, N_FRAMES), s16=False, zero=False)
    c.update(CASES[name])
    return c


def early_of(mode):
    return geometry(mode)["CP"] // 2


@functools.lru_cache(maxsize=None)
def chain(mode, stages):
    """The oracle's chain on case_bits: (3, tf) complex64.  Computed once per process; do not write to it."""
    import oracle as O
    kw = dict(gain_mode=2, normalise=DC.NORMALISE) if stages else {}
    y = O.Chain(mode=mode, stages=stages, **kw).process(SY.case_bits(mode, N_FRAMES - 1))
    y = np.asarray(y).reshape(N_FRAMES, geometry(mode)["tf"]).astype(np.complex64)
    y.setflags(write=False)
    return y


def data_power(y, mode):
    g = geometry(mode)
    return float(np.mean(np.abs(np.asarray(y).reshape(-1, g["tf"])[:, g["null"]:].astype(np.complex128)) ** 2))


def build(name, seed=None):
    """-> (frames: (n, tf) complex64 or (n, 2 tf) int16, mode).  seed: another noise realisation of the same case."""
    c = case(name)
    mode, tf = c["mode"], geometry(c["mode"])["tf"]
    f0, f1 = c["frames"]
    if c["zero"]:
        return np.zeros((f1 - f0, tf), np.complex64), mode
    y = chain(mode, c["stages"])
    s = y.astype(np.complex128).reshape(-1)
    x = s if c["paths"] is None else sum(g * np.roll(s, d) for d, g in c["paths"])
    if c["cn_db"] is not None:
        rs = np.random.RandomState(SEED if seed is None else seed)
        sigma = np.sqrt(data_power(y, mode) / 10.0 ** (c["cn_db"] / 10.0) / 2.0)
        x = x + sigma * (rs.randn(x.size) + 1j * rs.randn(x.size))
    x = x.reshape(N_FRAMES, tf)[f0:f1]
    if c["s16"]:
        import oracle as O
        q, _ = O.format_convert((x.reshape(-1) * S16_SCALE).astype(np.complex64), "s16")
        return np.asarray(q, np.int16).reshape(f1 - f0, 2 * tf), mode
    return x.astype(np.complex64), mode


@functools.lru_cache(maxsize=None)
def named(name):
    """-> (frames, mode, early, window, min_ratio).  Computed once per process; do not write to it."""
    x, mode = build(name)
    x.setflags(write=False)
    c = case(name)
    return x, mode, early_of(mode), c["window"], c["min_ratio"]


@functools.lru_cache(maxsize=None)
def model(name):
    """The float64 model's verdict on a named case, once per process."""
    from tests.cir_model import cir_model
    x, mode, early, window, min_ratio = named(name)
    return cir_model(x, mode, early, window, min_ratio, MIN_REL)
