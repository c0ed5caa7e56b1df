"""Inputs shared by tests/test_csi_cpu.py and tests/test_csi_gpu.py: the operating point of "weighted beats unweighted" behind a
narrowband interferer, the white-noise levels of the two soft paths, and the small frames of the kernel tests."""
import numpy as np

from tests import channel_cases as CC
from tests import channel_model as CM
from tests import csi_model as X
from tests import soft_cases as SC
from tests.receiver import MODES

# ---- the operating point.  The signal is tests/soft_cases.py's (Mode II, 18 frames, FIC + one 24-CU sub-channel at 3-A, cfg 3,
# early 44) with the channel's own white noise (tests/channel_model.py, seed channel_cases.OP_SEED) 3 dB above soft_cases'
# level, plus a comb of unmodulated tones over the whole stream (csi_model.tone_comb): tone j sits comb_bins(n)[j] carrier
# spacings above the centre frequency -- never on a carrier.  The carrier-to-interference ratio (data power, as
# channel_cases.data_power takes it, over the comb's total power) goes down in 1 dB steps; L = the highest C/I at which the
# unweighted soft path has a payload bit error in every returned frame.  The comb qualifies when the weighted path has none at
# L - 2, L - 1, L, L + 1 and L + 2 dB.  Found by tests/test_csi_cpu.py's search on the numpy models (recorded in
# profiles/csi.txt): one tone qualifies, so no other comb was tried.
OP_CN_DB = SC.OP_LEVEL_DB + 3.0
OP_CI_START_DB, OP_CI_STOP_DB = 12, -10
OP_COMBS_TRIED = (1,)
OP_TONES, OP_CI_DB = 1, 7
OP_MARGIN_DB = 2

# ---- white noise alone (the same signal, the channel model's noise, seed channel_cases.OP_SEED), C/N downwards from
# WN_START_DB in 0.25 dB steps: the last level before the first one at which a path has a payload bit error in a returned
# frame.  Measured on the models, not chosen (profiles/csi.txt).
WN_START_DB, WN_STEP_DB, WN_STOP_DB = 6.0, 0.25, 2.0
WN_WEIGHTED_DB, WN_UNWEIGHTED_DB = 4.0, 4.0


def comb_bins(n):
    return [40.37 + 9.31 * j for j in range(n)]


def op_input(y, power, cn_db, n_tones=None, ci_db=None, sigma_of=None):
    """(frames, tf_samples) clean IQ -> the same behind the channel model's noise at cn_db and, with n_tones, the comb at ci_db"""
    ch = CM.Channel([(0, 1.0, 0.0)], sigma_of(power, cn_db), CC.OP_SEED)
    yn = ch(np.asarray(y).reshape(-1)).reshape(np.asarray(y).shape)
    if n_tones:
        yn = yn + op_tones(yn.shape, power, n_tones, ci_db)
    return yn


def op_tones(shape, power, n_tones, ci_db):
    """the comb as (frames, tf_samples) complex128"""
    return X.tone_comb(int(np.prod(shape)), SC.OP_MODE, comb_bins(n_tones), power / 10.0 ** (ci_db / 10.0)).reshape(shape)


# ---- the kernel tests' frames: a random QPSK frame built in the frequency domain (no chain needed), noise, and interferers
def random_frame(mode, seed, cn_db=12.0, spur_positions=(), spur_db=10.0):
    """One transmission frame of `mode` as complex128: null symbol of zeros, differentially coded random QPSK on the K
    carriers, cyclic prefix; white noise cn_db below the data symbols; on every carrier position in spur_positions an
    unmodulated carrier spur_db above one data carrier, exactly on the carrier's frequency."""
    N, K, nsym, null, sym = MODES[mode]
    rs = np.random.RandomState(seed)
    bins = np.concatenate([np.arange(1, K // 2 + 1), np.arange(N - K // 2, N)])
    z = np.empty((nsym, K), np.complex128)
    z[0] = np.exp(0.5j * np.pi * rs.randint(0, 4, K))
    for s in range(1, nsym):
        z[s] = z[s - 1] * np.exp(0.5j * np.pi * rs.randint(0, 4, K) + 0.25j * np.pi)
    frame = np.zeros(null + nsym * sym, np.complex128)
    n = np.arange(null, null + nsym * sym, dtype=np.float64)
    for s in range(nsym):
        X_ = np.zeros(N, np.complex128)
        X_[bins] = z[s]
        x = np.fft.ifft(X_) * N / np.sqrt(K)                      # unit power per sample
        frame[null + s * sym: null + (s + 1) * sym] = np.concatenate([x[N - (sym - N):], x])
    for k in spur_positions:
        amp = np.sqrt(10.0 ** (spur_db / 10.0) / K)
        frame[null:] += amp * np.exp(2j * np.pi * bins[k] / N * n)
    sigma = np.sqrt(10.0 ** (-cn_db / 10.0) / 2.0)
    frame += sigma * (rs.standard_normal(frame.size) + 1j * rs.standard_normal(frame.size))
    return frame
