"""Crest-factor reduction in float64: clip -> FFT -> error clip -> IFFT (src/OfdmGenerator.cpp:222-277, :310-373), complex128
throughout (numpy's pocketfft), with every decision it takes and the decisions that two correct fp32 implementations may take
differently.

The ambiguity sets come from bars the project already holds, not from anything measured on the code under test:
  TAU_CLIP = 2e-5          the max-abs bar tests/test_gpu_parity.py::test_ofdm_generator_vs_float64_dft asserts for the transform
                           in all four modes: |t| of a correct fp32 transform lies that close to the float64 one;
  TAU_ERR  = TAU_CLIP+1e-6 the clipped symbol differs by at most TAU_CLIP per sample, so its bins / N by at most TAU_CLIP; the
                           forward transform adds the project's 1e-6 relative bar on bins of order 1.
A sample (bin) of a live symbol whose magnitude lies within tau of the threshold may be decided either way; every other decision
is the model's.  A live symbol is one whose carriers are not all exactly zero: a blank one stays exactly zero on both sides and
is never ambiguous."""
import types

import numpy as np

TAU_CLIP = 2e-5
TAU_ERR = TAU_CLIP + 1e-6
AMBIGUITY_CAP = 1e-3          # of a frame's decisions: half of the 0.2 % tests/test_gpu_parity.py::_check_cfr_stats allows


def bins_of(z, nsym, K, N):
    """The carriers of nsym symbols in their FFT bins (src/OfdmGenerator.cpp:222-226), complex128."""
    zs = np.asarray(z).reshape(nsym, K).astype(np.complex128)
    X = np.zeros((nsym, N), np.complex128)
    X[:, 1:K // 2 + 1] = zs[:, :K // 2]
    X[:, N - K // 2:] = zs[:, K // 2:]
    return X


def cfr_model(z, nsym, K, N, clip, error_clip):
    """Per symbol: t (the IFFT output), mag = |t|, clipped (the clip decisions), emag = |e| per bin, eclipped (the error-clip
    decisions), y (the output), papr_before / papr_after = (peak, mean) of |t|^2 / |y|^2, mer_iq / mer_delta (the MER sums, had
    the symbol been the frame's MER symbol), live; and the ambiguity sets amb_clip / amb_err (boolean, nsym x N).  The
    thresholds act through their squares (:315, :339): a negative one is its magnitude."""
    clip, eclip = abs(float(np.float32(clip))), abs(float(np.float32(error_clip)))
    X = bins_of(z, nsym, K, N)
    live = np.any(X != 0, axis=1)
    t = np.fft.ifft(X, axis=1) * N
    mag = np.abs(t)
    clipped = mag > clip
    tc = np.where(clipped, t * (clip / np.where(clipped, mag, 1.0)), t)
    c = np.fft.fft(tc, axis=1) / N
    e = X - c
    emag = np.abs(e)
    eclipped = emag > eclip
    e = np.where(eclipped, e * (eclip / np.where(eclipped, emag, 1.0)), e)
    y = np.fft.ifft(c + e, axis=1) * N
    p_t, p_y = mag ** 2, np.abs(y) ** 2
    m = types.SimpleNamespace(
        t=t, mag=mag, clipped=clipped, emag=emag, eclipped=eclipped, y=y, live=live,
        papr_before=np.stack([p_t.max(axis=1), p_t.mean(axis=1)], axis=1),
        papr_after=np.stack([p_y.max(axis=1), p_y.mean(axis=1)], axis=1),
        mer_iq=p_t.sum(axis=1), mer_delta=(np.abs(y - t) ** 2).sum(axis=1),
        amb_clip=live[:, None] & (np.abs(mag - clip) <= TAU_CLIP),
        amb_err=live[:, None] & (np.abs(emag - eclip) <= TAU_ERR))
    m.num_clip, m.num_error_clip = int(clipped.sum()), int(eclipped.sum())
    m.n_amb_clip, m.n_amb_err = int(m.amb_clip.sum()), int(m.amb_err.sum())
    m.num_samples = nsym * N
    return m
