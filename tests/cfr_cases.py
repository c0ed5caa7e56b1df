"""Crest-factor reduction across its clip / error-clip range: the regimes, the forms of the frame kernel that run it, their
inputs, and the oracle of a form (the reference's stages one after the other, as oracle.Chain runs them -- with the MER symbol
index a free argument and carriers as well as coded bits for input).  Shared by tests/test_cfr_cpu.py and tests/test_cfr_gpu.py.

Regimes are (clip, error_clip) with base = float32(50 sqrt(K / 1536)); tests/test_cfr_cpu.py asserts on the float64 model that
each is what its name says."""
import functools

import numpy as np

import oracle as O
from tests.cfr_model import cfr_model
from tests.golden.synth import synth_bits, synth_signal

FRAMES = 2


def base_clip(K):
    return float(np.float32(50.0 * np.sqrt(K / 1536.0)))


REGIMES = {
    "base": lambda b: (b, 0.1),                  # the one point every other CFR test runs at
    "off_high": lambda b: (1e9, 0.1),            # nothing clips, no error clips
    "clip_only": lambda b: (b, 1e9),             # no error clips: CFR undoes itself
    "all_clip": lambda b: (0.01 * b, 0.1),       # (nearly) every sample clipped; in-band bins all error-clipped, out-of-band none
    "err_zero": lambda b: (b, 0.0),              # every bin of every live symbol error-clipped
    "heavy": lambda b: (0.5 * b, 0.02),
    "light": lambda b: (1.6 * b, 0.5),           # a few samples clipped, no error clipped
    "clip_zero": lambda b: (0.0, 0.1),           # every non-zero sample clipped to 0
    "negative": lambda b: (-b, -0.1),            # the reference squares the thresholds: `base` again
}
NO_ERROR_CLIP = ("off_high", "clip_only", "light")          # the model clips no error bin: MER by its sums, not in dB


def thresholds(regime, K):
    clip, eclip = REGIMES[regime](base_clip(K))
    return float(np.float32(clip)), float(np.float32(eclip))


# ---- inputs: two frames per (mode, kind)
def bits_of(mode):
    return np.stack([synth_bits(O.tf_input_bytes(mode), seed=2300 + 10 * mode + f) for f in range(FRAMES)])


def carriers_of_bits(mode, bits):
    K = O.mode_params(mode)["carriers"]
    pr, _ = O.phase_reference(mode)
    return np.stack([O.signal_mux(np.zeros(K, np.complex64), O.diff_mod(pr, O.freq_interleave(O.qpsk_map(b, K), mode), K))
                     for b in bits])


@functools.lru_cache(maxsize=None)
def carriers(mode, kind):
    """kind "bits": the SignalMultiplexer output of bits_of(mode), blank null symbol; "signal": arbitrary carriers of about unit
    power, energy in symbol 0 as well."""
    m = O.mode_params(mode)
    if kind == "bits":
        z = carriers_of_bits(mode, bits_of(mode))
    else:
        n = (m["nb_symbols"] + 1) * m["carriers"]
        z = np.stack([synth_signal(n, seed=2400 + 10 * mode + f) * np.float32(1 / 40) for f in range(FRAMES)])
    z.setflags(write=False)
    return z


INPUTS = [(1, "bits"), (2, "bits"), (3, "bits"), (4, "bits"), (2, "signal")]


def geometry(mode):
    m = O.mode_params(mode)
    return m["carriers"], m["spacing"], m["nb_symbols"] + 1


@functools.lru_cache(maxsize=4)
def models(mode, kind, regime):
    K, N, nsym = geometry(mode)
    clip, eclip = thresholds(regime, K)
    return [cfr_model(z, nsym, K, N, clip, eclip) for z in carriers(mode, kind)]


# ---- forms: every cfr=1 variant the dispatch has
class Form:
    def __init__(self, name, mode, entry, gain=False, fir=None, overlap=0, fmt=None, chunks=1, kind="bits"):
        self.name, self.mode, self.entry, self.gain, self.fir = name, mode, entry, gain, fir
        self.overlap, self.fmt, self.chunks, self.kind = overlap, fmt, chunks, kind
        self.normalise = 32767.0 / 50000.0 if fmt else 1.0 / 50000.0
        self.guard = entry != "ofdm"

    @property
    def stages(self):
        return (O.STAGE_GAIN if self.gain else 0) | (O.STAGE_FIR if self.fir else 0)

    def __repr__(self):
        return self.name


def taps_of(n):
    """The default 45 taps, or the dispatch matrix's low-pass at 0.79 of Nyquist with n taps."""
    if n is None or n == 45:
        return O.fir_default_taps()
    k = np.arange(n) - (n - 1) / 2.0
    h = 0.79 * np.sinc(0.79 * k) * np.hamming(n)
    return (h / h.sum()).astype(np.float32)


FORMS = (
    [Form("ofdm-m%d" % m, m, "ofdm") for m in (1, 2, 3, 4)] +                                   # bits=0, no epilogue
    [Form("bits_guard-m%d-g%d" % (m, g), m, "chain", gain=bool(g)) for m in (1, 3) for g in (0, 1)] +   # Mode I: CFR_LEAN
    [Form("bits_fir45-m%d" % m, m, "chain", gain=True, fir=45) for m in (1, 2)] +               # Mode I: CFR_SEQ
    [Form("bits_fir101-m1", 1, "chain", gain=True, fir=101)] +                                  # the generic packed pair, hk8
    [Form("windowed-m1-f%d" % bool(t), 1, "chain", gain=True, fir=t, overlap=10) for t in (None, 45)] +
    [Form("s16-m1-f%d" % bool(t), 1, "chain", gain=True, fir=t, fmt="s16") for t in (None, 45)] +
    [Form("symbols-m2", 2, "symbols", gain=True, fir=45, kind="signal")] +
    [Form("bits_fir45-m1-chunks7", 1, "chain", gain=True, fir=45, chunks=7),
     Form("bits_guard-m1-g1-chunks7", 1, "chain", gain=True, chunks=7)])


def segments(form):
    """[(start, stop)] of every symbol in a frame of the form's output stream."""
    m = O.mode_params(form.mode)
    N, nsym = m["spacing"], m["nb_symbols"] + 1
    if not form.guard:
        return [(s * N, (s + 1) * N) for s in range(nsym)]
    ns, ss = m["null_size"], m["sym_size"]
    return [(0, ns)] + [(ns + (s - 1) * ss, ns + s * ss) for s in range(1, nsym)]


def oracle_frame(form, z, cfr, mer_index=0):
    """One frame of the form from carriers z: (complexf samples, CFR statistics, papr[nsym][4]); cfr = (clip, error_clip) or
    None for the chain without crest-factor reduction (statistics None)."""
    m = O.mode_params(form.mode)
    K, N, nsym = geometry(form.mode)
    st = papr = None
    if cfr is None:
        x = O.ofdm_generate(z, nsym, K, N)
    else:
        x, st, papr = O.ofdm_generate_cfr(z, nsym, K, N, cfr[0], cfr[1], mer_index)
    if form.gain:
        x = O.gain_control(x, N, O.GAIN_VAR, 1.0, form.normalise, 4.0)
    if form.guard:
        x = O.guard_interval(x, m["nb_symbols"], N, m["null_size"], m["sym_size"], form.overlap)
    if form.fir:
        x = O.fir_filter(x, taps_of(form.fir))
    return x, st, papr


def mer_indices(form, call):
    """The MER symbol of each frame of the call-th run (0, 1, ...) of a fresh context: the index advances once per frame."""
    nsym = geometry(form.mode)[2]
    return [(call * FRAMES + f + 1) % nsym for f in range(FRAMES)]
