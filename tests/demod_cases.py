"""The inputs of the receiver's tests, shared by tests/test_demod_cpu.py (which checks on the oracle's chains that every one of
them decodes with a comfortable margin) and tests/test_demod_gpu.py (which asserts exact bits on the device)."""
import numpy as np

from tests.golden.synth import synth_eti

GAIN, FIR = 1, 2
NORMALISE = 1.0 / 50000.0
CP = {1: 504, 2: 126, 3: 63, 4: 252}              # cyclic prefix of the data symbols: sym_size - spacing
CFR = (50.0, 0.1)                                  # clip, error clip: the suite's usual crest-factor reduction
TII = (3, 5, False)                                # comb, pattern, old variant
WINDOW = 10
MARGIN_FLOOR = 1e-3                                # four orders above the fp32 transform's 1.1e-7


def case_bits(mode, n_frames, per):
    """n_frames of seeded coded bits for a mode; the first three frames of the five-frame batch are the three-frame batch."""
    rs = np.random.RandomState(700 + mode)
    return np.frombuffer(rs.bytes(5 * per), np.uint8).reshape(5, per)[:n_frames].copy()


def eti_frames(n_tf, mode=1):
    """ETI frames of n_tf transmission frames: the suite's synthetic multiplex (one 128 kbit/s sub-channel, EEP 3-A)."""
    cifs = {1: 4, 2: 1, 3: 1, 4: 2}[mode]
    return synth_eti(n_tf * cifs, mid=mode & 3)


# The monitor's cases, Mode I, five frames: name -> (stages, oracle keywords, automatic early, output format).
# early: (45 - 1 with FIRFilter in the mask) + (the window overlap).
MONITOR_CASES = {
    "cfg2": (0, {}, 0, None),
    "cfg3": (GAIN | FIR, dict(gain_mode=2, normalise=NORMALISE), 44, None),
    "window10": (GAIN | FIR, dict(gain_mode=2, normalise=NORMALISE, window_overlap=WINDOW), 54, None),
    "cfr": (GAIN | FIR, dict(gain_mode=2, normalise=NORMALISE, cfr=CFR), 44, None),
    "tii": (GAIN | FIR, dict(gain_mode=2, normalise=NORMALISE, tii=TII), 44, None),
    "s16": (GAIN | FIR, dict(gain_mode=2, normalise=1.0), 44, "s16"),
}


def configure(pkg, md, name):
    """The device context's settings for a monitor case."""
    stages, kw, _, fmt = MONITOR_CASES[name]
    if "gain_mode" in kw:
        md.set_gain(kw["gain_mode"], 1.0, kw["normalise"], 4.0)
    if "window_overlap" in kw:
        md.set_window_overlap(kw["window_overlap"])
    if "cfr" in kw:
        md.set_cfr(True, *kw["cfr"])
    if "tii" in kw:
        md.set_tii(True, kw["tii"][0], kw["tii"][1], kw["tii"][2])
    if fmt:
        md.set_output_format(fmt)
    return stages
