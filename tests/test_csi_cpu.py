"""The carrier state without a device (include/dabgpu.h, "the carrier state"): the interface is declared and
exported, the model's weights are finite and inside [0, MAX] on the degenerate inputs, and -- on the numpy models alone -- the
operating point behind a narrowband interferer at which the weighted soft path decodes what the unweighted one loses, and what
the weighting costs on white noise.  The searches fix the inputs of tests/test_csi_gpu.py."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import channel_cases as CC
from tests import csi_cases as XC
from tests import csi_model as X
from tests import soft_cases as SC
from tests import soft_model as S
from tests.conftest import ROOT, load_pkg
from tests.receiver import MODES

ENTRIES = ["dabgpu_demod_csi", "dabgpu_demod_csi_dev", "dabgpu_demod_carrier_state", "dabgpu_demod_carrier_state_dev",
           "dabgpu_get_carrier_state", "dabgpu_debug_csi_unit_weights"]


# --------------------------------------------------------------------------- 1. the interface
def test_header_library_and_exports_are_in_step():
    pkg = load_pkg()
    header = open(os.path.join(ROOT, "include", "dabgpu.h")).read()
    lib = ctypes.CDLL(os.path.join(ROOT, "odr-dabmod_amd", "csrc", "libdabgpu.so"))
    for name in ENTRIES:
        assert re.search(r"DABGPU_API int %s\(" % name, header), name
        assert name in pkg.EXPORTS and hasattr(lib, name), name
    for method in ("demod_csi", "demod_csi_dev", "demod_carrier_state", "demod_carrier_state_dev", "carrier_state"):
        assert callable(getattr(pkg.Modulator, method))
    assert X.header_constants(header) == (X.FRAC_BITS, int(X.MAX_WEIGHT), X.TRIM_PASSES, X.TRIM_FACTOR)
    assert (pkg.CSI_FRAC_BITS, pkg.CSI_MAX_WEIGHT) == (X.FRAC_BITS, int(X.MAX_WEIGHT))


# --------------------------------------------------------------------------- 2. degenerate inputs
def _inside(w):
    return w.dtype == np.float32 and np.isfinite(w).all() and (w >= 0).all() and (w <= X.MAX_WEIGHT).all()


def test_weights_of_degenerate_frames_are_finite_and_inside_the_range():
    mode = 3
    N, K, nsym, null, sym = MODES[mode]
    # all-zero frames: q = 0, every sum 0, w = 1, softs 0
    m = X.demod_csi_model(np.zeros(null + nsym * sym, np.complex64), mode)
    assert not m["A"].any() and not m["V"].any() and (m["w"] == 1).all() and not m["soft"].any()
    # a clean frame (no noise at all): V rounds to 0 on every carrier or on most; whatever is left, the weights are inside
    clean = XC.random_frame(mode, 1, cn_db=400.0)
    m = X.demod_csi_model(clean, mode)
    assert m["V"].max() <= 1 and _inside(m["w"]) and (np.abs(m["soft"]) == 64).all()
    # one carrier nulled in a noisy frame: its A is small, its weight near 0, the others' near 1
    noisy = XC.random_frame(mode, 2, cn_db=15.0)
    u = X.scaled_d(noisy, mode)
    u[:, 17] *= 0.0
    A, V = X.sums(u)
    w = X.weights(A, V)
    assert A[17] == 0 and V[17] == 0 and w[17] == 0 and _inside(w)
    assert 0.4 < np.delete(w, 17).min() and np.delete(w, 17).max() < 2.5 and abs(np.delete(w, 17).mean() - 1) < 0.1
    # one carrier with V_k = 0 and signal: the floor holds it at the maximum
    A, V = X.sums(X.scaled_d(noisy, mode))
    V[40] = 0
    w = X.weights(A, V)
    assert w[40] == X.MAX_WEIGHT and _inside(w)
    # a carrier far above the rest is left out of the means: the others keep their weights
    A, V = X.sums(X.scaled_d(noisy, mode))
    w0 = X.weights(A, V)
    A[5], V[5] = 40 * A[5], 1600 * V[5]
    w1 = X.weights(A, V)
    assert w1[5] < 0.05 and np.abs(np.delete(w1, 5) / np.delete(w0, 5) - 1).max() < 0.02


def test_model_mer_per_carrier_follows_the_noise():
    """20 log10(A_k / sqrt(2^(F - 1) S V_k)) on white noise 15 dB below the samples' power, Mode III.  Expected: the carriers hold
    the power of N bins in K, so a carrier lies 15 + 10 log10(N / K) = 16.25 dB above the noise of its bin; d = z_s conj(z_(s-1))
    carries the noise of two symbols, of which the part at right angles to the decision is half: 16.25 dB again.  V_k is a sum
    of S = 152 squares, relative scatter sqrt(2 / 152) = 0.115 (0.5 dB); four of those, over 192 carriers, are the bounds."""
    m = X.demod_csi_model(XC.random_frame(3, 2, cn_db=15.0), 3)
    mer = X.mer_db(m["A"], m["V"], 3)
    print("per-carrier MER: median %.2f dB, %.2f ... %.2f dB" % (np.median(mer), mer.min(), mer.max()))
    want = 15.0 + 10.0 * np.log10(256 / 192)
    assert abs(np.median(mer) - want) < 0.3
    assert mer.min() > want + 10 * np.log10(1 / (1 + 4 * 0.115)) - 0.3 and mer.max() < want + 10 * np.log10(1 / (1 - 4 * 0.115)) + 0.3


# --------------------------------------------------------------------------- 3. the operating point behind an interferer
@pytest.fixture(scope="module")
def op():
    import oracle as O
    from tests import decode_model as M
    pkg = load_pkg()
    eti, bits, ref = SC.op_stream()
    layout = pkg.Modulator.frontend_describe(eti[0])
    y = np.asarray(O.Chain(mode=SC.OP_MODE, stages=3, gain_mode=2, normalise=SC.NORMALISE).process(bits)).reshape(SC.OP_FRAMES, -1)
    power = CC.data_power(y, SC.OP_MODE)
    K = MODES[SC.OP_MODE][1]

    def paths(cn_db, n_tones=None, ci_db=None):
        """payload bit errors per returned frame: (unweighted, weighted)"""
        yn = XC.op_input(y, power, cn_db, n_tones, ci_db, pkg.channel_sigma)
        ms = [X.demod_csi_model(f, SC.OP_MODE, SC.OP_EARLY) for f in yn]
        plain = np.stack([X.softs_of(m["u"], np.ones(K), SC.OP_MODE) for m in ms])
        # (the unweighted softs are tests/soft_model.py's: the same steps)
        assert np.array_equal(plain[0], S.demod_soft_model(yn[0], SC.OP_MODE, SC.OP_EARLY))
        weighted = np.stack([m["soft"] for m in ms])
        return (SC.frame_errors(S.decode_soft_stream(layout, plain, ref)[1]),
                SC.frame_errors(S.decode_soft_stream(layout, weighted, ref)[1]))
    return paths


def test_operating_point_weighted_decodes_what_unweighted_loses(op):
    """The search of csi_cases: C/I downwards in 1 dB steps at C/N = OP_CN_DB; L = the highest level at which the unweighted path
    has a payload bit error in every returned frame; the weighted path has none at L and 1 and 2 dB either side.  Combs are tried
    in order; the first that qualifies is the one csi_cases records (and the GPU test uses)."""
    found = None
    for n in XC.OP_COMBS_TRIED:
        level = None
        for ci in range(XC.OP_CI_START_DB, XC.OP_CI_STOP_DB - 1, -1):
            plain, weighted = op(XC.OP_CN_DB, n, ci)
            if all(e > 0 for e in plain):
                level = ci
                break
        assert level is not None, n
        at = {back: op(XC.OP_CN_DB, n, level + back) for back in range(-XC.OP_MARGIN_DB, XC.OP_MARGIN_DB + 1)}
        print("%d tone(s): L = %d dB; " % (n, level) +
              "; ".join("%+d dB: unweighted %s weighted %s" % (b, at[b][0], at[b][1]) for b in sorted(at)))
        if not any(any(at[b][1]) for b in at):
            found = (n, level)
            break
    assert found == (XC.OP_TONES, XC.OP_CI_DB)
    recorded = open(os.path.join(ROOT, "profiles", "csi.txt")).read()
    assert re.search(r"operating point: %d tone\(s\), C/N %.1f dB, L = C/I %d dB" % (found[0], XC.OP_CN_DB, found[1]), recorded)


def test_white_noise_costs_little(op):
    """Noise alone, C/N downwards in 0.25 dB steps: the last level before a path first loses a returned frame.  The figures are
    measured, not chosen; asserted is that the search gives what csi_cases records and that the weighted path is clean there."""
    last = {}
    for cn in np.arange(XC.WN_START_DB, XC.WN_STOP_DB - 1e-9, -XC.WN_STEP_DB):
        plain, weighted = op(float(cn))
        for name, errs in (("unweighted", plain), ("weighted", weighted)):
            if name not in last and any(errs):
                last[name] = float(cn) + XC.WN_STEP_DB
        if len(last) == 2:
            break
    print("white noise: weighted clean down to %.2f dB, unweighted down to %.2f dB" % (last["weighted"], last["unweighted"]))
    assert (last["weighted"], last["unweighted"]) == (XC.WN_WEIGHTED_DB, XC.WN_UNWEIGHTED_DB)
    assert not any(op(XC.WN_WEIGHTED_DB)[1])
    recorded = open(os.path.join(ROOT, "profiles", "csi.txt")).read()
    assert re.search(r"white noise: weighted clean down to %.2f dB, unweighted down to %.2f dB" % (XC.WN_WEIGHTED_DB, XC.WN_UNWEIGHTED_DB), recorded)
