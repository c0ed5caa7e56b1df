"""The spectrum monitor without a device: the window tables against their formulas, the float64 yardstick
(tests/spectrum_model.py) against what a periodogram must give, the host-only mask check against the model's restatement of
its rule, and the header."""
import os
import re

import numpy as np
import pytest

from tests.conftest import ROOT, load_pkg
from tests import spectrum_cases as SC
from tests import spectrum_model as SM


@pytest.mark.parametrize("window", [0, 1, 2])
def test_window_tables_are_the_formulas_rounded_once(window):
    """|table - formula| <= 2^-24: one fp32 rounding of a value of at most 1."""
    pkg = load_pkg()
    w = pkg.spectrum_window(window)
    assert w.dtype == np.float32 and w.shape == (2048,)
    want = SM.window_formula(window)
    assert want.max() <= 1.0 + 1e-15
    dev = float(np.max(np.abs(w.astype(np.float64) - want)))
    print("window %d: max |table - formula| = %.3g" % (window, dev))
    assert dev <= 2.0 ** -24
    if window:
        assert abs(float(w[1024]) - 1.0) <= 2.0 ** -24 and w[0] < 1e-4      # periodic form: the peak sits on sample N/2


def test_unknown_window_is_refused_without_a_device():
    pkg = load_pkg()
    for bad in (-1, 3):
        with pytest.raises(pkg.DabGpuError) as e:
            pkg.spectrum_window(bad)
        assert "window is 0" in str(e.value)


def test_model_puts_a_bin_centred_tone_in_its_bin_and_keeps_parseval():
    """Rectangular window: a unit tone on bin b gives segments x 2048^2 in bin b and nothing elsewhere; per segment the sum
    over the bins is 2048 x the segment's energy.  The segment rule: 1024 i ... 1024 i + 2047, none below 2048 samples."""
    n = np.arange(5 * 2048 + 700)
    x = np.exp(2j * np.pi * (37 / 2048.0) * n).astype(np.complex64)
    raw, segs = SM.welch_raw(x, np.ones(2048, np.float32))
    assert segs == 9 == SM.n_segments(x.size)
    assert abs(raw[37] / (segs * 2048.0 ** 2) - 1.0) < 1e-6
    assert np.delete(raw, 37).max() < 1e-6 * raw[37]
    rng = np.random.default_rng(3)
    y = (rng.standard_normal(2048) + 1j * rng.standard_normal(2048)).astype(np.complex64)
    raw, segs = SM.welch_raw(y, np.ones(2048, np.float32))
    assert segs == 1 and abs(raw.sum() / (2048.0 * np.sum(np.abs(y.astype(np.complex128)) ** 2)) - 1.0) < 1e-12
    assert [SM.n_segments(k) for k in (0, 2047, 2048, 3071, 3072, 2048 + 1024 * 7 + 513)] == [0, 0, 1, 1, 2, 8]
    assert SM.welch_raw(y[:2047], np.ones(2048, np.float32))[1] == 0
    # the integer formats: the value as it is, uint8 - 128
    assert np.array_equal(SM.as_complex(np.array([128, 0, 255, 127], np.uint8)), np.array([-128j, 127 - 1j]))
    assert np.array_equal(SM.as_complex(np.array([-3, 4], np.int8)), np.array([-3 + 4j]))
    assert np.array_equal(SM.as_complex(np.array([-300, 4], np.int16)), np.array([-300 + 4j]))


def test_the_synthetic_signal_is_what_the_tests_say():
    x = SC.signal()
    assert x.dtype == np.complex64 and x.size == 40 * 2048 and SM.n_segments(x.size) == 79
    raw, _ = SM.welch_raw(x, load_pkg().spectrum_window(2))
    lvl = 10 * np.log10(raw / raw[100])
    assert abs(lvl[2048 - 900] + 60.0) < 0.1 and lvl[1500] < -95.0            # (-900: bin-centred; the floor is the noise)
    assert SC.samples("s16").dtype == np.int16 and abs(int(SC.samples("s16").max()) - 3000) < 40
    u8, s8 = SC.samples("u8"), SC.samples("s8")
    assert u8.dtype == np.uint8 and s8.dtype == np.int8 and np.array_equal(u8.astype(np.int16) - 128, s8.astype(np.int16))


def _flat(rate=2048000.0, nfft=2048):
    """In-band 1.0, out of band -40 dB."""
    f = np.abs(SM.bin_freqs(nfft, rate))
    raw = np.where(f <= SM.BAND_HZ, 1.0, 1e-4)
    raw[0] = 7.0                                       # DC is no part of the reference
    return raw, f


def _same(got, want):
    for k in ("n_violations", "n_checked"):
        assert got[k] == want[k], (k, got, want)
    for k in ("ref", "worst_margin_db", "worst_freq_hz", "oob_max_db", "oob_freq_hz"):
        assert got[k] == pytest.approx(want[k], rel=1e-12, abs=1e-9), (k, got[k], want[k])


def test_check_mask_follows_the_rule_on_synthetic_spectra():
    pkg = load_pkg()
    rate = 2048000.0
    raw, f = _flat(rate)
    mask = [(800e3, -20.0), (900e3, -30.0), (1000e3, -35.0)]
    got = pkg.check_mask(raw, rate, mask)
    want = SM.check_mask_model(raw, rate, mask)
    _same(got, want)
    assert got["ref"] == 1.0 and got["n_violations"] == 0 and got["worst_margin_db"] == pytest.approx(5.0)
    assert got["n_checked"] == int(np.sum(f >= 800e3)) and got["oob_max_db"] == pytest.approx(-40.0)
    # a violation at one known bin, on the negative side; it is also the out-of-band maximum
    k = 2048 - 980                                      # -980 kHz: between the points at 900 and 1000 kHz, limit -34 dB
    bad = raw.copy()
    bad[k] = 10.0 ** (-31.0 / 10.0)
    got = pkg.check_mask(bad, rate, mask)
    _same(got, SM.check_mask_model(bad, rate, mask))
    assert got["n_violations"] == 1 and got["worst_freq_hz"] == -980e3 and got["worst_margin_db"] == pytest.approx(-3.0)
    assert got["oob_max_db"] == pytest.approx(-31.0) and got["oob_freq_hz"] == -980e3
    # oob_from_hz is a parameter: looked for from 990 kHz, the bin at 980 kHz is not part of it
    assert pkg.check_mask(bad, rate, mask, oob_from_hz=990e3)["oob_max_db"] == pytest.approx(-40.0)
    # interpolation between points: just under the line passes, just over it fails
    for db, nviol in ((-34.1, 0), (-33.9, 1)):
        t = raw.copy()
        t[k] = 10.0 ** (db / 10.0)
        assert pkg.check_mask(t, rate, mask)["n_violations"] == nviol, db
    # bins below the first point are not checked, however loud
    t = raw.copy()
    t[790] = 1e3
    got = pkg.check_mask(t, rate, mask)
    _same(got, SM.check_mask_model(t, rate, mask))
    assert got["n_violations"] == 0
    # the last value holds beyond the last offset
    t = raw.copy()
    t[1024] = 10.0 ** (-34.0 / 10.0)                     # -1024 kHz
    got = pkg.check_mask(t, rate, mask)
    assert got["n_violations"] == 1 and got["worst_freq_hz"] == -1024e3 and got["worst_margin_db"] == pytest.approx(-1.0)
    # no points: ref and the out-of-band maximum only
    got = pkg.check_mask(bad, rate)
    assert got["n_checked"] == 0 and got["n_violations"] == 0 and got["ref"] == 1.0 and got["oob_max_db"] == pytest.approx(-31.0)
    # another rate and a random spectrum: a resampled chain's axis
    rng = np.random.default_rng(8)
    r4 = rng.uniform(0.5, 2.0, 2048)
    m4 = [(900e3, 3.0), (2e6, 0.5), (3.5e6, 0.0)]
    _same(pkg.check_mask(r4, 8192000.0, m4), SM.check_mask_model(r4, 8192000.0, m4))


def test_check_mask_refusals():
    pkg = load_pkg()
    raw, _ = _flat()
    for kw, text in ((dict(rate_hz=0.0), "rate_hz"), (dict(rate_hz=1e12), "no bin lies in the occupied band"),
                     (dict(mask=[(900e3, -30.0), (800e3, -20.0)]), "strictly increasing"),
                     (dict(mask=[(800e3, -20.0), (800e3, -30.0)]), "strictly increasing")):
        args = dict(rate_hz=2048000.0, mask=())
        args.update(kw)
        with pytest.raises(pkg.DabGpuError) as e:
            pkg.check_mask(raw, args["rate_hz"], args["mask"])
        assert text in str(e.value), (kw, str(e.value))
    with pytest.raises(pkg.DabGpuError) as e:
        pkg.check_mask(np.zeros(2048), 2048000.0)
    assert "zero" in str(e.value)


def test_header_documents_every_new_entry():
    text = open(os.path.join(ROOT, "include", "dabgpu.h")).read()
    names = set(re.findall(r"DABGPU_API[^;]*?\b(dabgpu_[a-z_0-9]+)\s*\(", text, re.S))
    want = {"dabgpu_spectrum_window", "dabgpu_spectrum", "dabgpu_spectrum_dev", "dabgpu_get_spectrum", "dabgpu_reset_spectrum",
            "dabgpu_set_spectrum_monitor", "dabgpu_debug_spectrum_run_segments", "dabgpu_spectrum_check_mask"}
    assert want <= names
    pkg = load_pkg()
    assert want <= set(pkg.EXPORTS)
    comments = " ".join(re.findall(r"/\*.*?\*/", text, re.S))
    for n in want:
        assert re.search(r"\b%s\b" % n, comments), "no comment in the header speaks of %s" % n
    for m in ("spectrum", "spectrum_dev", "set_spectrum_monitor", "reset_spectrum", "spectrum_stats"):
        assert hasattr(pkg.Modulator, m), m
    info = re.search(r"typedef struct dabgpu_spectrum_info \{(.*?)\}", text, re.S).group(1)
    for field in ("segments", "nfft", "window", "sum_w2", "rate_hz"):
        assert field in info, field
    res = re.search(r"typedef struct dabgpu_mask_result \{(.*?)\}", text, re.S).group(1)
    for field in ("ref", "worst_margin_db", "worst_freq_hz", "n_violations", "oob_max_db", "oob_freq_hz"):
        assert field in res, field
