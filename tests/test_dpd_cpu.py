"""The DPD measurement without a device (include/dabgpu.h, "DPD measurement"): the host-only alignment solve on the model's
cross-spectra of synthetic captures, the fractional-delay taps, the statistics model and the reference-basis fit against the
reference's own engine (tests/golden/dpd_reference.json, written by tests/golden/make_dpd_golden.py), and the closed loop in
the model with the oracle's predistorter."""
import json
import os

import numpy as np
import pytest

from tests.conftest import ROOT, load_pkg
from tests import dpd_cases as DC
from tests import dpd_model as DM

GOLDEN = os.path.join(ROOT, "tests", "golden", "dpd_reference.json")


def _two_pass(solve, tx, rx):
    """Pass 1 at offset 0 gives the lag, pass 2 at rx_offset = lag the rest -- with `solve` on the model's cross-spectra."""
    S, pt, pr, _ = DM.xspectrum(tx, rx, 0)
    a1 = solve(S, pt, pr)
    S, pt, pr, _ = DM.xspectrum(tx, rx, a1["lag"])
    a2 = solve(S, pt, pr)
    a2["lag"] += a1["lag"]
    return a2


# --------------------------------------------------------------------------- 1. alignment
@pytest.mark.parametrize("delay", DC.DELAYS)
def test_alignment_of_a_synthetic_capture(delay):
    """Band-limited noise, delayed by a float64 phase ramp, gain 0.8 e^{0.4j}, noise at -60 dB.  The library's solve on the
    model's cross-spectra: the integer lag exact (either neighbour where the delay lies half-way), lag + tau within 1e-3
    samples, gain x capture gain within 1e-3 of 1; and within 1e-8 of the model's own solve."""
    pkg = load_pkg()
    tx, rx = DC.block(), DC.capture(delay)
    got = _two_pass(pkg.dpd_solve_alignment, tx, rx)
    want = _two_pass(DM.solve_alignment, tx, rx)
    total = got["lag"] + got["tau"]
    gg = got["gain"] * DC.GAIN0
    print("delay %g: lag %d tau %.6f (error %.3g)  |g g0| - 1 = %.3g  angle %.3g  coherence %.6f"
          % (delay, got["lag"], got["tau"], total - delay, abs(gg) - 1.0, np.angle(gg), got["coherence"]))
    frac = abs(delay - round(delay))
    if frac < 0.45:
        assert got["lag"] == int(round(delay))
    else:
        assert got["lag"] in (int(np.floor(delay)), int(np.ceil(delay)))
    assert abs(total - delay) <= 1e-3
    assert abs(gg - 1.0) <= 1e-3
    assert 0.99 < got["coherence"] <= 1.0 + 1e-12
    assert got["lag"] == want["lag"]
    assert abs(got["tau"] - want["tau"]) <= 1e-8
    assert abs(got["gain"] - want["gain"]) <= 1e-8 * abs(want["gain"])
    assert abs(got["coherence"] - want["coherence"]) <= 1e-8


def test_solve_alignment_refuses_what_it_cannot_use():
    pkg = load_pkg()
    z = np.zeros(2048)
    with pytest.raises(pkg.DabGpuError) as e:
        pkg.dpd_solve_alignment(z.astype(np.complex128), z, z)
    assert "no power" in str(e.value)
    with pytest.raises(pkg.DabGpuError):
        pkg.dpd_solve_alignment(np.ones(100, np.complex128), z, z)


# --------------------------------------------------------------------------- 2. the delay taps
def test_delay_taps():
    """tau = 0 is the unit impulse bit for bit; on |f| <= 0.375 cycles per sample the response sum_j h[j] e^{-2 pi j f (j - 15)}
    is within 5e-5 of e^{-2 pi j f tau} (measured 1.19e-5, 1.80e-5, 2.45e-5 at tau 0.25, 0.5, -0.37); the table is the
    model's formula rounded once."""
    pkg = load_pkg()
    h0 = pkg.dpd_delay_taps(0.0)
    want = np.zeros(32, np.float32)
    want[15] = 1.0
    assert h0.dtype == np.float32 and np.array_equal(h0.view(np.uint32), want.view(np.uint32))
    f = np.linspace(-0.375, 0.375, 1501)
    m = np.arange(32) - 15
    for tau in (0.25, 0.5, -0.37):
        h = pkg.dpd_delay_taps(tau).astype(np.float64)
        H = (h[None, :] * np.exp(-2j * np.pi * f[:, None] * m[None, :])).sum(axis=1)
        err = float(np.abs(H - np.exp(-2j * np.pi * f * tau)).max())
        dev = float(np.abs(h - DM.delay_taps(tau)).max())
        print("tau %g: response error %.3g, |table - formula| %.3g" % (tau, err, dev))
        assert err <= 5e-5
        assert dev <= 2.0 ** -24                     # one fp32 rounding of a value of at most 1
    for bad in (1.0, -1.0, float("nan")):
        with pytest.raises(pkg.DabGpuError):
            pkg.dpd_delay_taps(bad)


# --------------------------------------------------------------------------- 3. the reference's own engine
def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


def _none_to_nan(v):
    return np.array([np.nan if x is None else x for x in v], np.float64)


def test_model_statistics_are_the_references():
    """The model's bins equal ExtractStatistic's counts exactly; mean |rx| and mean phase within 1e-6 relative (float64 sums
    against numpy's float32 mean of complex64 values)."""
    g = _golden()
    p = g["params"]
    assert p == DC.GOLDEN
    tx, rx = DC.golden_pair(p)
    st = DM.stats(tx, rx, peak=p["peak"], n_bins=p["n_bins"])
    assert [int(v) for v in st["count"]] == g["counts"]
    assert st["samples_used"] == p["n"] - 31 and st["overflow"] == st["samples_used"] - sum(g["counts"])
    n = np.array(g["counts"], np.float64)
    have = n > 0
    rx_ref, ph_ref = _none_to_nan(g["mean_rx"]), _none_to_nan(g["mean_phase"])
    d_rx = np.abs(st["sum_rx"][have] / n[have] - rx_ref[have]) / rx_ref[have]
    # (the phase is held relative to the largest mean phase: a mean near zero has no relative accuracy)
    d_ph = np.abs(st["sum_phase"][have] / n[have] - ph_ref[have]) / np.abs(ph_ref[have]).max()
    print("mean |rx| %.3g, mean phase %.3g (relative)" % (d_rx.max(), d_ph.max()))
    assert d_rx.max() <= 1e-6 and d_ph.max() <= 1e-6
    centre = (np.arange(p["n_bins"]) + 0.5) * p["peak"] / p["n_bins"]
    assert np.allclose(g["tx_centre"], centre, rtol=1e-12)


def _golden_stats(g):
    n = np.array(g["counts"], np.float64)
    return {"n_bins": g["params"]["n_bins"], "peak": g["params"]["peak"], "count": np.array(g["counts"]),
            "sum_tx": np.zeros_like(n), "sum_rx": np.nan_to_num(_none_to_nan(g["mean_rx"])) * n,
            "sum_phase": np.nan_to_num(_none_to_nan(g["mean_phase"])) * n}


def test_reference_basis_fit_is_float64_least_squares_on_the_references_values():
    """dabgpu_dpd_fit_poly(BASIS_REFERENCE) against numpy's float64 least squares on the same fp32 abscissae (the reference's
    per-bin values, its leading run of bins, its tx_min rule, powers rounded to fp32): measured 2.84e-8 (AM/AM) and 6.92e-9
    (AM/PM), fp32 roundings of the result -- held to one fp32 ulp of the largest coefficient."""
    pkg = load_pkg()
    g = _golden()
    p = g["params"]
    st = _golden_stats(g)
    am, pm, info = pkg.dpd_fit_poly(st, "reference", min_count=p["min_count"], weighted=False, tx_min=p["tx_min"])
    wam, wpm = DM.fit_poly(st, "reference", p["min_count"], False, p["tx_min"])
    assert info["bins_used"] == g["bins_fitted"]
    d_am, d_pm = np.abs(am - wam).max(), np.abs(pm - wpm).max()
    print("against float64 numpy: am %.3g pm %.3g; cond %.3g / %.3g" % (d_am, d_pm, info["cond_am"], info["cond_pm"]))
    assert d_am <= np.spacing(np.float32(np.abs(wam).max())) and d_pm <= np.spacing(np.float32(np.abs(wpm).max()))


def test_reference_basis_fit_against_model_poly():
    """dabgpu_dpd_fit_poly(BASIS_REFERENCE) against Model_Poly's own coefficients at lr = 1
    (tests/golden/dpd_reference.json).  Measured: 0 for AM/AM and AM/PM -- the same ten fp32 numbers.  Both sides round a
    float64 solution to fp32, and two solutions that agree to 1e-9 can still fall either side of a rounding boundary, so the
    bar is not four times zero but the cap: one fp32 ulp of the largest coefficient (5.96e-8 / 1.49e-8).

    Model_Poly forms its design matrices as `sig ** i` on float32 arrays, and so does the library: the powers rounded to
    fp32.  The golden is generated with numpy's plain float32 power, which is the correctly rounded one (the generator asserts
    it).  With numpy's AVX-512 float32 power (off by up to 0.95 ulp per entry, and not the same function on every CPU) the
    reference's own coefficients move by 2.7e-5 (AM/AM) and 5.4e-7 (AM/PM): the unscaled matrix has a condition number of
    several thousand.  That is the reference's reproducibility, not the fit's accuracy."""
    pkg = load_pkg()
    g = _golden()
    p = g["params"]
    am, pm, _ = pkg.dpd_fit_poly(_golden_stats(g), "reference", min_count=p["min_count"], weighted=False, tx_min=p["tx_min"])
    ram, rpm = np.array(g["coefs_am"]), np.array(g["coefs_pm"])
    d_am, d_pm = np.abs(am - ram).max(), np.abs(pm - rpm).max()
    cap_am, cap_pm = np.spacing(np.float32(np.abs(ram).max())), np.spacing(np.float32(np.abs(rpm).max()))
    print("against Model_Poly: am %.3g (cap %.3g)  pm %.3g (cap %.3g)" % (d_am, cap_am, d_pm, cap_pm))
    assert d_am <= cap_am and d_pm <= cap_pm


def test_learning_rate_is_applied_once_and_few_bins_are_refused():
    pkg = load_pkg()
    g = _golden()
    st = _golden_stats(g)
    full_am, full_pm, _ = pkg.dpd_fit_poly(st, "reference", min_count=10, weighted=False, tx_min=0.1)
    prev_am, prev_pm = np.array([1, 0.1, 0, 0, 0], np.float32), np.array([0, 0.05, 0, 0, 0], np.float32)
    am, pm, _ = pkg.dpd_fit_poly(st, "reference", min_count=10, weighted=False, tx_min=0.1, prev_am=prev_am, prev_pm=prev_pm,
                                 lr_am=0.5, lr_pm=0.25)
    assert np.allclose(am, prev_am + 0.5 * (full_am - prev_am), rtol=0, atol=2e-7)
    assert np.allclose(pm, prev_pm + 0.25 * (full_pm - prev_pm), rtol=0, atol=2e-7)
    few = dict(st, count=np.where(np.arange(64) < 5, st["count"], 0))
    for basis in ("magsq", "reference"):
        with pytest.raises(pkg.DabGpuError) as e:
            pkg.dpd_fit_poly(few, basis, min_count=1)
        assert "fewer than six" in str(e.value)
    with pytest.raises(pkg.DabGpuError):
        pkg.dpd_fit_poly(dict(st, peak=0.0), "magsq")


# --------------------------------------------------------------------------- 4. the loop closes in the model
def _model_loop(x):
    """One iteration: normalise by the least-squares gain, bin, fit MAGSQ (weighted, min_count 1), predistort with the
    oracle's polynomial stage.  Returns (am, pm, stats, residual before, residual after)."""
    import oracle as O
    y = DC.pa(x)
    g = np.vdot(y, x) / np.vdot(y, y)
    peak = float(np.abs(x).max()) * 1.0001
    st = DM.stats(x, (g * y).astype(np.complex64), peak=peak, n_bins=64)
    am, pm = DM.fit_poly(st, "magsq", 1, True)
    xp = O.memless_poly(np.array(x), am.astype(np.float32), pm.astype(np.float32))
    return am, pm, st, DC.residual_db(y, x), DC.residual_db(DC.pa(xp), x)


def test_the_loop_closes_in_the_model():
    """The amplifier model of tests/dpd_cases.py on the band-limited block (rms 0.25, peak near 0.9): the residual against
    the clean signal falls by at least 10 dB with the oracle's predistorter (the reference's phasor approximation) --
    measured -36.1 dB -> -73.8 dB.  The library's MAGSQ fit on the model's statistics gives the model's coefficients."""
    pkg = load_pkg()
    x = DC.block()
    assert abs(np.sqrt(np.mean(np.abs(x.astype(np.complex128)) ** 2)) - 0.25) < 1e-6 and 0.8 < np.abs(x).max() < 1.0
    am, pm, st, before, after = _model_loop(x)
    print("residual %.2f dB -> %.2f dB; am %s pm %s" % (before, after, am, pm))
    assert after <= before - 10.0
    lam, lpm, info = pkg.dpd_fit_poly(st, "magsq", min_count=1, weighted=True)
    assert info["bins_used"] == int((st["count"] > 0).sum())
    assert np.abs(lam - am).max() <= np.spacing(np.float32(np.abs(am).max()))
    assert np.abs(lpm - pm).max() <= np.spacing(np.float32(np.abs(pm).max()))


# --------------------------------------------------------------------------- 5. the model itself
def test_model_segment_and_sample_rules():
    assert DM.segments(2047, 0) == [] and DM.segments(2048, 0) == [0] and DM.segments(3072, 0) == [0, 1]
    assert DM.segments(2048 + 1024 * 7 + 513, 7) == list(range(8)) and DM.segments(2048 + 1024 * 7 + 513, 1000) == list(range(7))
    assert DM.segments(2048 + 1024 * 7 + 513, -300) == list(range(1, 8)) and DM.segments(3071, -300) == []
    x = DC.block()
    for n, lag, used in ((31, 0, 0), (32, 0, 1), (33, 0, 2), (2048, 7, 2048 - 31 - 7 + 7), (2048, -300, 2048 - 300 - 16), (2048, 1000, 2048 - 1000 - 16)):
        st = DM.stats(x[:n], x[:n], lag=lag, peak=1.0)
        want = max(0, min(n, n - 16 - lag) - max(0, 15 - lag))
        assert st["samples_used"] == want, (n, lag)
    # rx = tx through the impulse: phase 0 and |r| = |t| (to float64 rounding in the model; exactly on the device)
    st = DM.stats(x, x, peak=1.0)
    assert np.abs(st["sum_phase"]).max() < 1e-12 and np.allclose(st["sum_rx"], st["sum_tx"], rtol=1e-14, atol=0)
    # a sample exactly on an edge belongs to the bin above; at the last edge it is overflow
    t = np.array([0.25 + 0j, 0.5 + 0j, 1.0 + 0j] + [0.1] * 40, np.complex64)
    st = DM.stats(np.concatenate([np.full(15, 0.1, np.complex64), t]), np.ones(15 + t.size, np.complex64), peak=1.0, n_bins=4)
    assert st["count"][1] == 1 and st["count"][2] == 1 and st["overflow"] == 1
