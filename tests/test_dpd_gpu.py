"""The DPD measurement on the device (dpd.hip; include/dabgpu.h, "DPD measurement"): the cross-spectrum against the float64
model at the edges of the segment rule, its run geometry and determinism; the aligned amplitude-bin statistics against the
model -- counts exactly, means to measured bars -- the impulse path, tile geometry, accumulation; the closed loop through the
library; dabmod_file --dpd-feedback; the refusals; the launch trace."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import dpd_cases as DC
from tests import dpd_model as DM
from tests.conftest import ROOT, record_bound
from tests.golden.synth import synth_bits, synth_eti

pytestmark = pytest.mark.gpu
HOST = os.path.join(ROOT, "odr-dabmod_amd", "host")
CFG3 = 1 | 2

# The cross-spectrum against the float64 model, per array (Re / Im of S taken together as |S_dev - S_model|, P_tx, P_rx):
#   (a) max |dev - model| / |model| over the bins with |model| >= mean |model|
#   (b) max |dev - model| / (|model| + 1e-9 mean |model|) over all bins
# (a) takes the bins at or above the mean level, not the spectrum test's "within 40 dB of the largest": the error an fp32
# transform leaves in a bin is a fraction (about 2^-24 sqrt(log2 2048) = 2e-7 in amplitude) of the segment's rms bin level,
# whatever the bin holds.  The spectrum test's tones put their energy into a few bins, so every bin within 40 dB of them is
# far above that floor; the noise-like block here fills 1500 bins evenly, and a bin 40 dB under the largest lies two orders
# under the rms level, where the same absolute error is 1e-5 of the bin (measured: 1.2e-5).  Those bins are held by (b).
# Bars: four times the worst value measured on the MI355X (profiles/dpd.txt), never above the spectrum kernel's caps of
# INTEGRATION.md F (2e-6 and 5e-2): it is the same transform and the same accumulation.
# Measured: (a) 5.63e-7 (P_rx, 3072 samples, offset -300), (b) 7.27e-5 (the same case); no run-to-run variation.
X_WORST_A, X_WORST_B = 5.63e-7, 7.27e-5
X_BAR_A = 2e-6 if X_WORST_A is None else min(4 * X_WORST_A, 2e-6)
X_BAR_B = 5e-2 if X_WORST_B is None else min(4 * X_WORST_B, 5e-2)
# The statistics' per-bin means against the float64 model, over the bins that hold a sample: mean |t| and mean |r| relative to
# peak, mean |r|^2 relative to peak^2, mean phase and mean phase^2 (rad, rad^2) on the bins whose centre is at least 0.1 peak
# (below that the phase of an fp32 32-tap sum is noise).  Bars: four times the worst value measured (profiles/dpd.txt).
# Without a measured value a bar is what fp32 allows at most: 2^-20 (sixteen ulp of an amplitude near peak; phases: the same in
# rad for amplitudes above 0.1 peak, where an error of 2^-24 peak in r turns the phase by at most 2^-24 / 0.1 rad).
# Measured: mean |t| 4.42e-8, mean |r| 2.49e-7, mean |r|^2 3.96e-7, mean phase 1.34e-7 rad, mean phase^2 2.92e-8 rad^2.
S_WORST = {"tx": 4.42e-8, "rx": 2.49e-7, "rx2": 3.96e-7, "phase": 1.34e-7, "phase2": 2.92e-8}
S_BAR = {k: 2.0 ** -20 if v is None else 4 * v for k, v in S_WORST.items()}
STATS_PEAK = 0.75                       # (the block's largest |x| is near 0.9: some samples overflow)
TILE = 2048
_models = {}


def _cuda(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()


def _xmodel(fmt, n, off, delay=0.37):
    key = ("x", fmt, n, off, delay)
    if key not in _models:
        tx = DC.block()[:n] if fmt == "cf32" else DC.block_s16()[:2 * n]
        _models[key] = DM.xspectrum(tx, DC.capture(delay)[:n], off)
    return _models[key]


def _xfigures(dev, model):
    err, mag = np.abs(dev - model), np.abs(model)
    if not mag.max() > 0:
        return 0.0, float(err.max())
    strong = mag >= mag.mean()
    return float(np.max(err[strong] / mag[strong])), float(np.max(err / (mag + 1e-9 * mag.mean())))


def _xcheck(got, model, label):
    S, pt, pr, segs = model
    assert got["segments"] == segs, (label, got["segments"], segs)
    if segs == 0:
        assert not got["S"].any() and not got["p_tx"].any() and not got["p_rx"].any()
        return True
    ok = True
    for name, d, m in (("S", got["S"], S), ("P_tx", got["p_tx"], pt), ("P_rx", got["p_rx"], pr)):
        a, b = _xfigures(d, m)
        print("xspectrum %s %s: (a) %.3g  (b) %.3g" % (label, name, a, b))
        ok_a = record_bound("dpd xspectrum (a) %s, %s" % (name, label), a, X_BAR_A)
        ok_b = record_bound("dpd xspectrum (b) %s, %s" % (name, label), b, X_BAR_B)
        ok = ok and ok_a and ok_b
    return ok


# --------------------------------------------------------------------------- 1. the cross-spectrum
@pytest.mark.parametrize("fmt", ["cf32", "s16"])
def test_cross_spectrum_follows_the_model_at_the_edges_of_the_segment_rule(pkg, fmt):
    md = pkg.Modulator(mode=1 if fmt == "cf32" else 2, max_frames=1)      # (Mode I reads the context's own twiddle table)
    try:
        d_tx = _cuda(DC.block() if fmt == "cf32" else DC.block_s16())
        d_rx = _cuda(DC.capture(0.37))
        ok = True
        for n in (2047, 2048, 3071, 3072, 2048 + 1024 * 7 + 513):
            for off in (0, 7, -300, 1000):
                md.dpd_xspectrum_dev(d_tx, d_rx, off, n_samples=n)
                got = md.dpd_xspectrum_result()
                assert got["segments"] == len(DM.segments(n, off))
                ok = _xcheck(got, _xmodel(fmt, n, off), "%s n %d offset %d" % (fmt, n, off)) and ok
        # the whole block, and the host-pointer form: the same bits
        md.dpd_xspectrum_dev(d_tx, d_rx, -300)
        got = md.dpd_xspectrum_result()
        ok = _xcheck(got, _xmodel(fmt, DC.N_SAMPLES, -300), "%s whole block offset -300" % fmt) and ok
        host = md.dpd_xspectrum(DC.block() if fmt == "cf32" else DC.block_s16(), DC.capture(0.37), -300)
        assert np.array_equal(host["S"].view(np.uint64), got["S"].view(np.uint64)) and host["segments"] == got["segments"] == 40
        assert ok
    finally:
        md.close()


def _same_but_for_order(got, want, scale, segments):
    """Within 2 segments 2^-53 of the sum of the terms' magnitudes, which `scale` bounds: the float64 reordering bound."""
    tol = 2.0 * segments * 2.0 ** -53
    assert np.all(np.abs(got - want) <= tol * scale), float(np.max(np.abs(got - want) / np.maximum(scale, 1e-300)))


def test_cross_spectrum_run_geometry_and_determinism(pkg):
    md = pkg.Modulator(mode=1, max_frames=1)
    try:
        d_tx, d_rx = _cuda(DC.block()), _cuda(DC.capture(0.37))
        md.dpd_xspectrum_dev(d_tx, d_rx, 7)
        first = md.dpd_xspectrum_result()
        assert first["segments"] == 40
        md.dpd_xspectrum_dev(d_tx, d_rx, 7)
        again = md.dpd_xspectrum_result()
        for k in ("S", "p_tx", "p_rx"):
            assert np.array_equal(again[k].view(np.uint64), first[k].view(np.uint64))
        # |S[k]| terms are bounded by sqrt(P_tx P_rx) per segment, whose sum Cauchy-Schwarz bounds by sqrt(sum P_tx sum P_rx)
        s_scale = np.sqrt(first["p_tx"] * first["p_rx"])
        for run in (1, 2, 7, 40):
            md.set_dpd_geometry(run_segments=run)
            md.dpd_xspectrum_dev(d_tx, d_rx, 7)
            got = md.dpd_xspectrum_result()
            assert got["segments"] == 40
            _same_but_for_order(got["S"].real, first["S"].real, s_scale, 40)
            _same_but_for_order(got["S"].imag, first["S"].imag, s_scale, 40)
            _same_but_for_order(got["p_tx"], first["p_tx"], first["p_tx"], 40)
            _same_but_for_order(got["p_rx"], first["p_rx"], first["p_rx"], 40)
            md.dpd_xspectrum_dev(d_tx, d_rx, 7)
            assert np.array_equal(md.dpd_xspectrum_result()["S"].view(np.uint64), got["S"].view(np.uint64)), run
        md.set_dpd_geometry()
        md.dpd_xspectrum_dev(d_tx, d_rx, 7)
        assert np.array_equal(md.dpd_xspectrum_result()["S"].view(np.uint64), first["S"].view(np.uint64))
    finally:
        md.close()


def test_short_forced_runs_follow_the_float64_model(pkg):
    """Runs of 3 segments and a shorter last one, then of one segment each, against the float64 model rather than the library's
    own default geometry: a half-segment that either walk over a run (welch.h: tx, and rx at rx_offset) shifted would be
    compared with itself there.  The first 2048 + 6 x 1024 samples, tx s16 in a Mode II context (the built table), rx_offset 0
    (7 segments) and -300 (6: the first has no rx range).  The model alone has 967 bins or more of every array at or above its
    mean level at this length: figure (a) is formed over them."""
    n = 2048 + 6 * 1024
    md = pkg.Modulator(mode=2, max_frames=1)
    try:
        d_tx, d_rx = _cuda(DC.block_s16()[:2 * n]), _cuda(DC.capture(0.37)[:n])
        ok = True
        for off, segs in ((0, 7), (-300, 6)):
            model = _xmodel("s16", n, off)
            assert model[3] == segs and all(np.count_nonzero(np.abs(m) >= np.abs(m).mean()) >= 1 for m in model[:3])
            for run in (3, 1):
                md.set_dpd_geometry(run_segments=run)
                md.dpd_xspectrum_dev(d_tx, d_rx, off)
                ok = _xcheck(md.dpd_xspectrum_result(), model, "s16 n %d offset %d in runs of %d" % (n, off, run)) and ok
        assert ok
    finally:
        md.close()


def test_align_on_the_device_finds_the_delay(pkg):
    """The two passes on the device against the two passes of the model (tests/test_dpd_cpu.py holds the solve itself)."""
    md = pkg.Modulator(mode=1, max_frames=1)
    try:
        d_tx = _cuda(DC.block())
        for delay in (0.37, -300.5, 511.25):
            al = md.dpd_align_dev(d_tx, _cuda(DC.capture(delay)))
            gg = al["gain"] * DC.GAIN0
            print("delay %g: lag %d tau %.6f gain error %.3g coherence %.6f" % (delay, al["lag"], al["tau"], abs(gg - 1), al["coherence"]))
            assert abs(al["lag"] + al["tau"] - delay) <= 1e-3 and abs(gg - 1.0) <= 1e-3 and al["coherence"] > 0.99
        host = md.dpd_align(DC.block(), DC.capture(511.25))
        assert host["lag"] == al["lag"] and host["tau"] == al["tau"] and host["gain"] == al["gain"]
        s16 = md.dpd_align(DC.block_s16(), DC.capture(0.37))
        assert s16["lag"] == 0 and abs(s16["tau"] - 0.37) <= 1e-3 and abs(s16["gain"] * DC.GAIN0 / DC.S16_SCALE - 1.0) <= 1e-3
    finally:
        md.close()


# --------------------------------------------------------------------------- 2. the statistics
def _smodel(fmt, n, lag, tau, gain, peak, taps):
    key = ("s", fmt, n, lag, tau, complex(gain), peak)
    if key not in _models:
        tx = DC.block()[:n] if fmt == "cf32" else DC.block_s16()[:2 * n]
        _models[key] = DM.stats(tx, DC.capture(lag + tau)[:n], lag, tau, gain, peak, DC.N_BINS, taps=taps)
    return _models[key]


def _scheck(st, model, label):
    """Counts, overflow and samples used exactly; the means to the bars.  Returns (ok, figures)."""
    assert st["samples_used"] == model["samples_used"] and st["overflow"] == model["overflow"], label
    assert np.array_equal(st["count"], model["count"]), label
    assert np.array_equal(st["raw"][:, 0], model["count"])
    n = model["count"].astype(np.float64)
    have = n > 0
    fig = dict.fromkeys(S_WORST, 0.0)
    if have.any():
        peak = model["peak"]
        centre = (np.arange(model["n_bins"]) + 0.5) * peak / model["n_bins"]
        loud = have & (centre >= 0.1 * peak)
        mean = lambda d, k, sel: np.abs(d[k][sel] / n[sel] - model[k][sel] / n[sel])
        fig["tx"] = float(np.max(mean(st, "sum_tx", have)) / peak)
        fig["rx"] = float(np.max(mean(st, "sum_rx", have)) / peak)
        fig["rx2"] = float(np.max(mean(st, "sum_rx2", have)) / peak ** 2)
        if loud.any():
            fig["phase"] = float(np.max(mean(st, "sum_phase", loud)))
            fig["phase2"] = float(np.max(mean(st, "sum_phase2", loud)))
    ok = True
    for k, v in fig.items():
        ok = record_bound("dpd stats mean %s, %s" % (k, label), v, S_BAR[k]) and ok
    print("stats %s: used %d overflow %d  %s" % (label, st["samples_used"], st["overflow"],
                                                   "  ".join("%s %.3g" % kv for kv in fig.items())))
    return ok


@pytest.mark.parametrize("tau", DC.STATS_TAUS)
@pytest.mark.parametrize("lag", DC.STATS_LAGS)
def test_statistics_follow_the_model(pkg, lag, tau):
    md = pkg.Modulator(mode=1, max_frames=1)
    try:
        gain = 1.0 / DC.GAIN0
        al = {"lag": lag, "tau": tau, "gain": gain}
        taps = pkg.dpd_delay_taps(tau)
        d_tx, d_rx = _cuda(DC.block()), _cuda(DC.capture(lag + tau))
        ok = True
        for n in (31, 32, 33, TILE - 1, TILE, TILE + 1, DC.N_SAMPLES):
            md.dpd_measure_dev(d_tx, d_rx, al, STATS_PEAK, DC.N_BINS, n_samples=n)
            st = md.dpd_stats()
            assert st["n_bins"] == DC.N_BINS and st["peak"] == np.float32(STATS_PEAK)
            ok = _scheck(st, _smodel("cf32", n, lag, tau, gain, STATS_PEAK, taps), "cf32 n %d lag %d tau %g" % (n, lag, tau)) and ok
        assert st["overflow"] > 0 and st["samples_used"] == DC.N_SAMPLES - max(0, 15 - lag) - max(0, 16 + lag)
        assert ok
    finally:
        md.close()


def test_statistics_of_s16_tx_and_the_host_pointer_form(pkg):
    md = pkg.Modulator(mode=3, max_frames=1)
    try:
        lag, tau, peak = 7, 0.37, STATS_PEAK * DC.S16_SCALE
        gain = DC.S16_SCALE / DC.GAIN0
        al = {"lag": lag, "tau": tau, "gain": gain}
        md.dpd_measure_dev(_cuda(DC.block_s16()), _cuda(DC.capture(lag + tau)), al, peak, DC.N_BINS)
        st = md.dpd_stats()
        ok = _scheck(st, _smodel("s16", DC.N_SAMPLES, lag, tau, gain, peak, pkg.dpd_delay_taps(tau)), "s16 whole block")
        md.dpd_measure(DC.block_s16(), DC.capture(lag + tau), al, peak, DC.N_BINS)
        assert np.array_equal(md.dpd_stats()["raw"], st["raw"])
        assert ok
    finally:
        md.close()


def test_impulse_path_is_exact(pkg):
    """al = NULL and rx = tx: every phase sum is exactly 0 and sum |r| equals sum |t| bit for bit."""
    md = pkg.Modulator(mode=1, max_frames=1)
    try:
        d = _cuda(DC.block())
        md.dpd_measure_dev(d, d.clone(), None, STATS_PEAK, DC.N_BINS)
        st = md.dpd_stats()
        assert st["samples_used"] == DC.N_SAMPLES - 31 and st["count"].sum() == st["samples_used"] - st["overflow"]
        assert not st["raw"][:, 3].any() and not st["raw"][:, 5].any() and not st["sum_phase"].any()
        assert np.array_equal(st["raw"][:, 2], st["raw"][:, 1]) and st["raw"][:, 1].any()
        assert np.array_equal(st["sum_rx"].view(np.uint64), st["sum_tx"].view(np.uint64))
    finally:
        md.close()


def test_statistics_are_the_same_bits_for_every_tile_and_repetition(pkg):
    md = pkg.Modulator(mode=1, max_frames=1)
    try:
        al = {"lag": -300, "tau": 0.37, "gain": 1.0 / DC.GAIN0}
        d_tx, d_rx = _cuda(DC.block()), _cuda(DC.capture(-300 + 0.37))
        md.dpd_measure_dev(d_tx, d_rx, al, STATS_PEAK, DC.N_BINS)
        first = md.dpd_stats()
        assert first["raw"][:, 3].any()
        for tile in (256, 512, 1280, 2048, 0):
            md.set_dpd_geometry(tile=tile)
            for _ in range(2):
                md.dpd_measure_dev(d_tx, d_rx, al, STATS_PEAK, DC.N_BINS)
                st = md.dpd_stats()
                assert np.array_equal(st["raw"], first["raw"]), tile
                assert st["overflow"] == first["overflow"] and st["samples_used"] == first["samples_used"]
        with pytest.raises(pkg.DabGpuError):
            md.set_dpd_geometry(tile=300)
        with pytest.raises(pkg.DabGpuError):
            md.set_dpd_geometry(tile=4096)
    finally:
        md.close()


def test_accumulating_two_halves_is_one_call_on_the_union(pkg):
    """lag 7: a call on samples [a, b) uses [a + 8, b - 23).  The halves [0, h + 23) and [h - 8, n) use [8, h) and
    [h, n - 23): together what one call on [0, n) uses, so the integer sums are the same bits."""
    md = pkg.Modulator(mode=1, max_frames=1)
    try:
        al = {"lag": 7, "tau": 0.37, "gain": 1.0 / DC.GAIN0}
        n, h = DC.N_SAMPLES, 20011
        x, y = DC.block(), DC.capture(7.37)
        md.dpd_measure_dev(_cuda(x), _cuda(y), al, STATS_PEAK, DC.N_BINS)
        whole = md.dpd_stats()
        md.reset_dpd()
        zero = md.dpd_stats()
        assert zero["n_bins"] == 0 and zero["samples_used"] == 0
        md.dpd_measure_dev(_cuda(x[:h + 23]), _cuda(y[:h + 23]), al, STATS_PEAK, DC.N_BINS, accumulate=True)
        one = md.dpd_stats()
        assert one["samples_used"] == h - 8
        md.dpd_measure_dev(_cuda(x[h - 8:]), _cuda(y[h - 8:]), al, STATS_PEAK, DC.N_BINS, accumulate=True)
        both = md.dpd_stats()
        assert both["samples_used"] == whole["samples_used"] == n - 31 and both["overflow"] == whole["overflow"]
        assert np.array_equal(both["raw"], whole["raw"])
        md.dpd_measure_dev(_cuda(x[:h + 23]), _cuda(y[:h + 23]), al, STATS_PEAK, DC.N_BINS)      # (accumulate 0 starts over)
        assert np.array_equal(md.dpd_stats()["raw"], one["raw"])
    finally:
        md.close()


# --------------------------------------------------------------------------- 3. the closed loop through the library
# the library's coefficients against the model's on the same inputs: four times the worst deviation measured on the device
# (profiles/dpd.txt); without a measured value, what the statistics' bars imply through a fit with cond ~ 1e3
# Measured: 6.67e-6 (cond 482 / 744); residual -36.35 dB -> -51.82 dB, the model loop's -51.82 dB.
C_WORST = 6.67e-6
C_BAR = 1e-2 if C_WORST is None else 4 * C_WORST


def test_closed_loop_through_the_library(pkg):
    """One Mode III frame of cfg 3 chain output, scaled to rms 0.25, as x; align and measure against pa(x) on the device; fit;
    set_poly; the poly stage entry on x; the amplifier model in numpy.  The coefficients against the model's on the same
    inputs, the residual within 0.5 dB of the model loop's and at least 10 dB better than without predistortion."""
    import oracle as O
    md = pkg.Modulator(mode=3, max_frames=1)
    try:
        md.set_gain(pkg.GAIN_VAR, 1.0, 1.0 / 50000.0, 4.0)
        bits = synth_bits(md.geometry["tf_input_bytes"], seed=5).reshape(1, -1)
        x = md.chain(bits, CFG3).reshape(-1).astype(np.complex128)
        x = (x * (0.25 / np.sqrt(np.mean(np.abs(x) ** 2)))).astype(np.complex64)
        y = DC.pa(x).astype(np.complex64)
        before = DC.residual_db(DC.pa(x), x)
        d_x, d_y = _cuda(x), _cuda(y)
        al = md.dpd_align_dev(d_x, d_y)
        assert al["lag"] == 0 and abs(al["tau"]) < 1e-3 and al["coherence"] > 0.99
        peak = float(np.abs(x).max()) * (1.0 + 1e-6)
        md.dpd_measure_dev(d_x, d_y, al, peak, 64)
        st = md.dpd_stats()
        assert st["overflow"] == 0
        am, pm, info = pkg.dpd_fit_poly(st, "magsq", min_count=1, weighted=True)
        # the model loop on the same inputs: the same alignment, the model's statistics and fit, the oracle's predistorter
        mst = DM.stats(x, y, al["lag"], al["tau"], al["gain"], peak, 64, taps=pkg.dpd_delay_taps(al["tau"]))
        assert np.array_equal(st["count"], mst["count"])
        mam, mpm = DM.fit_poly(mst, "magsq", 1, True)
        dev = max(float(np.abs(am - mam).max()), float(np.abs(pm - mpm).max()))
        model_after = DC.residual_db(DC.pa(O.memless_poly(x, mam.astype(np.float32), mpm.astype(np.float32))), x)
        md.set_poly(am, pm)
        after = DC.residual_db(DC.pa(md.poly(x).reshape(-1)), x)
        print("closed loop: %.2f dB -> %.2f dB (model loop %.2f dB); coefficients within %.3g of the model's; cond %.3g / %.3g"
              % (before, after, model_after, dev, info["cond_am"], info["cond_pm"]))
        ok = record_bound("dpd closed loop: coefficients vs the model's", dev, C_BAR)
        assert abs(after - model_after) <= 0.5 and after <= before - 10.0
        assert ok
    finally:
        md.close()


# --------------------------------------------------------------------------- 4. dabmod_file --dpd-feedback
def _dabmod_file(tmp_path, tag, extra, want_rc=0):
    fin = str(tmp_path / "in.eti")
    if not os.path.exists(fin):
        synth_eti(8).tofile(fin)                 # two transmission frames
    fout = str(tmp_path / ("out_" + tag))
    r = subprocess.run([os.path.join(HOST, "dabmod_file"), fin, fout] + extra, capture_output=True, text=True, timeout=300)
    assert r.returncode == want_rc, (r.returncode, r.stderr[-2000:])
    return np.fromfile(fout, np.complex64), r.stderr


def test_dabmod_file_fits_a_polynomial_from_its_own_output(tmp_path):
    """The program's earlier output through the amplifier model, delayed by 5 samples, as the feedback file: it prints lag 5,
    its coefficient file is accepted by --poly, and the second run's output gives the lower residual."""
    plain, _ = _dabmod_file(tmp_path, "plain", ["--fir", "default"])
    rms = float(np.sqrt(np.mean(np.abs(plain.astype(np.complex128)) ** 2)))
    opts = ["--fir", "default", "--gainmode", "var", "--normalise", "%.9g" % (0.25 / rms)]
    x, _ = _dabmod_file(tmp_path, "scaled", opts)
    assert abs(np.sqrt(np.mean(np.abs(x.astype(np.complex128)) ** 2)) - 0.25) < 0.01
    y = DC.pa(x)
    rx = np.concatenate([np.zeros(5, np.complex128), y[:-5]]).astype(np.complex64)
    rx_path, coef = str(tmp_path / "rx.iq"), str(tmp_path / "coef.txt")
    rx.tofile(rx_path)
    again, err = _dabmod_file(tmp_path, "dpd", opts + ["--dpd-feedback", rx_path, "--dpd-out", coef])
    assert np.array_equal(again.view(np.uint8), x.view(np.uint8))
    m = re.search(r"dpd: lag (-?\d+) tau (-?[\d.]+) gain", err)
    assert m and int(m.group(1)) == 5 and abs(float(m.group(2))) < 1e-3, err
    assert re.search(r"dpd: \d+ samples in 64 bins", err), err
    lines = open(coef).read().split()
    assert lines[:2] == ["1", "5"] and len(lines) == 12
    pre, _ = _dabmod_file(tmp_path, "pre", opts + ["--poly", coef])
    before, after = DC.residual_db(DC.pa(x), x), DC.residual_db(DC.pa(pre), x)
    print("dabmod_file: residual %.2f dB -> %.2f dB" % (before, after))
    assert after <= before - 10.0
    # refusals of the option
    for extra, text in ((["--dpd-feedback", rx_path], "go together"), (["--dpd-feedback", rx_path, "--dpd-out", coef, "--format", "u8"], "u8 / s8"),
                        (["--dpd-feedback", rx_path, "--dpd-out", coef, "--batch", "2", "--contexts", "2"], "--contexts above 1")):
        r = subprocess.run([os.path.join(HOST, "dabmod_file"), str(tmp_path / "in.eti"), str(tmp_path / "x")] + extra,
                           capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and text in r.stderr, (extra, r.stderr)
    # a feedback file that spans too few amplitudes: the fit is refused, exit status 4
    (0.01 * rx).astype(np.complex64)[:4096].tofile(rx_path)
    r = subprocess.run([os.path.join(HOST, "dabmod_file"), str(tmp_path / "in.eti"), str(tmp_path / "x")] + opts +
                       ["--dpd-feedback", rx_path, "--dpd-out", coef, "--dpd-min-count", "100000"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 4 and "the fit is refused" in r.stderr, r.stderr


# --------------------------------------------------------------------------- 5. refusals, each before anything is queued
def test_refusals(pkg):
    import torch
    md = pkg.Modulator(mode=1, max_frames=1)
    try:
        d = torch.zeros(4096, dtype=torch.complex64, device="cuda")
        lib, h, p = md._lib, md._h, d.data_ptr()
        al = pkg._DpdAlignment(1001, 0.0, 1.0, 0.0, 1.0)
        import ctypes as C
        cases = (((p, 0, p, 4096, None, 1.0, 0, 0), "n_bins is 1"), ((p, 0, p, 4096, None, 1.0, 257, 0), "n_bins is 1"),
                 ((p, 0, p, 4096, None, 0.0, 64, 0), "peak must be positive"), ((p, 0, p, 4096, None, -1.0, 64, 0), "peak must be positive"),
                 ((p, 0, p, 4096, None, float("inf"), 64, 0), "peak must be positive"),
                 ((p, 0, p, 2 ** 31 + 1, None, 1.0, 64, 0), "at most 2^31 samples"),
                 ((p, 0, p, 4096, C.byref(al), 1.0, 64, 0), "DABGPU_DPD_MAX_LAG"),
                 ((p, 2, p, 4096, None, 1.0, 64, 0), "tx is complexf"), ((p + 4, 0, p, 4096, None, 1.0, 64, 0), "aligned"),
                 ((None, 0, p, 4096, None, 1.0, 64, 0), "null argument"))
        for args, text in cases:
            assert lib.dabgpu_dpd_measure_dev(h, *args, None) == -1, args
            assert text in lib.dabgpu_last_error(h).decode(), (args, lib.dabgpu_last_error(h).decode())
        st = md.dpd_stats()
        assert st["samples_used"] == 0 and st["n_bins"] == 0
        # a changed peak or n_bins while accumulating; the cap while accumulating
        md.dpd_measure_dev(d, d, None, 1.0, 64, accumulate=True)
        for peak, bins in ((2.0, 64), (1.0, 32)):
            with pytest.raises(pkg.DabGpuError) as e:
                md.dpd_measure_dev(d, d, None, peak, bins, accumulate=True)
            assert "another peak or n_bins" in str(e.value)
        assert lib.dabgpu_dpd_measure_dev(h, p, 0, p, 2 ** 31 - 4095, None, 1.0, 64, 1, None) == -1      # (4096 held + this = 2^31 + 1)
        assert "at most 2^31 samples" in lib.dabgpu_last_error(h).decode()
        assert md.dpd_stats()["samples_used"] == 4096 - 31
        md.dpd_measure_dev(d, d, None, 2.0, 32)                     # (accumulate 0: any peak)
        assert md.dpd_stats()["peak"] == 2.0
        # alignment: a lag beyond +-1000 is refused with a message
        x = DC.block()
        with pytest.raises(pkg.DabGpuError) as e:
            md.dpd_align_dev(_cuda(x), _cuda(DC.capture(1020.6)))
        assert "DABGPU_DPD_MAX_LAG" in str(e.value)
        with pytest.raises(pkg.DabGpuError) as e:
            md.dpd_align_dev(_cuda(x[:2047]), _cuda(x[:2047]))
        assert "2048 samples" in str(e.value)
        assert lib.dabgpu_dpd_xspectrum_dev(h, p, 3, p, 4096, 0, None) == -1 and "tx is complexf" in lib.dabgpu_last_error(h).decode()
        with pytest.raises(pkg.DabGpuError):
            md.dpd_measure_dev(d, torch.zeros(4096, dtype=torch.int16, device="cuda"))
    finally:
        md.close()


# --------------------------------------------------------------------------- 6. the launch trace
def test_trace_names_the_launches_and_chain_calls_are_untouched(pkg):
    md = pkg.Modulator(mode=1, max_frames=1)
    try:
        md.set_gain(pkg.GAIN_VAR, 1.0, 1.0 / 50000.0, 4.0)
        bits = synth_bits(md.geometry["tf_input_bytes"], seed=3).reshape(1, -1)
        md.trace(True)
        before = md.chain(bits, CFG3).copy()
        chain_trace = md.last_variant()
        assert chain_trace and not any("dpd" in k for k in chain_trace)
        d_tx, d_rx = _cuda(DC.block()), _cuda(DC.capture(7.37))
        md.dpd_xspectrum_dev(d_tx, d_rx, 7)
        assert md.last_variant() == ["dpd_xspectrum_kernel<0>", "dpd_xspectrum_reduce_kernel"]
        md.dpd_xspectrum_dev(_cuda(DC.block_s16()), d_rx, 7)
        assert md.last_variant() == ["dpd_xspectrum_kernel<1>", "dpd_xspectrum_reduce_kernel"]
        al = md.dpd_align_dev(d_tx, d_rx)
        assert md.last_variant() == ["dpd_xspectrum_kernel<0>", "dpd_xspectrum_reduce_kernel"] * 2 and al["lag"] == 7
        md.dpd_measure_dev(d_tx, d_rx, al, STATS_PEAK, DC.N_BINS)
        assert md.last_variant() == ["dpd_stats_kernel<0>"]
        md.dpd_measure_dev(_cuda(DC.block_s16()), d_rx, al, STATS_PEAK * DC.S16_SCALE, DC.N_BINS)
        assert md.last_variant() == ["dpd_stats_kernel<1>"]
        md.dpd_measure_dev(d_tx[:20], d_rx[:20], al, STATS_PEAK * DC.S16_SCALE, DC.N_BINS)     # (no sample has its taps: no launch)
        assert md.last_variant() == []
        after = md.chain(bits, CFG3)
        assert md.last_variant() == chain_trace
        assert np.array_equal(after.view(np.uint8), before.view(np.uint8))
    finally:
        md.close()
