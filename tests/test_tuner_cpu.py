"""The tuner without a device (include/dabgpu.h, "the tuner"): the host-only entries -- ratio and tap count,
the rows of the tap table against the formula, the filters' responses, the output counts -- and the float64 model
(tests/tuner_model.py) at the operating points tests/test_tuner_gpu.py repeats on the device: a resampled capture, with and
without interferers, through the model and the receiver's models."""
import os
import re

import numpy as np
import pytest

from tests import tuner_cases as TC
from tests import tuner_model as TM
from tests.conftest import ROOT, load_pkg, record_bound

ENTRIES = ["dabgpu_tuner_check", "dabgpu_tuner_geometry", "dabgpu_tuner_taps", "dabgpu_tuner_count", "dabgpu_tuner_out_max",
           "dabgpu_set_tuner", "dabgpu_tuner_reset", "dabgpu_get_tuner_position", "dabgpu_tuner_dev", "dabgpu_tuner",
           "dabgpu_debug_tuner_run_samples"]


@pytest.fixture(scope="module")
def pkg():
    p = load_pkg()
    if not os.path.exists(p.LIB_PATH):
        p.build()
    return p


def test_entries_are_declared_exported_and_wrapped(pkg):
    text = open(os.path.join(ROOT, "include", "dabgpu.h")).read()
    lib = pkg.load_library()
    for name in ENTRIES:
        assert re.search(r"DABGPU_API\s+\w+\s+%s\(" % name, text), name
        assert name in pkg.EXPORTS and hasattr(lib, name), name
    for words in ("q = m M, i_m = q div L, p = q mod L", "for j = 0, 1, ... P - 1 in this order", "a time-varying offset"):
        assert words in text, words
    for m in ("set_tuner", "tuner_reset", "tuner_position", "tuner", "tuner_dev"):
        assert callable(getattr(pkg.Modulator, m)), m
    for f in ("tuner_geometry", "tuner_taps", "tuner_count", "tuner_out_max"):
        assert callable(getattr(pkg, f)), f


# --------------------------------------------------------------------------- 1. geometry
def test_geometry_of_the_listed_rates_and_the_refusals(pkg):
    for rate, (L, M) in TC.LISTED.items():
        for sel in (0, 1):
            assert pkg.tuner_geometry(rate, sel) == (L, M, TC.taps_per_output(rate, sel)) == TM.geometry(rate, sel), (rate, sel)
            assert TC.taps_per_output(rate, sel) <= TM.MAX_TAPS and L <= TM.MAX_L
            pkg.tuner_check(rate, sel, rate / 4.0 - 1.0)
            pkg.tuner_check(rate, sel, -(rate / 4.0 - 1.0))
    for (rate, sel, off), words in TC.REFUSED:
        with pytest.raises(pkg.DabGpuError, match=re.escape(words)):
            pkg.tuner_check(rate, sel, off)
        with pytest.raises(pkg.DabGpuError, match=re.escape(words)):
            pkg.tuner_geometry(rate, sel, off)
        if np.isfinite(off) and abs(off) < rate / 4.0:
            assert TM.geometry(rate, sel) is None
    lib = pkg.load_library()
    assert lib.dabgpu_tuner_check(None) != 0 and b"null argument" in lib.dabgpu_last_error(None)


# --------------------------------------------------------------------------- 2. taps
def test_rows_are_the_formulas_fp32_bits_and_ratio_1_wide_is_the_unit_impulse(pkg):
    for rate, (L, M) in TC.LISTED.items():
        for sel in (0, 1):
            for p in sorted({0, 1 % L, L // 2, L - 1}):
                got = pkg.tuner_taps(rate, sel, p)
                want = TM.formula_taps(rate, sel, p).astype(np.float32)
                assert got.dtype == np.float32 and got.shape == want.shape
                assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (rate, sel, p)
            for bad in (-1, L):
                with pytest.raises(pkg.DabGpuError, match="rows are 0 ... L - 1"):
                    pkg.tuner_taps(rate, sel, bad)
    impulse = np.zeros(32, np.float32)
    impulse[15] = 1.0
    assert np.array_equal(pkg.tuner_taps(2048000, 0, 0).view(np.uint32), impulse.view(np.uint32))


# --------------------------------------------------------------------------- 3. response
def _phases(L):
    return sorted({0, 1 % L, L // 4, L // 2, (3 * L) // 4, L - 1})


@pytest.mark.parametrize("sel", [0, 1], ids=["wide", "channel"])
def test_pass_band_and_stop_band_of_the_returned_taps(pkg, sel):
    """From the returned fp32 taps, in float64, per sampled row with its own fractional delay taken off: |H - 1| <= 2e-5 up to
    768 kHz; |H| <= -95 dB from 1280 kHz (wide) / 944 kHz (channel) up to in_rate / 2, wherever that band exists.  Measured
    when written: 1.2e-5 and -99 dB worst; the bars leave a factor below 2, and 4 dB, for the sampling of phases and
    frequencies."""
    worst_pass = worst_stop = 0.0
    for rate, (L, M) in TC.LISTED.items():
        if rate == 2048000 and sel == 0:
            continue                                # (the unit impulse: no filter)
        pass_f = np.linspace(-768e3, 768e3, 193)
        edge = 1280e3 if sel == 0 else 944e3
        stop_f = np.arange(edge, rate / 2.0 + 1.0, 4e3)
        for p in _phases(L):
            row = pkg.tuner_taps(rate, sel, p)
            worst_pass = max(worst_pass, float(np.abs(TM.response(row, L, pass_f, rate, p) - 1.0).max()))
            if stop_f.size:
                both = np.concatenate([stop_f, -stop_f])
                worst_stop = max(worst_stop, float(np.abs(TM.response(row, L, both, rate, p)).max()))
    stop_db = 20.0 * np.log10(worst_stop)
    print("%s: pass band off 1 by %.3g at most, stop band %.1f dB at most" % (("wide", "channel")[sel], worst_pass, stop_db))
    assert record_bound("tuner pass band |H - 1|, %s" % ("wide", "channel")[sel], worst_pass, 2e-5)
    assert record_bound("tuner stop band |H|, %s" % ("wide", "channel")[sel], worst_stop, 10.0 ** (-95.0 / 20.0))


# --------------------------------------------------------------------------- 4. counts
@pytest.mark.parametrize("rate", [2400000, 8192000, 10000000])
def test_count_is_the_brute_force_count_and_out_max_bounds_every_call(pkg, rate):
    for sel in (0, 1):
        L, M, P = pkg.tuner_geometry(rate, sel)
        counts = []
        for T in range(3 * P + 1):
            brute, m = 0, 0
            while (m * M) // L + P // 2 <= T - 1:
                brute += 1
                m += 1
            assert pkg.tuner_count(rate, sel, T) == brute == TM.count(L, M, P, T), (sel, T)
            counts.append(brute)
        assert counts[P // 2] == 0 and counts[P // 2 + 1] == 1
        for n in (1, 2, 7, P // 2, P, 2 * P):
            room = pkg.tuner_out_max(rate, sel, n)
            assert room == -(-n * L // M) + 1
            assert max(counts[T + n] - counts[T] for T in range(3 * P + 1 - n)) <= room
        for T in (2 ** 32 - 1000, 2 ** 40 + 77, 2 ** 50):
            assert pkg.tuner_count(rate, sel, T) == -(-(T - P // 2) * L // M) == TM.count(L, M, P, T)
        with pytest.raises(pkg.DabGpuError, match="position must not exceed 2\\^50"):
            pkg.tuner_count(rate, sel, 2 ** 50 + 1)
    assert pkg.load_library().dabgpu_tuner_out_max(None, 100) == 0


# --------------------------------------------------------------------------- 5. the model's operating points
def _receive(pkg, rate, sel, offset, stream):
    x, mode, bits, early = TC.capture()
    y, _ = TM.run(pkg, rate, sel, offset, stream)
    return TM.receive(y, mode, early, bits)


@pytest.mark.parametrize("rate", TC.OPERATING_POINTS["clean"][0])
def test_clean_resampled_capture_comes_back(pkg, rate):
    r = _receive(pkg, rate, 0, 0.0, TC.resampled(rate))
    print("clean %d: starts %s shifts %s bit errors %s MER %.2f dB" % (rate, r["starts"], r["shifts"], r["bit_errors"], r["mer_db"]))
    assert r["starts"] == TC.EXPECTED_STARTS and r["shifts"] == [0, 0] and r["valid"] == [1, 1] and r["bit_errors"] == [0, 0]
    assert abs(r["mer_db"] - 66.5) <= 0.1


@pytest.mark.parametrize("rate", TC.OPERATING_POINTS["near_tones"][0])
def test_near_tones_need_the_channel_setting(pkg, rate):
    x = TC.with_tones(rate, TC.NEAR_TONES)
    r = _receive(pkg, rate, 1, 0.0, x)
    print("near tones %d channel: starts %s bit errors %s MER %.2f dB" % (rate, r["starts"], r["bit_errors"], r["mer_db"]))
    assert r["starts"] == TC.EXPECTED_STARTS and r["valid"] == [1, 1] and r["bit_errors"] == [0, 0]
    assert 66.3 <= r["mer_db"] <= 66.6
    w = _receive(pkg, rate, 0, 0.0, x)              # the same input through the wide setting does not even synchronise
    print("near tones %d wide: starts %s bit errors %s" % (rate, w["starts"], w["bit_errors"]))
    assert w["starts"] != TC.EXPECTED_STARTS and min(w["bit_errors"]) >= 10000


def test_far_tones_need_the_filter(pkg):
    x, mode, bits, early = TC.capture()
    y = TC.with_tones(8192000, TC.FAR_TONES)
    r = _receive(pkg, 8192000, 0, 0.0, y)
    print("far tones wide: starts %s bit errors %s MER %.2f dB" % (r["starts"], r["bit_errors"], r["mer_db"]))
    assert r["starts"] == TC.EXPECTED_STARTS and r["valid"] == [1, 1] and r["bit_errors"] == [0, 0]
    assert abs(r["mer_db"] - 65.5) <= 0.1
    # without a filter: every fourth sample, and the mean of four, of the same input
    for name, plain in (("every fourth sample", y[::4]), ("the mean of four", y[:y.size // 4 * 4].reshape(-1, 4).mean(axis=1))):
        w = TM.receive(plain, mode, early, bits)
        print("far tones, %s: bit errors %s" % (name, w["bit_errors"]))
        assert min(w["bit_errors"]) >= 10000, name


def test_two_blocks_in_one_capture_are_both_received(pkg):
    y = TC.second_block(TC.resampled(8192000))
    a = _receive(pkg, 8192000, 1, 0.0, y)
    b = _receive(pkg, 8192000, 1, TC.SECOND_BLOCK_HZ, y)
    print("two blocks: starts %s / %s, bit errors %s / %s, MER %.2f / %.2f dB"
          % (a["starts"], b["starts"], a["bit_errors"], b["bit_errors"], a["mer_db"], b["mer_db"]))
    assert a["starts"] == TC.EXPECTED_STARTS and b["starts"] == TC.SECOND_BLOCK_STARTS
    for r in (a, b):
        assert r["shifts"] == [0, 0] and r["valid"] == [1, 1] and r["bit_errors"] == [0, 0]
    assert abs(b["mer_db"] - 40.8) <= 0.1 and abs(a["mer_db"] - 41.0) <= 0.2      # (set by the unfiltered neighbour's side lobes)


# --------------------------------------------------------------------------- the model against itself
def test_model_chunking_positions_and_the_mixer(pkg):
    """the model's own stream state: any chunking gives one call's outputs; a tone at +offset comes out at 0 Hz"""
    x = TC.signal(3000, 11)
    whole, counts = TM.run(pkg, 2400000, 1, 100000.0, x, position=2 ** 40)
    parts, _ = TM.run(pkg, 2400000, 1, 100000.0, x, [1, 95, 96, 97, 191, 192, 193, 3000 - 865], position=2 ** 40)
    assert np.allclose(parts, whole, rtol=0, atol=1e-12) and counts == [pkg.tuner_count(2400000, 1, 2 ** 40 + 3000) - pkg.tuner_count(2400000, 1, 2 ** 40)]
    k = np.arange(4000)
    tone = np.exp(2j * np.pi * 300e3 / 8192000 * k).astype(np.complex64)
    y, _ = TM.run(pkg, 8192000, 1, 300e3, tone)
    settled = y[200:y.size - 10]
    assert np.abs(settled - settled[0]).max() < 1e-4 and abs(abs(settled[0]) - 1.0) < 1e-4
