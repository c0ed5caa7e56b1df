"""The clock without a device: the tap table is the header's formula, the output counts are the definition's for a few thousand
(ppm, T) pairs, the float64 model (tests/clock_model.py, written from include/dabgpu.h) is the same stream however it is cut,
the refusals of the setting are host code alone, and what the definition itself costs a DAB signal is measured."""
import os
import re

import numpy as np
import pytest

from tests import clock_cases as KC
from tests import clock_model as KM
from tests.conftest import ROOT, load_pkg

ENTRIES = ["dabgpu_clock_check", "dabgpu_clock_step", "dabgpu_clock_count", "dabgpu_clock_phase_taps", "dabgpu_set_clock",
           "dabgpu_clock_reset", "dabgpu_get_clock_position", "dabgpu_clock_dev", "dabgpu_clock", "dabgpu_debug_clock_run_samples"]


@pytest.fixture(scope="module")
def pkg():
    p = load_pkg()
    p.build()
    return p


def test_header_library_and_exports_are_in_step(pkg):
    text = open(os.path.join(ROOT, "include", "dabgpu.h")).read()
    lib = pkg.load_library()
    for name in ENTRIES:
        assert re.search(r"DABGPU_API int %s\(" % name, text), name
        assert name in pkg.EXPORTS and hasattr(lib, name) and not name.endswith("_process"), name
    assert re.search(r"DABGPU_API size_t dabgpu_clock_out_max\(", text) and re.search(r"DABGPU_API double dabgpu_clock_inverse_ppm\(", text)
    for define, value in (("TAPS", KM.TAPS), ("PHASES", KM.PHASES), ("HISTORY", KM.HISTORY)):
        assert "#define DABGPU_CLOCK_%s %d" % (define, value) in text
    for words in ("step = llrint(ppm 1e-6 2^64)", "for j = 0, 1, ... 31 in this order", "a time-varying offset"):
        assert words in text, words
    for m in ("set_clock", "clock_reset", "clock_position", "clock", "clock_dev"):
        assert callable(getattr(pkg.Modulator, m)), m
    for f in ("clock_check", "clock_step", "clock_count", "clock_out_max", "clock_phase_taps", "clock_inverse_ppm"):
        assert callable(getattr(pkg, f)), f


# --------------------------------------------------------------------------- 1. the table
def test_table_rows_are_the_formula_and_the_end_rows_are_unit_impulses(pkg):
    t = KM.table(pkg)
    want = np.stack([KM.formula_taps(p / 512.0) for p in range(513)])
    dev = float(np.abs(t.astype(np.float64) - want).max())
    print("largest |table - formula|: %.3g" % dev)
    assert dev <= 1e-7
    for row, tap in ((0, 15), (512, 16)):
        impulse = np.zeros(32, np.float32)
        impulse[tap] = 1.0
        assert np.array_equal(t[row].view(np.uint32), impulse.view(np.uint32)), row
    for p in range(0, 513, 64):                       # the rows are dabgpu_dpd_delay_taps', bit for bit, where that is defined
        if p < 512:
            assert np.array_equal(t[p], pkg.dpd_delay_taps(p / 512.0))
    for bad in (-1, 513):
        with pytest.raises(pkg.DabGpuError, match="rows are 0 ... 512"):
            pkg.clock_phase_taps(bad)


# --------------------------------------------------------------------------- 2. step and counts
def test_step_is_the_rounded_product(pkg):
    for ppm in (0.0, 1e-3, -1e-3, 20.0, -20.0, 37.5, 999.999, 1000.0, -1000.0):
        step = pkg.clock_step(ppm)
        assert step == int(np.rint(np.float64(ppm) * np.float64(1e-6) * np.float64(2.0 ** 64))), ppm
        assert abs(step) <= 18446744073709552
    assert pkg.clock_step(0.0) == 0 and pkg.clock_step(-20.0) == -pkg.clock_step(20.0)
    assert abs(pkg.clock_inverse_ppm(37.5) + 37.5 / (1.0 + 37.5e-6)) < 1e-12 and pkg.clock_inverse_ppm(0.0) == 0.0
    d, e = 37.5e-6, pkg.clock_inverse_ppm(37.5) * 1e-6
    assert abs((1.0 + d) * (1.0 + e) - 1.0) < 1e-15


def _pairs():
    rs = np.random.RandomState(11)
    ppms = [1000.0, -1000.0, 1e-3, -1e-3, 0.0, 20.0, -20.0] + list(rs.uniform(-1000.0, 1000.0, 13))
    Ts = list(range(0, 41)) + [2 ** 32 + k for k in range(-40, 41)] + [2 ** 40 + k for k in range(-40, 1)]
    Ts += [int(v) for v in rs.randint(0, 2 ** 31, 20)] + [int(v) << 9 for v in rs.randint(0, 2 ** 31, 20)]
    return [(p, T) for p in ppms for T in Ts]


def test_counts_equal_the_big_integer_count_and_add_up(pkg):
    pairs = _pairs()
    assert len(pairs) >= 3000
    for ppm, T in pairs:
        step = pkg.clock_step(ppm)
        assert pkg.clock_count(ppm, T) == KM.count(step, T), (ppm, T)
    for ppm in (1000.0, -1000.0, 1e-3, 0.0, -333.3):
        m = [pkg.clock_count(ppm, T) for T in range(0, 3000)]
        assert m[16] == 0 and m[17] in (1, 2) and all(0 <= b - a <= 2 for a, b in zip(m, m[1:])), ppm
        assert pkg.clock_count(ppm, 2 ** 40) >= pkg.clock_count(ppm, 2 ** 40 - 1) >= pkg.clock_count(ppm, 2 ** 32)
        # a stream cut anywhere: the counts of the calls sum to the count of the whole, and no call exceeds clock_out_max
        rs = np.random.RandomState(5)
        for base in (0, 2 ** 32 - 1000, 2 ** 40 - 50000):
            cuts = [0] + sorted(int(v) for v in rs.randint(0, 50000, 40)) + [50000]
            counts = [pkg.clock_count(ppm, base + b) - pkg.clock_count(ppm, base + a) for a, b in zip(cuts, cuts[1:])]
            assert sum(counts) == pkg.clock_count(ppm, base + 50000) - pkg.clock_count(ppm, base)
            assert all(c <= pkg.clock_out_max(b - a) for c, a, b in zip(counts, cuts, cuts[1:]))
    assert pkg.clock_count(0.0, 12345) == 12345 - 16
    assert pkg.clock_out_max(1) >= 2 and pkg.clock_out_max(2 ** 40) >= pkg.clock_count(-1000.0, 2 ** 40)


# --------------------------------------------------------------------------- 3. the model is one stream
def test_model_chunked_equals_unchunked_identity_and_reset(pkg):
    x = KC.signal(KC.N_STREAM, 2)
    q = KC.signal(KC.N_STREAM, 3, s16=True)
    for ppm in KC.STREAM_PPM:
        step = pkg.clock_step(ppm)
        whole, counts = KM.run(pkg, ppm, x)
        assert counts == [KM.count(step, KC.N_STREAM)] and np.abs(whole).min() > 0
        assert len(KC.slips(step, 1, whole.size)) in (19, 20, 21)
        for name, lengths in KC.splits(step).items():
            got, counts = KM.run(pkg, ppm, x, lengths)
            assert np.array_equal(got, whole), (ppm, name)
            assert sum(counts) == whole.size
        want, _ = KM.run(pkg, ppm, q)
        got, _ = KM.run(pkg, ppm, KM.as_samples(q).astype(np.complex64), KC.splits(step)["sevens"])
        assert np.array_equal(got, want)
        # a reset at P = the tail of a run from 0 whose input is zeros up to P
        P = 5000
        padded, _ = KM.run(pkg, ppm, np.concatenate([np.zeros(P, np.complex64), x]))
        tail, _ = KM.run(pkg, ppm, x, position=P)
        assert np.array_equal(tail, padded[KM.count(step, P):])
    same, _ = KM.run(pkg, 0.0, x)
    assert np.array_equal(same, x[:KC.N_STREAM - 16].astype(np.complex128))


# --------------------------------------------------------------------------- 4. the refusals of the setting, host code alone
@pytest.mark.parametrize("ppm,words", [(float("nan"), "ppm must be finite"), (float("inf"), "ppm must be finite"),
                                       (-float("inf"), "ppm must be finite"), (1000.0001, r"\|ppm\| must not exceed 1000"),
                                       (-1e9, r"\|ppm\| must not exceed 1000")])
def test_refusals_of_the_setting(pkg, ppm, words):
    for fn in (pkg.clock_check, pkg.clock_step, lambda p: pkg.clock_count(p, 100)):
        with pytest.raises(pkg.DabGpuError, match="clock: " + words):
            fn(ppm)


def test_what_is_allowed_passes_and_a_position_beyond_2_62_does_not(pkg):
    for ppm in (0.0, 1000.0, -1000.0, 1e-3):
        pkg.clock_check(ppm)
    assert pkg.clock_count(20.0, 2 ** 62) > 2 ** 61
    with pytest.raises(pkg.DabGpuError, match="position must not exceed 2\\^62"):
        pkg.clock_count(20.0, 2 ** 62 + 1)


# --------------------------------------------------------------------------- 5. what the definition costs a DAB signal
def test_fidelity_of_the_definition_on_a_mode_ii_signal(pkg):
    """Properties of the definition, not of a kernel, as relative RMS over a Mode II signal (null symbol left out): the
    table's 512 phases and linear blend against the formula at mu itself, and +37.5 ppm followed by its inverse against the
    input.  Measured: blend 8.7e-7; round trip 1.05e-5 on the filtered signal (cfg 3: GainControl and FIRFilter) and 5.6e-3
    on the unfiltered one (no stages), whose rectangular symbols leak past 0.85 of Nyquist, where the interpolator is not
    flat: that part of the signal does not come back (1.9e-4 of it inside the occupied carriers).  Held: the blend and the
    filtered round trip, to the interpolator's worst error against exact tones inside DAB's band (8.1e-6 with the blend;
    the blend is a share of it, the round trip passes through it twice).  The unfiltered figure is recorded only."""
    import oracle as O
    from tests import demod_cases as DC
    from tests.sync_cases import case_bits
    from tests.sync_model import geometry
    g = geometry(2)
    ppm = 37.5
    figures = {}
    for name, stages, kw in (("unfiltered", 0, {}), ("cfg3", DC.GAIN | DC.FIR, dict(gain_mode=2, normalise=DC.NORMALISE))):
        y = np.asarray(O.Chain(mode=2, stages=stages, **kw).process(case_bits(2, 1))).reshape(-1)
        y = y[g["null"]:g["null"] + 30000].astype(np.complex64)
        table, _ = KM.run(pkg, ppm, y)
        if name == "cfg3":
            exact, _ = KM.run(pkg, ppm, y, exact_taps=True)
            figures["blend"] = float(np.sqrt(np.mean(np.abs(table - exact) ** 2) / np.mean(np.abs(exact) ** 2)))
        back, _ = KM.run(pkg, pkg.clock_inverse_ppm(ppm), table)
        ref = y[:back.size].astype(np.complex128)
        figures[name] = float(np.sqrt(np.mean(np.abs(back - ref)[64:] ** 2) / np.mean(np.abs(ref[64:]) ** 2)))
    print("table against exact taps: %(blend).3g; +37.5 ppm and its inverse against the input: %(cfg3).3g filtered, "
          "%(unfiltered).3g unfiltered" % figures)
    assert figures["blend"] <= 8.1e-6 and figures["cfg3"] <= 2 * 8.1e-6


# --------------------------------------------------------------------------- 6. the operating points of the GPU loop test
def test_estimator_entries_are_declared(pkg):
    text = open(os.path.join(ROOT, "include", "dabgpu.h")).read()
    lib = pkg.load_library()
    for name in ("dabgpu_sco_dev", "dabgpu_sco", "dabgpu_get_sco"):
        assert re.search(r"DABGPU_API int %s\(" % name, text) and name in pkg.EXPORTS and hasattr(lib, name), name
    st = re.search(r"typedef struct dabgpu_sco_frame \{(.*?)\}", text, re.S).group(1)
    for field in ("a_hi_re", "a_hi_im", "a_lo_re", "a_lo_im", "s;", "ppm", "residual_cfo", "quality", "valid"):
        assert field in st, field
    import ctypes as C
    assert C.sizeof(pkg._ScoFrame) == 72
    for m in ("sco", "sco_dev", "sco_result"):
        assert callable(getattr(pkg.Modulator, m)), m
    for words in ("second order", "pi/4", "since built"):
        assert words in text, words


def test_estimator_model_reads_a_pure_rotation_exactly():
    """carriers of equal amplitude turned by 2 pi k delta sym / N: the estimate is delta, the residual offset the common turn"""
    from tests.receiver import MODES
    N, K, nsym, null, sym = MODES[2]
    rs = np.random.RandomState(3)
    k = np.concatenate([np.arange(1, K // 2 + 1), np.arange(-K // 2, 0)])
    for ppm, cfo in ((50.0, 0.0), (-200.0, 0.01), (0.0, -0.02)):
        d = np.exp(1j * (np.pi / 4 + np.pi / 2 * rs.randint(0, 4, (nsym - 1, K))))
        d = d * np.exp(2j * np.pi * (k * ppm * 1e-6 + cfo) * sym / N)
        c = ((1.0 - 2.0 * (d.real < 0)) + 1j * (1.0 - 2.0 * (d.imag < 0))) / np.sqrt(2.0)
        e = d * np.conj(c)
        fig = KM.sco_figures(e[:, :K // 2].sum(), e[:, K // 2:].sum(), np.abs(e).sum(), 2)
        assert abs(fig["ppm"] - ppm) < 1e-9 * max(1.0, abs(ppm)) + 1e-3 * abs(ppm) and fig["valid"] == 1
        assert abs(fig["residual_cfo"] - cfo) < 1e-4 and 0.9 < fig["quality"] <= 1.0
    assert KM.sco_figures(0.0, 0.0, 0.0, 2) == dict(a_hi=0j, a_lo=0j, s=0.0, ppm=0.0, residual_cfo=0.0, quality=0.0, valid=0)


@pytest.mark.parametrize("name", list(KC.LOOP_CASES))
def test_operating_points_of_the_loop_on_the_models(pkg, name):
    """channel -> clock(+p) -> sync -> extract -> sco, then clock(inverse of the estimate) on that capture -> sync -> extract
    -> demod and sco, all on the models: the estimate within max(0.5 ppm, 1 % of |p|) of p, the second estimate within
    0.5 ppm, no bit error after the correction, every frame found and valid.  Measured (estimate / second estimate, ppm):
    m2_p20 19.927 / -0.001, m2_p100 99.908 / 0.018, m2_m100 -100.065 / -0.008, m2_p100_echo 100.190 / -0.166,
    m1_p20 19.924 / 0.073; sum_quadrature / sum_signal falls from 4.0e-3 ... 1.2e-2 to 3.7e-3 ... 4.6e-3 (the noise's).
    tests/clock_cases.py says which cases were tried before these."""
    from tests import channel_model as CM
    x, mode, bits, early, ppm, (paths, sigma, seed) = KC.loop_case(name, pkg.channel_sigma)
    r = KM.loop_model(pkg, x, mode, ppm, early, bits, CM.Channel(paths, sigma, seed))
    for k in ("first", "second"):
        p = r[k]
        print("%s %s: starts %s shifts %s bit errors %s, sum_quadrature / sum_signal %.4g, estimate %.4f ppm"
              % (name, k, p["starts"], p["shifts"], p["bit_errors"], p["ratio"], p["estimate"]))
        assert p["valid"] == [1, 1] and len(p["starts"]) == 2
    assert abs(r["first"]["estimate"] - ppm) <= max(0.5, 0.01 * abs(ppm))
    assert abs(r["second"]["estimate"]) <= 0.5
    assert r["second"]["bit_errors"] == [0, 0]
    assert r["second"]["ratio"] < r["first"]["ratio"]
    # the margins of the synchroniser's integer decisions, tests/test_sync_cpu.py's bars: the device reproduces them
    for k in ("first", "second"):
        s = r[k]["sync"]
        assert s["s_second"] >= 1.5 * s["s_lowest"], (k, s["s_second"], s["s_lowest"])
        assert all(m["d_runner_up"] <= 0.5 and m["c_runner_up"] <= 0.5 for m in s["margins"]), k
