"""The TII analyser without a device: the float64 model (tests/tii_scan_model.py) reads every case the GPU tests assert equal
integers on (tests/tii_scan_cases.py, built from the oracle's chains) as expected, with every integer decision far from going
the other way; the pattern table and the cells against the oracle's TII carrier sets for all 70 patterns -- Mode I reads as
configured, Mode II as the pattern with its halves exchanged --; and the settings' refusals, which are host
code alone."""
import os
import re

import numpy as np
import pytest

from tests import tii_scan_cases as TC
from tests.conftest import ROOT, load_pkg
from tests.sync_model import geometry, phase_reference_bins
from tests.tii_scan_model import PATTERNS, exchanged, tii_scan_model

ENTRIES = ["dabgpu_tii_scan_dev", "dabgpu_tii_scan", "dabgpu_get_tii_scan", "dabgpu_tii_scan_check"]
GAP = {1: 16.0, 2: 4.0}                            # |delay_coarse - delay| at most, in samples


def _conditions(name, r, mode):
    """Every decision of the result r is far from going the other way; -> the figures, for the log."""
    E, on, thr = r["E"], r["on"], r["thr"]
    weakest = float(E[on].min() / thr) if on.any() else float("inf")
    strongest = float(E[~on].max() / thr) if thr > 0 else 0.0
    gap = max([abs(e["delay_coarse"] - e["delay"]) for e in r["entries"]] + [0.0])
    runner = max([e["runner_up"] for e in r["entries"]] + [0.0])
    print("%s: weakest set cell %.3g x thr, strongest unset %.3g x thr, coarse-to-fine %.3g samples, runner-up %.3g"
          % (name, weakest, strongest, gap, runner))
    assert weakest >= 2.0 and strongest <= 0.5, (name, weakest, strongest)
    assert gap <= GAP[mode], (name, gap)
    assert runner <= 0.5, (name, runner)


def _expected(name, r):
    want, parity = TC.EXPECT[name]
    assert r["n_entries"] == len(want), (name, r["entries"])
    if parity is not None:
        assert r["parity"] == parity
    for e, (comb, pattern, delay) in zip(r["entries"], want):
        assert (e["comb"], e["pattern"], e["n_set"], e["mask"]) == (comb, pattern, 4, PATTERNS[pattern]), (name, e)
        assert e["delay"] == delay, (name, e)
    if name in TC.TWO_CASES:
        level = 10.0 * np.log10(r["entries"][0]["energy"] / r["entries"][1]["energy"])
        print("%s: level difference %.2f dB" % (name, level))
        assert abs(level - TC.LEVEL_DB) <= TC.LEVEL_TOL_DB, (name, level)


@pytest.mark.parametrize("name", sorted(TC.CASES))
def test_model_reads_every_case_as_expected_with_margin(name):
    x, mode, early, old = TC.named(name)
    r = TC.model(name)
    n = x.shape[0]
    assert r["n_used"] == (n - r["parity"] + 1) // 2
    _expected(name, r)
    _conditions(name, r, mode)
    if name == "m1_zero":
        assert r["floor"] == 0.0 and r["total"] == [0.0, 0.0] and r["thr"] == 0.0
    if name == "m1_odd":
        a, b = r["entries"][0], TC.model("m1_single")["entries"][0]
        assert (a["comb"], a["mask"], a["delay"]) == (b["comb"], b["mask"], b["delay"])


@pytest.mark.parametrize("name", ["m1_two", "m2_two", "m1_none"])
@pytest.mark.parametrize("seed", [6, 7])
def test_other_seeds_of_the_noisy_cases_qualify_as_well(name, seed):
    x, mode = TC.build(name, seed=seed)
    r = tii_scan_model(x, mode, TC.EARLY[mode], False, TC.MIN_RATIO, TC.MIN_REL)
    _expected(name, r)
    _conditions("%s seed %d" % (name, seed), r, mode)


def _null_symbol_frames(mode, comb, pattern):
    """Two frames, the first with the TII symbol of (comb, pattern) as the oracle's TII stage emits it -- its carrier set and
    its symbol, placed on the bins as the phase reference symbol is -- in the last N samples of the null symbol; no chain."""
    import oracle as O
    g = geometry(mode)
    N, K, null, tf = g["N"], g["K"], g["null"], g["tf"]
    pr, _ = O.phase_reference(mode)
    sym = np.asarray(O.tii_process(pr, O.tii_pattern(mode, comb, pattern), False, True), np.complex128).reshape(-1)
    R = np.zeros(N, np.complex128)
    R[1:K // 2 + 1] = sym[:K // 2]
    R[N - K // 2:] = sym[K // 2:]
    x = np.zeros((2, tf), np.complex64)
    x[0, null - N:null] = np.fft.ifft(R)
    return x


@pytest.mark.parametrize("mode", [1, 2])
def test_every_pattern_reads_as_configured_in_mode_1_and_half_exchanged_in_mode_2(mode):
    """All 70 patterns on combs 0, 3 and 23: the mask the model reads from the oracle's carrier set is row p of the table in
    Mode I and the row with bits b and b + 4 exchanged in Mode II, at delay 0."""
    P, _ = phase_reference_bins(mode)
    assert len(PATTERNS) == 70 and PATTERNS[0] == 0x0f and PATTERNS[5] == 0x27 and PATTERNS[69] == 0xf0
    for comb in (0, 3, 23):
        for p in range(70):
            r = tii_scan_model(_null_symbol_frames(mode, comb, p), mode, 0)
            want = p if mode == 1 else exchanged(p)
            assert r["n_entries"] == 1 and r["parity"] == 0 and r["n_used"] == 1, (mode, comb, p, r["entries"])
            e = r["entries"][0]
            assert (e["comb"], e["pattern"], e["mask"], e["n_set"]) == (comb, want, PATTERNS[want], 4), (mode, comb, p, e)
            assert e["delay"] == 0.0 and abs(e["delay_coarse"]) < 1e-6, (mode, comb, p, e)
    assert exchanged(5) == 32 and all(exchanged(exchanged(p)) == p for p in range(70))


def test_tii_scan_check_accepts_and_refuses_the_documented_ranges():
    pkg = load_pkg()
    for mode in (1, 2):
        g = geometry(mode)
        top = g["null"] - g["N"]
        pkg.tii_scan_check(mode, 2, 0)
        pkg.tii_scan_check(mode, 64, top, True, 1.0, 0.0)
        for bad in (-1, top + 1):
            with pytest.raises(pkg.DabGpuError) as e:
                pkg.tii_scan_check(mode, 2, bad)
            assert "early must lie in 0 ... null_size - spacing" in str(e.value)
        for n in (0, 1):
            with pytest.raises(pkg.DabGpuError) as e:
                pkg.tii_scan_check(mode, n, 0)
            assert "n_frames must lie in 2 ... max_frames" in str(e.value)
        for bad in (0.999, -3.0, float("inf"), float("nan")):
            with pytest.raises(pkg.DabGpuError) as e:
                pkg.tii_scan_check(mode, 2, 0, False, bad)
            assert "min_ratio must be finite and at least 1" in str(e.value)
        for bad in (1.0, -1e-6, float("nan"), float("inf")):
            with pytest.raises(pkg.DabGpuError) as e:
                pkg.tii_scan_check(mode, 2, 0, False, 12.0, bad)
            assert "min_rel must lie in [0, 1)" in str(e.value)
    for mode in (3, 4, 0):
        with pytest.raises(pkg.DabGpuError) as e:
            pkg.tii_scan_check(mode, 2, 0)
        assert "only transmission modes I and II carry TII" in str(e.value)
    with pytest.raises(pkg.DabGpuError) as e:
        pkg.tii_scan_check(9, 2, 0)
    assert "mode not valid" in str(e.value)
    lib = pkg.load_library()
    assert lib.dabgpu_tii_scan_check(1, 2, None) != 0 and b"null argument" in lib.dabgpu_last_error(None)


def test_header_library_and_exports_are_in_step():
    import ctypes as C
    pkg = load_pkg()
    text = open(os.path.join(ROOT, "include", "dabgpu.h")).read()
    lib = pkg.load_library()
    for name in ENTRIES:
        assert re.search(r"DABGPU_API int %s\(" % name, text), name
        assert name in pkg.EXPORTS and hasattr(lib, name) and not name.endswith("_process"), name
    for struct, fields in (("dabgpu_tii_scan_config", ("early", "old_variant", "min_ratio", "min_rel")),
                           ("dabgpu_tii_scan_head", ("n_used", "parity", "n_entries", "floor", "total[2]")),
                           ("dabgpu_tii_entry", ("comb", "pattern", "mask", "n_set", "energy", "delay_coarse", "delay", "runner_up"))):
        st = re.search(r"typedef struct %s\s*\{(.*?)\}" % struct, text, re.S).group(1)
        for field in fields:
            assert field in st, (struct, field)
    assert C.sizeof(pkg._TiiScanHead) == 40 and C.sizeof(pkg._TiiEntry) == 48 and pkg.TII_SLOTS == 24
    for m in ("tii_scan", "tii_scan_dev", "tii_scan_result", "tii_scan_result_bytes"):
        assert callable(getattr(pkg.Modulator, m)), m
    assert callable(pkg.tii_scan_check)
    assert "bits b and b + 4 exchanged" in text and "the TII analyser" in text
