"""The synchroniser without a device: the float64 model (tests/sync_model.py) finds the frames of every capture the GPU tests
assert equal integers on (tests/sync_cases.py, built from the oracle's chains), every integer decision is far from going the
other way, the model's extracted frames decode to the input bits through the numpy receiver, and the shape refusals are host
code alone."""
import os
import re

import numpy as np
import pytest

from tests import demod_cases as DC
from tests import sync_cases as SY
from tests.conftest import ROOT, load_pkg
from tests.receiver import dab_demodulate
from tests.sync_model import extract_model, extract_slots, geometry, integer_phase, phase_step, sync_model

ENTRIES = ["dabgpu_sync_dev", "dabgpu_sync", "dabgpu_get_sync_result", "dabgpu_sync_extract_dev", "dabgpu_sync_extract",
           "dabgpu_sync_check"]


@pytest.mark.parametrize("name", sorted(SY.CASES))
def test_model_finds_the_frames_of_every_case_with_margin_and_its_frames_decode(name):
    x, mode, bits, start, cfo = SY.named(name)
    g = geometry(mode)
    r = sync_model(x, mode, SY.MAX_SHIFT, 2)
    assert r["n_frames"] == 2, r
    print("%s: coarse0 %d, null_depth %.3g, S second/lowest %.3g / %.3g" % (name, r["coarse0"], r["null_depth"], r["s_second"], r["s_lowest"]))
    assert r["s_lowest"] == 0.0 or r["s_second"] >= 1.5 * r["s_lowest"]
    for k, (fr, mg) in enumerate(zip(r["frames"], r["margins"])):
        true = start + k * g["tf"]
        print("  frame %d: start %d (true %d) shift %d eps %+.6f quality %.4f, runner-up D %.3g c %.3g"
              % (k, fr["start"], true, fr["shift"], fr["eps"], fr["quality"], mg["d_runner_up"], mg["c_runner_up"]))
        if name in SY.CFG3_CASES:
            assert abs(fr["start"] - true) <= SY.NTAPS - 1
        else:
            assert fr["start"] == true
        assert fr["valid"] == 1
        assert abs(fr["shift"] + fr["eps"] - cfo) <= 1e-3
        assert abs(fr["cfo_hz"] - (fr["shift"] + fr["eps"]) * 2048000.0 / g["N"]) < 1e-6
        assert fr["quality"] >= 0.8 and fr["quality"] <= 1.0 + 1e-12
        assert mg["d_runner_up"] <= 0.5 and mg["c_runner_up"] <= 0.5
        assert abs(fr["eps"]) <= 0.45
    if name == "m2_clean":
        assert r["null_depth"] == 0.0 and r["coarse0"] == 0
    frames = extract_model(x, mode, r["frames"], extract_slots(SY.n_samples(x), mode, 2))
    assert frames.shape == (2, g["tf"])
    for k in range(2):
        assert np.array_equal(dab_demodulate(frames[k], mode, g["CP"] // 2), bits[k]), (name, k)


def test_model_marks_a_frame_that_refines_past_the_end_of_the_buffer_not_valid():
    """The cfg 3 capture with its tail cut to B / 2 samples: the last candidate's coarse start still fits, its refined start
    does not.  (What the device is asserted to do with it follows the model's verdict: tests/test_sync_gpu.py.)"""
    g = geometry(1)
    x, mode, _, start, _ = SY.named("m1_cfg3", g["B"] // 2)
    r = sync_model(x, mode, SY.MAX_SHIFT, 2)
    print([(f["start"], f["valid"]) for f in r["frames"]], SY.n_samples(x))
    assert r["n_frames"] >= 1 and r["frames"][0]["valid"] == 1
    frames = extract_model(x, mode, r["frames"], 2)
    for k, fr in enumerate(r["frames"]):
        assert fr["valid"] == int(fr["start"] + g["tf"] <= SY.n_samples(x))
        if not fr["valid"]:
            assert not frames[k].any()


def test_model_marks_a_frame_that_starts_before_the_buffer_not_valid():
    """The clean Mode II capture without its first five samples (the second capture of tests/test_sync_gpu.py's section 5)."""
    g = geometry(2)
    x = np.array(SY.named("m2_clean", g["null"] + 16)[0][5:])
    pkg = load_pkg()
    pkg.sync_check(2, x.size, SY.MAX_SHIFT)
    r = sync_model(x, 2, SY.MAX_SHIFT, 2)
    assert [(f["start"], f["valid"]) for f in r["frames"]] == [(-5, 0), (g["tf"] - 5, 1)]
    frames = extract_model(x, 2, r["frames"], 2)
    assert not frames[0].any() and frames[1].any()
    assert all(m["d_runner_up"] <= 0.5 and m["c_runner_up"] <= 0.5 for m in r["margins"])


def test_integer_phase_is_the_exact_rotation_to_a_32_bit_turn_fraction():
    step = phase_step(-(12 + 0.4998) / 2048)
    assert 0 <= step < 1 << 64
    ph = integer_phase(196608, step)
    want = -2.0 * np.pi * (12 + 0.4998) / 2048 * np.arange(196608)
    err = np.angle(np.exp(1j * (ph - want)))
    assert np.abs(err).max() < 2.0 * np.pi * 2.0 ** -31
    assert phase_step(0.0) == 0 and not integer_phase(8, 0).any()


def test_sync_check_accepts_and_refuses_the_documented_ranges():
    pkg = load_pkg()
    for mode in (1, 2, 3, 4):
        g = geometry(mode)
        least = 2 * g["tf"] + g["null"]
        pkg.sync_check(mode, least, 0)
        pkg.sync_check(mode, least + 12345, 31)
        with pytest.raises(pkg.DabGpuError) as e:
            pkg.sync_check(mode, least - 1, 5)
        assert "too short" in str(e.value)
        for bad in (-1, 32):
            with pytest.raises(pkg.DabGpuError) as e:
                pkg.sync_check(mode, least, bad)
            assert "max_shift" in str(e.value)
    with pytest.raises(pkg.DabGpuError) as e:
        pkg.sync_check(9, 10 ** 6, 0)
    assert "mode" in str(e.value)


def test_header_library_and_exports_are_in_step():
    pkg = load_pkg()
    text = open(os.path.join(ROOT, "include", "dabgpu.h")).read()
    lib = pkg.load_library()
    for name in ENTRIES:
        assert re.search(r"DABGPU_API int %s\(" % name, text), name
        assert name in pkg.EXPORTS and hasattr(lib, name), name
    st = re.search(r"typedef struct dabgpu_sync_frame \{(.*?)\}", text, re.S).group(1)
    for field in ("start", "shift", "valid", "eps", "cfo_hz", "quality", "null_depth"):
        assert field in st, field
    for m in ("sync", "sync_dev", "sync_result", "sync_extract", "sync_extract_dev"):
        assert callable(getattr(pkg.Modulator, m)), m
    assert "shift + eps" in text and "sampling-clock offset" in text
    assert DC.CP[1] == geometry(1)["CP"]
