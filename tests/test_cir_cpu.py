"""The channel estimator without a device: the float64 model (tests/cir_model.py) reads every case the GPU tests assert equal
integers on (tests/cir_cases.py, built from the oracle's chains) as the table of the definition's issue says, with every integer
decision far from going the other way; a closed form -- a window built from known taps reads back as those taps --; and the
settings' refusals, which are host code alone."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import cir_cases as CC
from tests.cir_model import HEAD_INTS, HEAD_REALS, cir_model, impulse_response
from tests.conftest import ROOT, load_pkg
from tests.sync_model import geometry, phase_reference_bins

ENTRIES = ["dabgpu_cir_dev", "dabgpu_cir", "dabgpu_get_cir", "dabgpu_get_cir_profile", "dabgpu_cir_check"]
MARGIN_DB = 0.05                                   # every local maximum of the profile lies this far from the threshold
NEIGHBOUR = 1.01                                   # every reported peak exceeds both neighbours by 1 %
# two reported paths next to each other in the list differ in power by this much, relative: the device's float64 transform
# differs from np.fft by some 1e-13 of the peak, so the order of the list is not at stake
ORDER = 1e-9


def _levels(r):
    top = r["paths"][0]["power"]
    return [(p["delay"], 10.0 * np.log10(p["power"] / top)) for p in r["paths"]]


@pytest.mark.parametrize("name", sorted(CC.CASES))
def test_model_reads_every_case_as_the_table_says_with_margin(name):
    x, mode, early, window, min_ratio = CC.named(name)
    r = CC.model(name)
    want, n_peaks = CC.EXPECT[name]
    got = _levels(r) if r["paths"] else []
    print("%s: n_peaks %d, paths %s, margin %.2f dB, floor / peak %.3g, outside_guard %.5f, resp_min / resp_mean %.3g"
          % (name, r["n_peaks"], [(d, round(float(l), 2)) for d, l in got], r["margin_db"],
             r["floor"] / r["peak"] if r["peak"] else 0.0, r["outside_guard"], r["resp_min"] / r["resp_mean"] if r["resp_mean"] else 0.0))
    assert r["n_frames"] == x.shape[0] and r["window"] == window
    assert r["n_peaks"] == n_peaks and r["n_paths"] == min(n_peaks, 16) == len(r["paths"])
    if name == "m1_zero":
        assert all(r[k] == 0 for k in HEAD_INTS if k not in ("n_frames", "window")) and all(r[k] == 0.0 for k in HEAD_REALS)
        assert not r["pdp"].any() and not r["resp"].any()
        return
    # the delays exactly, the levels within 0.5 dB; side lobes of equal height (the rectangular cases) in either order
    head = got[:len(want)]
    assert sorted(d for d, _ in head) == sorted(d for d, _ in want), (name, got)
    for d, level in head:
        assert abs(level - dict(want)[d]) <= CC.LEVEL_TOL_DB, (name, d, level)
    assert [l for _, l in got] == sorted((l for _, l in got), reverse=True)
    pdp, N = r["pdp"], pdp_len(mode)
    for p in r["paths"]:
        l = p["index"]
        assert pdp[l] >= NEIGHBOUR * pdp[(l - 1) % N] and pdp[l] >= NEIGHBOUR * pdp[(l + 1) % N], (name, p)
        assert abs(p["fine"]) <= 0.5
    for p, q in zip(r["paths"], r["paths"][1:]):
        assert p["power"] >= (1.0 + ORDER) * q["power"], (name, p, q)
    assert r["margin_db"] >= MARGIN_DB, (name, r["margin_db"])
    assert r["peak_index"] == r["paths"][0]["index"] and r["first_delay"] == min(d for d, _ in got)
    assert abs(r["path_power"] / sum(p["power"] for p in r["paths"]) - 1.0) < 1e-12
    if name in ("m1_four", "m1_s16"):
        assert abs(r["outside_guard"] - CC.OUTSIDE_GUARD_M1_FOUR) <= 1e-4, r["outside_guard"]      # (the table's last digit)
    elif max(d for d, _ in got) - min(d for d, _ in got) <= geometry(mode)["CP"]:
        assert r["outside_guard"] == 0.0
    if name == "m1_close":
        assert abs(r["resp_min"] / r["resp_mean"] / CC.RESP_DIP_M1_CLOSE - 1.0) <= 0.05
    if name == "m1_s16":
        a = CC.model("m1_four")
        assert [(p["index"], p["delay"]) for p in r["paths"]] == [(p["index"], p["delay"]) for p in a["paths"]]
        assert all(r[k] == a[k] for k in HEAD_INTS)


def pdp_len(mode):
    return geometry(mode)["N"]


@pytest.mark.parametrize("mode", [1, 2, 3, 4])
def test_a_window_built_from_three_taps_reads_back_as_those_taps(mode):
    """x's window = IDFT(P sum_p g_p e^{-j 2 pi k d_p / N}) exactly, three integer delays: with the rectangular weights
    h[d_p] = g_p to 1e-12, and with one isolated path alone `fine` is 0 to 1e-9.  The delays lie multiples of 8 samples apart:
    a tap leaks into index l as (1 / K) sum_k e^{j 2 pi k m / N} at distance m, which with K = 3 N / 4 carriers around an empty
    centre is 2 sin(3 pi m / 8) cos(...) / (K sin(pi m / N)) -- zero at every multiple of 8, so the taps do not touch each other
    there, and by the same sum the mean of |H|^2 over the carriers is sum |g_p|^2."""
    g = geometry(mode)
    N, K, null, CP, tf = g["N"], g["K"], g["null"], g["CP"], g["tf"]
    P, occ = phase_reference_bins(mode)
    k = np.where(np.arange(N) <= N // 2, np.arange(N), np.arange(N) - N)
    early = CP // 2
    taps = [(3, 1.0 + 0.0j), (3 + N // 8, 0.4 * np.exp(1j * 1.0)), (3 + N // 4 + 8, -0.1j)]
    for paths in (taps, taps[:1]):
        spec = P * sum(gp * np.exp(-2j * np.pi * k * d / N) for d, gp in paths)
        x = np.zeros((1, tf), np.complex128)
        w0 = null + CP - early
        x[0, w0:w0 + N] = np.fft.ifft(spec)
        h, H = impulse_response(x, mode, early, 0)
        for d, gp in paths:
            assert abs(h[0, d] - gp) <= 1e-12, (mode, d, h[0, d], gp)
        assert np.allclose(np.abs(H[0, occ]) ** 2, np.abs(sum(gp * np.exp(-2j * np.pi * k * d / N) for d, gp in paths))[occ] ** 2,
                           rtol=0, atol=1e-12)
        r = cir_model(x, mode, early, 0, 20.0, 1e-3)
        assert r["paths"][0]["index"] == 3 and r["paths"][0]["delay"] == 3.0 - early
        assert abs(r["resp_mean"] - sum(abs(gp) ** 2 for _, gp in paths)) <= 1e-12
    assert abs(r["paths"][0]["fine"]) <= 1e-9 and abs(r["paths"][0]["power"] - 1.0) <= 1e-12


def test_cir_check_accepts_and_refuses_the_documented_ranges():
    pkg = load_pkg()
    for mode in (1, 2, 3, 4):
        g = geometry(mode)
        pkg.cir_check(mode, 1, 0)
        pkg.cir_check(mode, 64, g["CP"], 0, 1.0, 0.0)
        for bad in (-1, g["CP"] + 1):
            with pytest.raises(pkg.DabGpuError) as e:
                pkg.cir_check(mode, 1, bad)
            assert "early must lie in 0 ... sym_size - spacing" in str(e.value)
        with pytest.raises(pkg.DabGpuError) as e:
            pkg.cir_check(mode, 0, 0)
        assert "n_frames must lie in 1 ... max_frames" in str(e.value)
        for bad in (-1, 2, 7):
            with pytest.raises(pkg.DabGpuError) as e:
                pkg.cir_check(mode, 1, 0, bad)
            assert "window is 0 (rectangular) or 1 (Hann)" in str(e.value)
        for bad in (0.999, -3.0, float("inf"), float("nan")):
            with pytest.raises(pkg.DabGpuError) as e:
                pkg.cir_check(mode, 1, 0, 1, bad)
            assert "min_ratio must be finite and at least 1" in str(e.value)
        for bad in (1.0, -1e-6, float("nan"), float("inf")):
            with pytest.raises(pkg.DabGpuError) as e:
                pkg.cir_check(mode, 1, 0, 1, 20.0, bad)
            assert "min_rel must lie in [0, 1)" in str(e.value)
    with pytest.raises(pkg.DabGpuError) as e:
        pkg.cir_check(9, 1, 0)
    assert "mode not valid" in str(e.value)
    lib = pkg.load_library()
    assert lib.dabgpu_cir_check(1, 1, None) != 0 and b"null argument" in lib.dabgpu_last_error(None)


def test_header_library_and_exports_are_in_step():
    pkg = load_pkg()
    text = open(os.path.join(ROOT, "include", "dabgpu.h")).read()
    lib = pkg.load_library()
    for name in ENTRIES:
        assert re.search(r"DABGPU_API int %s\(" % name, text), name
        assert name in pkg.EXPORTS and hasattr(lib, name) and not name.endswith("_process"), name
    for struct, fields in (("dabgpu_cir_config", ("early", "window", "min_ratio", "min_rel")),
                           ("dabgpu_cir_head", HEAD_INTS + HEAD_REALS + ("reserved",)),
                           ("dabgpu_cir_path", ("index", "reserved", "delay", "fine", "power"))):
        st = re.search(r"typedef struct %s\s*\{(.*?)\}" % struct, text, re.S).group(1)
        for field in fields:
            assert field in st, (struct, field)
    assert C.sizeof(pkg._CirHead) == 128 and C.sizeof(pkg._CirPath) == 32 and pkg.CIR_MAX_PATHS == 16
    assert re.search(r"#define DABGPU_CIR_MAX_PATHS 16\b", text)
    for m in ("cir", "cir_dev", "cir_result", "cir_result_bytes", "cir_profile"):
        assert callable(getattr(pkg.Modulator, m)), m
    assert callable(pkg.cir_check)
    for phrase in ("the channel estimator", "coherent averaging across frames", "Doppler per path", "sampling-clock offset",
                   "u8 / s8", "resampled captures", "e^{-0.69 min_ratio}"):
        assert phrase in text, phrase
