"""The channel estimator on the device (cir.hip; include/dabgpu.h, "the channel estimator"): on every case of tests/cir_cases.py
the integers of the float64 model (tests/cir_model.py) exactly and its real figures and arrays within measured bars; byte-identical
repeats and the host-pointer entry; the s16 input form; the whole receiver on the device, modulator -> channel (four paths,
noise, carrier offset) -> sync -> extract -> cir (and demod); refusals; a call between two chain calls; dabmod_file's option.
tests/test_cir_cpu.py checks on the model that every integer decision asked for here is far from going the other way."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import channel_cases as CH
from tests import cir_cases as CC
from tests import demod_cases as DC
from tests import sync_cases as SY
from tests.cir_model import HEAD_INTS, cir_model
from tests.conftest import ROOT, record_bound
from tests.sync_model import geometry

pytestmark = pytest.mark.gpu

E_INVALID = -1
S16 = 1
RESULT_BYTES = 128 + 16 * 32
# Deviation of the device's figures from the float64 model on the same samples, worst over the thirteen cases; measured on the
# device (profiles/cir.txt; one run on one box).  Each bar is four times its worst value, the project's margin for box-to-box
# variation, and no bar may exceed its cap.  A value beyond a cap is a bug in the kernel, not a bar.  Relative (cap 1e-6):
# floor, threshold, peak, total, path_power, resp_mean / resp_min / resp_max (one figure, "resp") and the paths' power.
# Absolute in samples (cap 1e-6): fine, mean_delay, delay_spread.  Absolute (cap 1e-9): outside_guard.  Arrays (cap 1e-9):
# max |difference| / peak for pdp, / resp_max for resp.  Both sides are float64 throughout: what is left is the order of the
# transforms' additions (radix 2 with fused multiply-adds here, np.fft's radices there), a few units in the last place of the
# peak.  floor is the largest relative figure because it is the smallest value: 1e-6 ... 1e-5 of the peak, 1e-7 of it on
# m1_clean, carrying the same absolute rounding.  mean_delay and delay_spread are sums of products with delays of up to 600
# samples.  The worst values below are rounded up in their third digit.
WORST = {
    "floor": 1.32e-14, "threshold": 2.79e-15, "peak": 5.56e-16, "total": 4.45e-16, "path_power": 6.67e-16, "resp": 5.12e-15,
    "power": 8.89e-16, "fine": 7.23e-16, "mean_delay": 1.08e-14, "delay_spread": 2.14e-14, "outside_guard": 3.48e-18,
    "pdp": 5.83e-16, "resp_array": 1.55e-15,
}
CAP = {
    "floor": 1e-6, "threshold": 1e-6, "peak": 1e-6, "total": 1e-6, "path_power": 1e-6, "resp": 1e-6, "power": 1e-6,
    "fine": 1e-6, "mean_delay": 1e-6, "delay_spread": 1e-6, "outside_guard": 1e-9, "pdp": 1e-9, "resp_array": 1e-9,
}


def _bar(figure):
    return min(4.0 * WORST[figure], CAP[figure])


@pytest.fixture(scope="module")
def mods(pkg):
    """one context per mode, three frames, shared"""
    ms = {m: pkg.Modulator(mode=m, max_frames=3) for m in (1, 2, 3, 4)}
    yield ms
    for m in ms.values():
        m.close()


def _run(md, name):
    """cir_dev on the named case -> (head, paths, result bytes, (pdp, resp), the device tensor)"""
    import torch
    x, mode, early, window, min_ratio = CC.named(name)
    d_x = torch.from_numpy(np.array(x)).cuda()
    md.cir_dev(d_x, x.shape[0], early, window, min_ratio, CC.MIN_REL)
    torch.cuda.synchronize()
    head, paths = md.cir_result()
    return head, paths, md.cir_result_bytes(), md.cir_profile(), d_x


def _rel(a, b):
    if b == 0.0:
        assert a == 0.0, (a, b)
        return 0.0
    return abs(a / b - 1.0)


# --------------------------------------------------------------------------- 1 - 2. every case
@pytest.mark.parametrize("name", sorted(CC.CASES))
def test_every_case_gives_the_models_integers_figures_and_arrays_and_repeats_byte_for_byte(mods, name):
    """(1) n_frames, n_peaks, n_paths, peak_index, resp_min_bin, resp_max_bin and every path's index and delay EQUAL to the
    model's; the real figures, pdp and resp within the bars.  (2) a second call on the same buffer and the host-pointer entry
    give the same 640 bytes and the same two arrays."""
    x, mode, early, window, min_ratio = CC.named(name)
    md = mods[mode]
    want = CC.model(name)
    head, got, raw, (pdp, resp), d_x = _run(md, name)
    assert len(raw) == RESULT_BYTES and not any(raw[128 + 32 * head["n_paths"]:])
    for k in HEAD_INTS:
        assert head[k] == want[k], (name, k, head[k], want[k])
    assert len(got) == len(want["paths"]) == want["n_paths"]
    if name == "m1_zero":
        zero = bytearray(RESULT_BYTES)
        zero[0:4] = np.int32(x.shape[0]).tobytes()
        zero[12:16] = np.int32(window).tobytes()
        assert raw == bytes(zero) and not pdp.any() and not resp.any()
    dev = dict.fromkeys(WORST, 0.0)
    for a, b in zip(got, want["paths"]):
        assert (a["index"], a["delay"]) == (b["index"], b["delay"]), (name, a, b)
        dev["power"] = max(dev["power"], _rel(a["power"], b["power"]))
        dev["fine"] = max(dev["fine"], abs(a["fine"] - b["fine"]))
    for k in ("floor", "threshold", "peak", "total", "path_power"):
        dev[k] = _rel(head[k], want[k])
    dev["resp"] = max(_rel(head[k], want[k]) for k in ("resp_mean", "resp_min", "resp_max"))
    for k in ("mean_delay", "delay_spread", "outside_guard"):
        dev[k] = abs(head[k] - want[k])
    assert head["first_delay"] == want["first_delay"]
    if want["peak"] > 0.0:
        dev["pdp"] = float(np.max(np.abs(pdp - want["pdp"])) / want["peak"])
        dev["resp_array"] = float(np.max(np.abs(resp - want["resp"])) / want["resp_max"])
    print("%s: deviation %s; floor device %.6g, model %.6g" % (name, ", ".join("%s %.3g" % kv for kv in dev.items()), head["floor"], want["floor"]))
    # (2) again, and from a host pointer
    md.cir_dev(d_x, x.shape[0], early, window, min_ratio, CC.MIN_REL)
    assert md.cir_result_bytes() == raw
    again = md.cir_profile()
    assert np.array_equal(again[0].view(np.uint64), pdp.view(np.uint64)) and np.array_equal(again[1].view(np.uint64), resp.view(np.uint64))
    md.cir(np.array(x), early, window, min_ratio, CC.MIN_REL)
    assert md.cir_result_bytes() == raw
    host = md.cir_profile()
    assert np.array_equal(host[0].view(np.uint64), pdp.view(np.uint64)) and np.array_equal(host[1].view(np.uint64), resp.view(np.uint64))
    ok = [record_bound("cir %s vs float64 model, %s" % (k, name), dev[k], _bar(k)) for k in WORST]
    assert all(ok), dev


# --------------------------------------------------------------------------- 3. the s16 input form
def test_the_s16_form_gives_the_integers_of_the_complexf_form(mods):
    a = _run(mods[1], "m1_four")
    b = _run(mods[1], "m1_s16")
    assert b[4].dtype.is_floating_point is False
    for k in HEAD_INTS:
        assert a[0][k] == b[0][k], k
    assert [(p["index"], p["delay"]) for p in a[1]] == [(p["index"], p["delay"]) for p in b[1]] and len(b[1]) == 4


# --------------------------------------------------------------------------- 4. the whole receiver on the device
def test_four_paths_through_channel_sync_and_extract_read_as_given(pkg):
    """A modulator (Mode I, cfg 3), four frames with a 1200-sample lead-in from the end of a frame and a tail; channel_dev with
    FOUR1, every path rotated by CC.CFO carrier spacings, noise at C/N 20 dB, seed 5; sync_dev -> sync_extract_dev ->
    cir_dev(early = CP / 2): four paths at 0, 37, 200 and 600 samples from the strongest, levels within 0.5 dB of the model's
    on the same frames, the first three within 0.5 dB of 0 / -6.02 / -12.04 (the fourth loses part of its symbol to the
    null symbol), outside_guard within 1e-3 of the model's.  A second pass through the three paths inside the guard interval
    alone -- those paths and the offset, no noise --, sync -> extract -> demod_dev: no bit error.  (With the noise left on the
    hard decisions of that pass are not error-free, and are not expected to be: the three paths fade some carriers to
    (1 - 0.5 - 0.25)^2 = -12 dB, 8 dB above the noise; measured 18, 29, 42 and 24 errors in the 230400 bits of the four frames.
    The pass with noise is printed, not asserted.)"""
    import torch
    mode, n, lead = 1, 4, 1200
    g = geometry(mode)
    tf, early = g["tf"], g["CP"] // 2
    bits = SY.case_bits(mode, n)                                        # n + 1 frames: the last one lends its ends
    stages = pkg.STAGE_GAIN | pkg.STAGE_FIR
    tail = max(2 * g["B"] + g["N"], g["null"] - lead) + 600
    f = CH.CFO * 2048000.0 / g["N"]
    rx = pkg.Modulator(mode=mode, max_frames=n)
    tx = pkg.Modulator(mode=mode, max_frames=n + 1)
    try:
        d_bits = torch.from_numpy(bits).cuda()
        tx.set_gain(pkg.GAIN_VAR, 1.0, DC.NORMALISE, 4.0)
        tx.set_fir_taps(None)
        d_y = torch.empty((n + 1, tf), dtype=torch.complex64, device="cuda")
        tx.chain_dev(d_bits, n + 1, stages, d_y)
        torch.cuda.synchronize()
        d_stream = torch.cat([d_y[n][tf - lead:], d_y[:n].reshape(-1), d_y[n][:tail]]).contiguous()
        power = CH.data_power(d_stream[lead:lead + n * tf].cpu().numpy(), mode)
        sigma = pkg.channel_sigma(power, 20.0)
        d_frames = torch.zeros((n, tf), dtype=torch.complex64, device="cuda")

        def receive(paths, sigma):
            d_cap = torch.zeros_like(d_stream)
            tx.set_channel([(d, complex(gp), f) for d, gp in paths], sigma, 5)
            tx.channel_reset(0)
            tx.channel_dev(d_stream, d_cap)
            rx.sync_dev(d_cap, 31)
            assert rx.sync_slots(d_cap.numel()) == n
            rx.sync_extract_dev(d_cap, d_frames)
            torch.cuda.synchronize()
            sync = rx.sync_result()
            assert len(sync) == n and all(r["valid"] == 1 and abs(r["shift"] + r["eps"] - CH.CFO) <= 1e-3 for r in sync), sync
            return sync

        sync = receive(CC.FOUR1, sigma)
        rx.cir_dev(d_frames, n, early)
        torch.cuda.synchronize()
        head, got = rx.cir_result()
        want = cir_model(d_frames.cpu().numpy(), mode, early)
        level = [10.0 * np.log10(p["power"] / got[0]["power"]) for p in got]
        level_model = [10.0 * np.log10(p["power"] / want["paths"][0]["power"]) for p in want["paths"]]
        print("sync starts %s; paths %s; levels %s (model on the same frames %s); outside_guard %.5f (model %.5f)"
              % ([r["start"] for r in sync], [(p["delay"], p["fine"]) for p in got], np.round(level, 3), np.round(level_model, 3),
                 head["outside_guard"], want["outside_guard"]))
        assert head["n_paths"] == 4 == want["n_paths"] and head["n_frames"] == n, (head, got)
        assert [p["delay"] - got[0]["delay"] for p in got] == [0.0, 37.0, 200.0, 600.0], got
        assert [p["index"] for p in got] == [p["index"] for p in want["paths"]]
        assert all(abs(a - b) <= 0.5 for a, b in zip(level, level_model)), (level, level_model)
        assert all(abs(a - b) <= 0.5 for a, b in zip(level[:3], (0.0, -6.02, -12.04))), level
        assert abs(head["outside_guard"] - want["outside_guard"]) <= 1e-3
        d_out = torch.zeros((n, rx.geometry["tf_input_bytes"]), dtype=torch.uint8, device="cuda")
        for noise in (sigma, 0.0):
            receive(CC.FOUR1[:3], noise)
            rx.demod_dev(d_frames, n, early, d_out, d_bits[:n].contiguous())
            torch.cuda.synchronize()
            stats = [rx.monitor_stats(k) for k in range(n)]
            print("three paths, sigma %.4g: bit errors per frame %s" % (noise, [s["bit_errors"] for s in stats]))
        assert all(s["bit_errors"] == 0 and s["n_bits"] == 8 * bits.shape[1] for s in stats), stats
        assert np.array_equal(d_out.cpu().numpy(), bits[:n])
    finally:
        rx.close()
        tx.close()


# --------------------------------------------------------------------------- 5. refusals
def test_refusals_return_invalid_and_leave_the_previous_result_alone(pkg, mods):
    import torch
    x, mode, early, window, min_ratio = CC.named("m1_four")
    md = mods[mode]
    lib, h = md._lib, md._h
    g = geometry(mode)
    fresh = pkg.Modulator(mode=mode, max_frames=2)
    try:
        with pytest.raises(pkg.DabGpuError, match="no channel estimate"):
            fresh.cir_result()
        with pytest.raises(pkg.DabGpuError, match="no channel estimate"):
            fresh.cir_profile()
    finally:
        fresh.close()
    _, _, raw, (pdp, resp), d_x = _run(md, "m1_four")
    px = d_x.data_ptr()
    d_s16 = torch.zeros(4 * g["tf"], dtype=torch.int16, device="cuda")

    def cfg(early=early, window=1, min_ratio=20.0, min_rel=1e-3):
        c = pkg._CirConfig()
        c.early, c.window, c.min_ratio, c.min_rel = early, window, min_ratio, min_rel
        return C.byref(c)

    def dev(p, fmt, n, c):
        return lib.dabgpu_cir_dev(h, p, fmt, n, c, None)

    host = np.array(x)
    hp = host.ctypes.data
    calls = {
        "no frame": (lambda: dev(px, 0, 0, cfg()), "n_frames must lie in 1 ... max_frames"),
        "more than max_frames": (lambda: dev(px, 0, 4, cfg()), "n_frames must lie in 1 ... max_frames"),
        "early below": (lambda: dev(px, 0, 3, cfg(early=-1)), "early must lie in 0 ... sym_size - spacing"),
        "early above": (lambda: dev(px, 0, 3, cfg(early=g["CP"] + 1)), "early must lie in 0 ... sym_size - spacing"),
        "window 2": (lambda: dev(px, 0, 3, cfg(window=2)), "window is 0 (rectangular) or 1 (Hann)"),
        "window negative": (lambda: dev(px, 0, 3, cfg(window=-1)), "window is 0 (rectangular) or 1 (Hann)"),
        "min_ratio below 1": (lambda: dev(px, 0, 3, cfg(min_ratio=0.5)), "min_ratio must be finite and at least 1"),
        "min_ratio nan": (lambda: dev(px, 0, 3, cfg(min_ratio=float("nan"))), "min_ratio must be finite and at least 1"),
        "min_ratio inf": (lambda: dev(px, 0, 3, cfg(min_ratio=float("inf"))), "min_ratio must be finite and at least 1"),
        "min_rel 1": (lambda: dev(px, 0, 3, cfg(min_rel=1.0)), "min_rel must lie in [0, 1)"),
        "min_rel negative": (lambda: dev(px, 0, 3, cfg(min_rel=-0.5)), "min_rel must lie in [0, 1)"),
        "min_rel nan": (lambda: dev(px, 0, 3, cfg(min_rel=float("nan"))), "min_rel must lie in [0, 1)"),
        "u8": (lambda: dev(px, 2, 3, cfg()), "input format is complexf"),
        "s8": (lambda: dev(px, 3, 3, cfg()), "input format is complexf"),
        "null frames": (lambda: dev(None, 0, 3, cfg()), "null argument"),
        "null settings": (lambda: dev(px, 0, 3, None), "null argument"),
        "misaligned": (lambda: dev(px + 4, 0, 2, cfg()), "aligned to a sample"),
        "misaligned s16": (lambda: dev(d_s16.data_ptr() + 2, S16, 1, cfg()), "aligned to a sample"),
        "host form, no frame": (lambda: lib.dabgpu_cir(h, hp, 0, 0, cfg()), "n_frames must lie in 1 ... max_frames"),
        "host form, too many": (lambda: lib.dabgpu_cir(h, hp, 0, 4, cfg()), "n_frames must lie in 1 ... max_frames"),
        "host form, early": (lambda: lib.dabgpu_cir(h, hp, 0, 3, cfg(early=g["CP"] + 1)), "early must lie in 0 ... sym_size - spacing"),
        "host form, window": (lambda: lib.dabgpu_cir(h, hp, 0, 3, cfg(window=3)), "window is 0 (rectangular) or 1 (Hann)"),
        "host form, min_ratio": (lambda: lib.dabgpu_cir(h, hp, 0, 3, cfg(min_ratio=0.0)), "min_ratio must be finite and at least 1"),
        "host form, min_rel": (lambda: lib.dabgpu_cir(h, hp, 0, 3, cfg(min_rel=2.0)), "min_rel must lie in [0, 1)"),
        "host form, u8": (lambda: lib.dabgpu_cir(h, hp, 2, 3, cfg()), "input format is complexf"),
        "host form, null": (lambda: lib.dabgpu_cir(h, None, 0, 3, cfg()), "null argument"),
        "host form, null settings": (lambda: lib.dabgpu_cir(h, hp, 0, 3, None), "null argument"),
    }
    for name, (call, message) in calls.items():
        assert call() == E_INVALID, name
        assert message in lib.dabgpu_last_error(h).decode(), (name, lib.dabgpu_last_error(h))
        assert md.cir_result_bytes() == raw, name
    with pytest.raises(pkg.DabGpuError):
        md.cir_dev(d_x, 4, early)                                       # (the wrapper: the tensor holds three frames)
    with pytest.raises(pkg.DabGpuError):
        md.cir(host.reshape(-1)[:-1], early)
    assert md.cir_result_bytes() == raw
    again = md.cir_profile()
    assert np.array_equal(again[0], pdp) and np.array_equal(again[1], resp)
    _, _, once_more, _, _ = _run(md, "m1_four")                          # a valid call follows
    assert once_more == raw


# --------------------------------------------------------------------------- 6. between two chain calls
def test_a_call_between_two_chain_calls_leaves_the_second_calls_bytes_alone(pkg):
    """cfg 3 with TII, one frame per call (the TII parity advances with every call): call, call -> y1, y2; call, cir, call on
    the same context -> the same y1, y2."""
    import torch
    mode = 1
    tf = geometry(mode)["tf"]
    x, _, early, _, _ = CC.named("m1_four")
    bits = SY.case_bits(mode, 1)
    stages = pkg.STAGE_GAIN | pkg.STAGE_FIR
    md = pkg.Modulator(mode=mode, max_frames=2)
    try:
        md.set_gain(pkg.GAIN_VAR, 1.0, DC.NORMALISE, 4.0)
        md.set_fir_taps(None)
        md.set_tii(True, 3, 5)
        d_bits = torch.from_numpy(bits).cuda()
        d_x = torch.from_numpy(np.array(x[:2])).cuda()
        outs = []
        for between in (False, True):
            d_y = torch.zeros((2, tf), dtype=torch.complex64, device="cuda")
            md.chain_dev(d_bits[0:1], 1, stages, d_y[0])
            if between:
                md.cir_dev(d_x, 2, early)
            md.chain_dev(d_bits[1:2], 1, stages, d_y[1])
            torch.cuda.synchronize()
            outs.append(d_y.cpu().numpy())
        head, got = md.cir_result()
        assert head["n_frames"] == 2 and head["n_paths"] >= 1 and got[0]["delay"] == -22.0
        assert outs[0].any() and np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32))
        assert not np.array_equal(outs[0][0, :2656], outs[0][1, :2656])  # (the two calls differ: one null symbol carries TII)
    finally:
        md.close()


# --------------------------------------------------------------------------- 7. dabmod_file --cir
def _dabmod_file(fin, fout, opts):
    exe = os.path.join(ROOT, "odr-dabmod_amd", "host", "dabmod_file")
    return subprocess.run([exe, fin, fout] + opts, capture_output=True, text=True, timeout=300)


def _paths(stderr):
    """[(delay, level in dB, fine)] of the "cir: path" lines"""
    out = []
    for ln in stderr.splitlines():
        if "cir: path delay" in ln:
            w = ln.split()
            out.append((float(w[w.index("delay") + 1]), float(w[w.index("level") + 1]), float(w[w.index("fine") + 1])))
    return out


def test_dabmod_file_cir_reads_the_filters_look_ahead(tmp_path):
    """Mode I, FIRFilter, four frames in one batch: one path at delay -22, exit 0, FILE has one line per tap."""
    fin, fcir = str(tmp_path / "in.eti"), str(tmp_path / "cir.txt")
    DC.eti_frames(4, 1).tofile(fin)
    r = _dabmod_file(fin, str(tmp_path / "out"), ["--mode", "1", "--fir", "default", "--batch", "4", "--cir", fcir])
    print(r.stderr[-900:])
    assert r.returncode == 0, r.stderr[-2000:]
    assert "cir: 4 frames, window 44 samples early" in r.stderr and "1 peak, 1 path" in r.stderr
    paths = _paths(r.stderr)
    assert len(paths) == 1 and paths[0][0] == -22.0 and paths[0][1] == 0.0
    rows = np.loadtxt(fcir)
    assert rows.shape == (2048, 2) and np.array_equal(rows[:, 0], np.arange(-1024, 1024) - 44)
    assert rows[np.argmax(rows[:, 1]), 0] == -22.0 and rows[:, 1].max() == 0.0


def test_dabmod_file_cir_shows_the_echo_the_channel_was_given(tmp_path):
    """--loopback --channel-cn 30 --channel-echo 37,-6,1.0: the batch behind the channel reads as two paths 37 samples and
    6.0 +- 0.5 dB apart."""
    fin, fcir = str(tmp_path / "in.eti"), str(tmp_path / "cir.txt")
    DC.eti_frames(4, 1).tofile(fin)
    r = _dabmod_file(fin, str(tmp_path / "out"), ["--mode", "1", "--batch", "4", "--gpu-frontend", "--loopback", "--channel-cn", "30",
                                                  "--channel-echo", "37,-6,1.0", "--cir", fcir])
    print(r.stderr[-1200:])
    assert r.returncode == 0, r.stderr[-2000:]
    assert "frames behind the channel" in r.stderr
    paths = _paths(r.stderr)
    assert len(paths) == 2 and paths[1][0] - paths[0][0] == 37.0 and abs(paths[0][1] - paths[1][1] - 6.0) <= 0.5, paths
    assert np.loadtxt(fcir).shape == (2048, 2)


def test_dabmod_file_refuses_cir_where_there_is_nothing_it_can_read(tmp_path):
    fin = str(tmp_path / "in.eti")
    DC.eti_frames(1, 2).tofile(fin)
    for opts, why in ((["--rate", "4096000"], "--rate"), (["--format", "u8"], "u8 / s8"), (["--format", "s8"], "u8 / s8"),
                      (["--bits-only"], "--bits-only"), (["--separate-converter"], "--separate-converter")):
        fout, fcir = str(tmp_path / "refused"), str(tmp_path / "refused.txt")
        r = _dabmod_file(fin, fout, ["--mode", "2", "--cir", fcir] + opts)
        assert r.returncode == 2 and "--cir does not go with " + why in r.stderr, (opts, r.stderr[-500:])
        assert not os.path.exists(fout) and not os.path.exists(fcir), opts
