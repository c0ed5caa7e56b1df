"""The TII analyser on the device (tii_scan.hip; include/dabgpu.h, "the TII analyser"): on every case of tests/tii_scan_cases.py
the integers of the float64 model (tests/tii_scan_model.py) exactly and its real figures within measured bars; byte-identical
repeats and the host-pointer entry; the whole receiver on the device, two modulators with different TII -> channel -> sync ->
extract -> scan (and demod); refusals; a scan between two chain calls; dabmod_file's option.  tests/test_tii_scan_cpu.py checks on the model that
every integer decision asked for here is far from going the other way."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import channel_cases as CC
from tests import demod_cases as DC
from tests import sync_cases as SY
from tests import tii_scan_cases as TC
from tests.conftest import ROOT, record_bound
from tests.sync_model import geometry
from tests.tii_scan_model import tii_scan_model

pytestmark = pytest.mark.gpu

E_INVALID = -1
S16 = 1
# Deviation of the device's figures from the float64 model on the same samples, worst over the nine cases; measured on the
# device (profiles/tii_scan.txt; one run on one box).  Each bar is four times its worst value, the project's margin for
# box-to-box variation, and no bar may exceed its cap: 1e-6 relative (the standing bar of INTEGRATION.md F), 1e-3 samples for
# delay_coarse.  A value beyond a cap is a bug, not a bar.  energy, floor, total: relative; delay_coarse: absolute, in samples;
# runner_up: absolute.  The worst values below are rounded up in their third digit.
# energy, total and delay_coarse are float64 on both sides: a few units in the last place.  floor: on a clean capture it is the
# samples' own rounding, 1e-14 of the set cells, and either side's float64 rounding shows in it.  runner_up: the fp32 inner
# sums of the fine delay.  (With the fp32 transform that was built first the floor of the four clean cases was 0.19 ... 0.54
# off -- beyond the cap -- and the other figures 7e-8: the transform is a float64 direct sum for that reason.)
WORST_ENERGY = 7.78e-16
WORST_FLOOR = 1.87e-9
WORST_TOTAL = 8.89e-16
WORST_DELAY_COARSE = 1.53e-13
WORST_RUNNER_UP = 1.13e-7
CAP_RELATIVE, CAP_DELAY_COARSE = 1e-6, 1e-3


def _bar(worst, cap=None):
    bar = 4.0 * worst if worst is not None else 0.0
    return bar if cap is None else min(bar, cap)


@pytest.fixture(scope="module")
def mods(pkg):
    """one context per mode, five frames, shared"""
    ms = {m: pkg.Modulator(mode=m, max_frames=5) for m in (1, 2)}
    yield ms
    for m in ms.values():
        m.close()


def _scan(md, name):
    """tii_scan_dev on the named case -> (head, entries, result bytes, the device tensor)"""
    import torch
    x, mode, early, old = TC.named(name)
    d_x = torch.from_numpy(np.array(x)).cuda()
    md.tii_scan_dev(d_x, x.shape[0], early, old, TC.MIN_RATIO, TC.MIN_REL)
    torch.cuda.synchronize()
    head, entries = md.tii_scan_result()
    return head, entries, md.tii_scan_result_bytes(), d_x


def _rel(a, b):
    return abs(a / b - 1.0)


# --------------------------------------------------------------------------- 1 - 2. every case
@pytest.mark.parametrize("name", sorted(TC.CASES))
def test_every_case_gives_the_models_integers_and_figures_and_repeats_byte_for_byte(mods, name):
    """(1) n_used, parity (where asserted), n_entries, comb, mask, n_set, pattern EQUAL to the model's; delay within one grid
    step of the model's; energy, floor, total, delay_coarse, runner_up within the bars.  (2) a second call on the same buffer
    and the host-pointer entry give the same result bytes."""
    x, mode, early, old = TC.named(name)
    md = mods[mode]
    want = TC.model(name)
    head, got, raw, d_x = _scan(md, name)
    assert head["n_used"] == want["n_used"] and head["n_entries"] == want["n_entries"] == len(got), (head, want["entries"])
    if TC.EXPECT[name][1] is not None:
        assert head["parity"] == want["parity"] == TC.EXPECT[name][1]
    dev_e = dev_f = dev_t = dev_c = dev_r = 0.0
    differ = 0
    for a, b in zip(got, want["entries"]):
        assert (a["comb"], a["mask"], a["n_set"], a["pattern"]) == (b["comb"], b["mask"], b["n_set"], b["pattern"]), (a, b)
        assert abs(a["delay"] - b["delay"]) <= want["step"], (a, b)
        differ += a["delay"] != b["delay"]
        dev_e = max(dev_e, _rel(a["energy"], b["energy"]))
        dev_c = max(dev_c, abs(a["delay_coarse"] - b["delay_coarse"]))
        dev_r = max(dev_r, abs(a["runner_up"] - b["runner_up"]))
    if want["floor"] == 0.0:
        assert head["floor"] == 0.0
    else:
        dev_f = _rel(head["floor"], want["floor"])
    for p in (0, 1):
        if want["total"][p] == 0.0:
            assert head["total"][p] == 0.0
        else:
            dev_t = max(dev_t, _rel(head["total"][p], want["total"][p]))
    print("%s: deviation energy %.3g, floor %.3g (device %.6g, model %.6g), total %.3g, delay_coarse %.3g, runner_up %.3g; "
          "delays that differ at all: %d of %d" % (name, dev_e, dev_f, head["floor"], want["floor"], dev_t, dev_c, dev_r, differ, len(got)))
    # (2) again, and from a host pointer
    md.tii_scan_dev(d_x, x.shape[0], early, old, TC.MIN_RATIO, TC.MIN_REL)
    assert md.tii_scan_result_bytes() == raw and len(raw) == 40 + 24 * 48
    assert not any(raw[40 + 48 * head["n_entries"]:])
    md.tii_scan(np.array(x), early, old, TC.MIN_RATIO, TC.MIN_REL)
    assert md.tii_scan_result_bytes() == raw
    ok = [record_bound("tii_scan energy vs float64 model, %s" % name, dev_e, _bar(WORST_ENERGY, CAP_RELATIVE)),
          record_bound("tii_scan floor vs float64 model, %s" % name, dev_f, _bar(WORST_FLOOR, CAP_RELATIVE)),
          record_bound("tii_scan total vs float64 model, %s" % name, dev_t, _bar(WORST_TOTAL, CAP_RELATIVE)),
          record_bound("tii_scan delay_coarse vs float64 model, %s" % name, dev_c, _bar(WORST_DELAY_COARSE, CAP_DELAY_COARSE)),
          record_bound("tii_scan runner_up vs float64 model, %s" % name, dev_r, _bar(WORST_RUNNER_UP))]
    assert all(ok), (dev_e, dev_f, dev_t, dev_c, dev_r)


# --------------------------------------------------------------------------- 3. the whole receiver on the device
def test_two_transmitters_through_channel_sync_and_extract_read_as_two_entries_37_samples_apart(pkg):
    """Two contexts modulate the same bits (Mode I, cfg 3) with TII (3, 5) and (7, 5); B goes through channel_dev (one path:
    delay 37, gain 0.5 e^{j 1.0}, noise at C/N 20 dB); the sum gets a 1200-sample lead-in from the end of a frame and a tail and
    is rotated by 3.37 spacings; sync_dev -> sync_extract_dev -> tii_scan_dev(early = CP / 2): both entries with pattern 5,
    delay_B - delay_A = 37 within two grid steps, the level difference within 0.5 dB of the model's on the same frames;
    demod_dev on the same frames: no bit error."""
    import torch
    mode, n, lead = 1, 4, 1200
    g = geometry(mode)
    tf, early = g["tf"], g["CP"] // 2
    bits = SY.case_bits(mode, n)                                        # n + 1 frames: the last one lends its ends
    stages = pkg.STAGE_GAIN | pkg.STAGE_FIR
    tail = max(2 * g["B"] + g["N"], g["null"] - lead) + 37
    rx = pkg.Modulator(mode=mode, max_frames=n)
    tx = []
    try:
        d_bits = torch.from_numpy(bits).cuda()
        streams = []
        for comb, pattern in (TC.A, TC.B):
            m = pkg.Modulator(mode=mode, max_frames=n + 1)
            tx.append(m)
            m.set_gain(pkg.GAIN_VAR, 1.0, DC.NORMALISE, 4.0)
            m.set_fir_taps(None)
            m.set_tii(True, comb, pattern)
            d_y = torch.empty((n + 1, tf), dtype=torch.complex64, device="cuda")
            m.chain_dev(d_bits, n + 1, stages, d_y)
            torch.cuda.synchronize()
            streams.append(torch.cat([d_y[n][tf - lead:], d_y[:n].reshape(-1), d_y[n][:tail]]).contiguous())
        power = CC.data_power(streams[0][lead:lead + n * tf].cpu().numpy(), mode)
        d_b = torch.zeros_like(streams[1])
        tx[1].set_channel([(37, complex(TC.B_GAIN), 0.0)], pkg.channel_sigma(power, 20.0), 5)
        tx[1].channel_dev(streams[1], d_b)
        torch.cuda.synchronize()
        d_sum = (streams[0] + d_b).contiguous()
        d_cap = torch.zeros_like(d_sum)
        tx[0].set_channel([(0, 1.0 + 0.0j, CC.CFO * 2048000.0 / g["N"])], 0.0, 0)
        tx[0].channel_dev(d_sum, d_cap)
        rx.sync_dev(d_cap, 31)
        assert rx.sync_slots(d_cap.numel()) == n
        d_frames = torch.zeros((n, tf), dtype=torch.complex64, device="cuda")
        rx.sync_extract_dev(d_cap, d_frames)
        rx.tii_scan_dev(d_frames, n, early)
        d_out = torch.zeros((n, rx.geometry["tf_input_bytes"]), dtype=torch.uint8, device="cuda")
        rx.demod_dev(d_frames, n, early, d_out, d_bits[:n].contiguous())
        torch.cuda.synchronize()
        sync = rx.sync_result()
        assert len(sync) == n and all(r["valid"] == 1 and abs(r["shift"] + r["eps"] - CC.CFO) <= 1e-3 for r in sync), sync
        head, got = rx.tii_scan_result()
        want = tii_scan_model(d_frames.cpu().numpy(), mode, early)
        print("sync starts %s; scan %s" % ([r["start"] for r in sync], got))
        assert head["n_used"] == 2 and head["n_entries"] == 2 == want["n_entries"], (head, got)
        assert [(e["comb"], e["pattern"], e["n_set"]) for e in got] == [(3, 5, 4), (7, 5, 4)], got
        assert abs(got[1]["delay"] - got[0]["delay"] - 37.0) <= 2.0 * want["step"], got
        level = 10.0 * np.log10(got[0]["energy"] / got[1]["energy"])
        level_model = 10.0 * np.log10(want["entries"][0]["energy"] / want["entries"][1]["energy"])
        print("level difference %.3f dB (model on the same frames %.3f dB)" % (level, level_model))
        assert abs(level - level_model) <= 0.5
        stats = [rx.monitor_stats(f) for f in range(n)]
        assert all(s["bit_errors"] == 0 and s["n_bits"] == 8 * bits.shape[1] for s in stats), stats
        assert np.array_equal(d_out.cpu().numpy(), bits[:n])
    finally:
        rx.close()
        for m in tx:
            m.close()


# --------------------------------------------------------------------------- 4. refusals
def test_refusals_return_invalid_and_leave_the_previous_result_alone(pkg, mods):
    import torch
    x, mode, early, old = TC.named("m1_two")
    md = mods[mode]
    lib, h = md._lib, md._h
    g = geometry(mode)
    fresh = pkg.Modulator(mode=mode, max_frames=2)
    try:
        with pytest.raises(pkg.DabGpuError, match="no TII scan result"):
            fresh.tii_scan_result()
    finally:
        fresh.close()
    _, _, raw, d_x = _scan(md, "m1_two")
    px = d_x.data_ptr()
    d_s16 = torch.zeros(4 * g["tf"], dtype=torch.int16, device="cuda")

    def cfg(early=early, old=0, min_ratio=12.0, min_rel=1e-3):
        c = pkg._TiiScanConfig()
        c.early, c.old_variant, c.min_ratio, c.min_rel = early, old, min_ratio, min_rel
        return C.byref(c)

    def dev(p, fmt, n, c):
        return lib.dabgpu_tii_scan_dev(h, p, fmt, n, c, None)

    host = np.array(x)
    calls = {
        "one frame": (lambda: dev(px, 0, 1, cfg()), "n_frames must lie in 2 ... max_frames"),
        "no frame": (lambda: dev(px, 0, 0, cfg()), "n_frames must lie in 2 ... max_frames"),
        "more than max_frames": (lambda: dev(px, 0, 6, cfg()), "n_frames must lie in 2 ... max_frames"),
        "early below": (lambda: dev(px, 0, 5, cfg(early=-1)), "early must lie in 0 ... null_size - spacing"),
        "early above": (lambda: dev(px, 0, 5, cfg(early=g["null"] - g["N"] + 1)), "early must lie in 0 ... null_size - spacing"),
        "min_ratio below 1": (lambda: dev(px, 0, 5, cfg(min_ratio=0.5)), "min_ratio must be finite and at least 1"),
        "min_ratio nan": (lambda: dev(px, 0, 5, cfg(min_ratio=float("nan"))), "min_ratio must be finite and at least 1"),
        "min_ratio inf": (lambda: dev(px, 0, 5, cfg(min_ratio=float("inf"))), "min_ratio must be finite and at least 1"),
        "min_rel 1": (lambda: dev(px, 0, 5, cfg(min_rel=1.0)), "min_rel must lie in [0, 1)"),
        "min_rel negative": (lambda: dev(px, 0, 5, cfg(min_rel=-0.5)), "min_rel must lie in [0, 1)"),
        "min_rel nan": (lambda: dev(px, 0, 5, cfg(min_rel=float("nan"))), "min_rel must lie in [0, 1)"),
        "u8": (lambda: dev(px, 2, 5, cfg()), "input format is complexf"),
        "s8": (lambda: dev(px, 3, 5, cfg()), "input format is complexf"),
        "null frames": (lambda: dev(None, 0, 5, cfg()), "null argument"),
        "null settings": (lambda: dev(px, 0, 5, None), "null argument"),
        "misaligned": (lambda: dev(px + 4, 0, 4, cfg()), "aligned to a sample"),
        "misaligned s16": (lambda: dev(d_s16.data_ptr() + 2, S16, 2, cfg()), "aligned to a sample"),
        "host form, one frame": (lambda: lib.dabgpu_tii_scan(h, host.ctypes.data, 0, 1, cfg()), "n_frames must lie in 2 ... max_frames"),
        "host form, u8": (lambda: lib.dabgpu_tii_scan(h, host.ctypes.data, 2, 5, cfg()), "input format is complexf"),
        "host form, null": (lambda: lib.dabgpu_tii_scan(h, None, 0, 5, cfg()), "null argument"),
    }
    for name, (call, message) in calls.items():
        assert call() == E_INVALID, name
        assert message in lib.dabgpu_last_error(h).decode(), (name, lib.dabgpu_last_error(h))
        assert md.tii_scan_result_bytes() == raw, name
    with pytest.raises(pkg.DabGpuError):
        md.tii_scan_dev(d_x, 6, early)                                  # (the wrapper: the tensor holds five frames)
    with pytest.raises(pkg.DabGpuError):
        md.tii_scan(host.reshape(-1)[:-1], early)
    for m3 in (3, 4):
        other = pkg.Modulator(mode=m3, max_frames=2)
        try:
            assert other._lib.dabgpu_tii_scan_dev(other._h, px, 0, 2, cfg(early=0), None) == E_INVALID
            assert "only transmission modes I and II carry TII" in other._lib.dabgpu_last_error(other._h).decode()
            with pytest.raises(pkg.DabGpuError, match="no TII scan result"):
                other.tii_scan_result()
        finally:
            other.close()
    assert md.tii_scan_result_bytes() == raw
    head, got, again, _ = _scan(md, "m1_two")                           # a valid call follows
    assert again == raw


# --------------------------------------------------------------------------- 5. between two chain calls
def test_a_scan_between_two_chain_calls_leaves_the_second_calls_bytes_alone(pkg):
    """cfg 3 with TII, one frame per call (the TII parity advances with every call): call, call -> y1, y2; call, scan, call
    on the same context -> the same y1, y2."""
    import torch
    mode = 1
    tf = geometry(mode)["tf"]
    x, _, early, _ = TC.named("m1_single")
    bits = SY.case_bits(mode, 1)
    stages = pkg.STAGE_GAIN | pkg.STAGE_FIR
    md = pkg.Modulator(mode=mode, max_frames=2)
    try:
        md.set_gain(pkg.GAIN_VAR, 1.0, DC.NORMALISE, 4.0)
        md.set_fir_taps(None)
        md.set_tii(True, *TC.A)
        d_bits = torch.from_numpy(bits).cuda()
        d_x = torch.from_numpy(np.array(x[:2])).cuda()
        outs = []
        for scan in (False, True):
            d_y = torch.zeros((2, tf), dtype=torch.complex64, device="cuda")
            md.chain_dev(d_bits[0:1], 1, stages, d_y[0])
            if scan:
                md.tii_scan_dev(d_x, 2, early)
            md.chain_dev(d_bits[1:2], 1, stages, d_y[1])
            torch.cuda.synchronize()
            outs.append(d_y.cpu().numpy())
        head, got = md.tii_scan_result()
        assert head["n_entries"] == 1 and (got[0]["comb"], got[0]["pattern"]) == (3, 5)
        assert outs[0].any() and np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32))
        assert not np.array_equal(outs[0][0, :2656], outs[0][1, :2656])  # (the two calls differ: one null symbol carries TII)
    finally:
        md.close()


# --------------------------------------------------------------------------- 6. dabmod_file --tii-scan
def _dabmod_file(fin, fout, opts):
    exe = os.path.join(ROOT, "odr-dabmod_amd", "host", "dabmod_file")
    return subprocess.run([exe, fin, fout] + opts, capture_output=True, text=True, timeout=300)


@pytest.mark.parametrize("mode, opts, entry, verdict", [
    (1, ["--fir", "default", "--tii", "3,5"], "comb 3 pattern 5 mask 0x27 (4 cells)", "read by the standard as pattern 5: read"),
    (2, ["--format", "s16", "--tii", "3,5"], "comb 3 pattern 32 mask 0x72 (4 cells)", "read by the standard as pattern 32: read"),
    (1, [], None, None),
])
def test_dabmod_file_tii_scan_reads_the_configured_identifier(tmp_path, mode, opts, entry, verdict):
    """Four frames in one batch, the last batch scanned: Mode I with FIRFilter reads (3, 5) at delay -22, Mode II (s16) reads the
    exchanged pattern 32 at delay 0, both exit 0; without --tii there is no entry and nothing to hold it against."""
    fin = str(tmp_path / "in.eti")
    DC.eti_frames(4, mode).tofile(fin)
    r = _dabmod_file(fin, str(tmp_path / "out"), ["--mode", "%d" % mode, "--batch", "4", "--tii-scan"] + opts)
    print(r.stderr[-900:])
    assert r.returncode == 0, r.stderr[-2000:]
    assert "tii: 4 frames scanned, 2 used (parity 0)" in r.stderr
    if entry is None:
        assert "0 entries" in r.stderr and "tii: comb" not in r.stderr and "configured" not in r.stderr
        return
    line = [ln for ln in r.stderr.splitlines() if "tii: comb" in ln]
    assert len(line) == 1 and entry in line[0] and verdict in r.stderr
    assert ("delay -22.000 samples" if "--fir" in opts else "delay +0.000 samples") in line[0]


def test_dabmod_file_refuses_tii_scan_where_there_is_nothing_it_can_read(tmp_path):
    fin = str(tmp_path / "in.eti")
    DC.eti_frames(1, 2).tofile(fin)
    for opts, why in ((["--batch", "4", "--rate", "4096000"], "--rate"), (["--batch", "4", "--format", "u8"], "u8 / s8"),
                      (["--batch", "4", "--format", "s8"], "u8 / s8"), ([], "--batch below 2"), (["--batch", "4", "--bits-only"], "--bits-only")):
        fout = str(tmp_path / "refused")
        r = _dabmod_file(fin, fout, ["--mode", "2", "--tii-scan"] + opts)
        assert r.returncode == 2 and "--tii-scan does not go with " + why in r.stderr and not os.path.exists(fout), (opts, r.stderr[-500:])
