"""The receiver on the device (demod.hip; include/dabgpu.h, "the receiver"): the chain's output decoded back to the coded bits
byte for byte, the run geometry, counted bit errors, the quality sums against the float64 model, the monitor that rides on a
chain call, and dabmod_file --monitor.  The inputs are those tests/test_demod_cpu.py checks for margin on the oracle's chains."""
import os
import subprocess

import numpy as np
import pytest

from tests import demod_cases as DC
from tests.conftest import ROOT, record_bound
from tests.demod_model import demod_model, mer_db
from tests.golden.synth import synth_eti
from tests.receiver import dab_demodulate

pytestmark = pytest.mark.gpu
HOST = os.path.join(ROOT, "odr-dabmod_amd", "host")

# Relative deviation of the device's sums from the float64 model on the same noisy samples (chain output plus complex Gaussian
# noise 20 dB below it), three frames per mode.  Measured on the device, worst over modes I - IV (profiles/r06_measured_bounds.jsonl):
# sum_signal 1.036e-7 (Mode I), sum_quadrature 1.128e-7 (Mode II); each bar is four times its worst value, the margin for
# box-to-box variation in clock and atomic ordering.  (The fp32 transform's own error is 1.1e-7.)
BAR_SIGNAL = 4 * 1.036e-7
BAR_QUADRATURE = 4 * 1.128e-7


def _chain(pkg, md, bits, stages, s16=False):
    import torch
    n = bits.shape[0]
    ns = md.out_samples_per_frame(stages)
    out = torch.empty((n, 2 * ns) if s16 else (n, ns), dtype=torch.int16 if s16 else torch.complex64, device="cuda")
    md.chain_dev(torch.from_numpy(bits.copy()).cuda(), n, stages, out)
    return out


def _demod(md, d_iq, n, early, ref=None):
    import torch
    d_bits = torch.zeros((n, md.geometry["tf_input_bytes"]), dtype=torch.uint8, device="cuda")
    d_ref = torch.from_numpy(np.ascontiguousarray(ref)).cuda() if ref is not None else None
    md.demod_dev(d_iq, n, early, d_bits, d_ref)
    torch.cuda.synchronize()
    return d_bits.cpu().numpy(), [md.monitor_stats(f) for f in range(n)]


def _noisy(y, mode, seed):
    """y (frames x samples, complex64) plus complex Gaussian noise 20 dB below the data symbols' power, as complex64."""
    rs = np.random.RandomState(seed)
    null = {1: 2656, 2: 664, 3: 345, 4: 1328}[mode]
    p = float(np.mean(np.abs(y[:, null:].astype(np.complex128)) ** 2))
    sigma = np.sqrt(p / 100.0 / 2.0)
    return (y + sigma * (rs.randn(*y.shape) + 1j * rs.randn(*y.shape))).astype(np.complex64)


# --------------------------------------------------------------------------- 1. round trip
@pytest.mark.parametrize("mode", [1, 2, 3, 4])
def test_round_trip_equals_the_input_bits_and_the_numpy_receiver(pkg, mode):
    """cfg 2, three frames, early 0 / 1 / the whole cyclic prefix; then cfg 3 at early 44 as complexf and as s16.  Mode III is
    the 32-lane workgroup, Mode I has bin K/2 on lane 0 beside the skipped DC bin, frames 1 and 2 the frame offsets."""
    md = pkg.Modulator(mode=mode, max_frames=3)
    try:
        per = md.geometry["tf_input_bytes"]
        bits = DC.case_bits(mode, 3, per)
        d_y = _chain(pkg, md, bits, 0)
        y = d_y.cpu().numpy()
        for early in (0, 1, DC.CP[mode]):
            got, st = _demod(md, d_y, 3, early, ref=bits)
            assert np.array_equal(got, bits), (mode, early)
            for f in range(3):
                assert np.array_equal(got[f], dab_demodulate(y[f], mode, early)), (mode, early, f)
                assert st[f]["bit_errors"] == 0 and st[f]["n_bits"] == 8 * per
                assert st[f]["min_margin"] > 0.7
        md.set_gain(2, 1.0, DC.NORMALISE, 4.0)
        stages = pkg.STAGE_GAIN | pkg.STAGE_FIR
        d_y = _chain(pkg, md, bits, stages)
        y = d_y.cpu().numpy()
        got, st = _demod(md, d_y, 3, 44)
        assert np.array_equal(got, bits) and all(s["n_bits"] == 0 and s["bit_errors"] == 0 for s in st)
        for f in range(3):
            assert np.array_equal(got[f], dab_demodulate(y[f], mode, 44)), (mode, f)
        md.set_gain(2, 1.0, 1.0, 4.0)
        md.set_output_format("s16")
        d_q = _chain(pkg, md, bits, stages, s16=True)
        got, st = _demod(md, d_q, 3, 44, ref=bits)
        assert np.array_equal(got, bits) and all(s["bit_errors"] == 0 for s in st)
        # the host-pointer form, on the same integers
        assert np.array_equal(md.demod(d_q.cpu().numpy(), 44, ref_bits=bits), bits)
        assert md.monitor_stats(2)["bit_errors"] == 0
    finally:
        md.close()


def test_early_outside_the_cyclic_prefix_and_other_formats_are_refused(pkg):
    import torch
    md = pkg.Modulator(mode=3, max_frames=1)
    try:
        d_y = torch.zeros(md.geometry["tf_samples"], dtype=torch.complex64, device="cuda")
        for bad in (-1, 64):
            with pytest.raises(pkg.DabGpuError) as e:
                md.demod_dev(d_y, 1, bad)
            assert "cyclic prefix" in str(e.value)
        with pytest.raises(pkg.DabGpuError):
            md.demod(np.zeros(2 * md.geometry["tf_samples"], np.int8))
        with pytest.raises(pkg.DabGpuError) as e:
            md.monitor_stats(0)
        assert "no demodulator statistics" in str(e.value)
    finally:
        md.close()


# --------------------------------------------------------------------------- 2. run geometry
@pytest.mark.parametrize("mode", [1, 3])
def test_run_geometry_gives_the_same_bits_and_the_same_sums(pkg, mode):
    """Symbols per workgroup forced to 1, 2, 7 (divides neither 75 nor 152) and the whole frame: the clean output decodes to
    the input bits, the noisy one to the same bits every time, and its sums stay within the bars of the quality test.  The
    same with the noisy frames as s16 (scaled into the format's range and truncated, as test_clock_gpu.py does): the same
    bytes at every geometry and on repetition."""
    import torch
    md = pkg.Modulator(mode=mode, max_frames=3)
    try:
        per = md.geometry["tf_input_bytes"]
        nblocks = md.geometry["nb_symbols"] - 1
        bits = DC.case_bits(mode, 3, per)
        d_y = _chain(pkg, md, bits, 0)
        noisy = _noisy(d_y.cpu().numpy(), mode, 40 + mode)
        scale = 20000.0 / float(np.abs(noisy.view(np.float32)).max())
        q = np.trunc(noisy.view(np.float32).reshape(3, -1) * scale).astype(np.int16)
        for fmt, d_n in (("complexf", torch.from_numpy(noisy).cuda()), ("s16", torch.from_numpy(q).cuda())):
            first = None
            for spr in (1, 2, 7, nblocks):
                assert nblocks % 7
                md.set_demod_run_symbols(spr)
                if fmt == "complexf":
                    got, _ = _demod(md, d_y, 3, 0, ref=bits)
                    assert np.array_equal(got, bits), spr
                nb, st = _demod(md, d_n, 3, 0, ref=bits)
                if first is None:
                    first = (nb, st)
                if fmt == "s16":
                    again, st2 = _demod(md, d_n, 3, 0, ref=bits)
                    assert np.array_equal(again, nb), spr
                    assert [s["bit_errors"] for s in st2] == [s["bit_errors"] for s in st], spr
                assert np.array_equal(nb, first[0]), (fmt, spr)
                for f in range(3):
                    assert st[f]["bit_errors"] == first[1][f]["bit_errors"]
                    assert st[f]["min_margin"] == first[1][f]["min_margin"]
                    assert abs(st[f]["sum_signal"] / first[1][f]["sum_signal"] - 1.0) <= BAR_SIGNAL
                    assert abs(st[f]["sum_quadrature"] / first[1][f]["sum_quadrature"] - 1.0) <= BAR_QUADRATURE
    finally:
        md.close()


# --------------------------------------------------------------------------- 3. counted errors
def test_bit_errors_are_counted_against_the_reference_bits(pkg):
    """Bits B' that differ from B in 1000 seeded positions per frame, the first and the last data block among them: with B as
    the reference every frame counts 1000 errors in 8 x tf_input_bytes bits, and the decoded bytes are B'."""
    md = pkg.Modulator(mode=1, max_frames=3)
    try:
        per = md.geometry["tf_input_bytes"]
        block_bits = 8 * per // (md.geometry["nb_symbols"] - 1)
        bits = DC.case_bits(1, 3, per)
        other = bits.copy()
        rs = np.random.RandomState(99)
        for f in range(3):
            pos = rs.choice(8 * per, 1000, replace=False)
            pos[:4] = (0, block_bits - 1, 8 * per - block_bits, 8 * per - 1)      # first and last block, both ends
            pos = np.unique(pos)
            while pos.size < 1000:
                pos = np.unique(np.concatenate([pos, rs.choice(8 * per, 1000 - pos.size)]))
            flip = np.zeros(8 * per, np.uint8)
            flip[pos] = 1
            other[f] ^= np.packbits(flip)
            assert int(np.unpackbits(other[f] ^ bits[f]).sum()) == 1000
        d_y = _chain(pkg, md, other, 0)
        got, st = _demod(md, d_y, 3, 0, ref=bits)
        assert np.array_equal(got, other)
        for f in range(3):
            assert st[f]["bit_errors"] == 1000 and st[f]["n_bits"] == 8 * per, (f, st[f])
    finally:
        md.close()


# --------------------------------------------------------------------------- 4. quality sums
@pytest.mark.parametrize("mode", [1, 2, 3, 4])
def test_quality_sums_follow_the_float64_model_on_a_noisy_signal(pkg, mode):
    import torch
    md = pkg.Modulator(mode=mode, max_frames=3)
    try:
        per = md.geometry["tf_input_bytes"]
        bits = DC.case_bits(mode, 3, per)
        noisy = _noisy(_chain(pkg, md, bits, 0).cpu().numpy(), mode, 40 + mode)
        _, st = _demod(md, torch.from_numpy(noisy).cuda(), 3, 0, ref=bits)
        dev_s = dev_q = 0.0
        for f in range(3):
            want = demod_model(noisy[f], mode, 0, ref_bits=bits[f])
            dev_s = max(dev_s, abs(st[f]["sum_signal"] / want["sum_signal"] - 1.0))
            dev_q = max(dev_q, abs(st[f]["sum_quadrature"] / want["sum_quadrature"] - 1.0))
            assert abs(st[f]["min_margin"] - want["min_margin"]) <= 1e-4 + 1e-3 * want["min_margin"], (f, st[f], want["min_margin"])
            print("mode %d frame %d: MER %.3f dB (model %.3f), errors %d (model %d)"
                  % (mode, f, st[f]["mer_db"], mer_db(want), st[f]["bit_errors"], want["bit_errors"]))
        print("mode %d: relative deviation sum_signal %.3g, sum_quadrature %.3g" % (mode, dev_s, dev_q))
        ok_s = record_bound("demod sum_signal vs float64 model, mode %d" % mode, dev_s, BAR_SIGNAL)
        ok_q = record_bound("demod sum_quadrature vs float64 model, mode %d" % mode, dev_q, BAR_QUADRATURE)
        assert ok_s and ok_q, (dev_s, dev_q)
    finally:
        md.close()


# --------------------------------------------------------------------------- 5. the monitor
def _monitored_pair(pkg, name, run):
    """run(md) -> output bytes, on two fresh contexts configured alike: the monitor off, then on.  Returns both outputs, both
    traces and the monitored context (still open: the caller closes it)."""
    outs, traces = [], []
    md = None
    for on in (False, True):
        if md is not None:
            md.close()
        md = pkg.Modulator(mode=1, max_frames=5)
        stages = DC.configure(pkg, md, name)
        md.set_monitor(on)
        md.trace(True)
        outs.append(np.ascontiguousarray(run(md, stages)).view(np.uint8).copy())
        traces.append(md.last_variant())
    return outs, traces, md


@pytest.mark.parametrize("name", sorted(DC.MONITOR_CASES))
def test_monitor_counts_no_error_and_leaves_the_iq_alone(pkg, name):
    bits = DC.case_bits(1, 5, 28800)
    outs, traces, md = _monitored_pair(pkg, name, lambda m, stages: m.chain(bits, stages))
    try:
        assert np.array_equal(outs[0], outs[1])
        assert traces[1][:-1] == traces[0] and len(traces[1]) == len(traces[0]) + 1, traces
        assert traces[1][-1].startswith("demod_kernel<11>") and not any("demod" in k for k in traces[0])
        st = [md.monitor_stats(f) for f in range(5)]
        assert all(s["bit_errors"] == 0 and s["n_bits"] == 8 * 28800 for s in st), st
        print("%s: MER of the clean output %s dB, worst margin %.4f"
              % (name, " ".join("%.2f" % s["mer_db"] for s in st), min(s["min_margin"] for s in st)))
        with pytest.raises(pkg.DabGpuError):
            md.monitor_stats(5)
    finally:
        md.close()


def test_monitor_off_leaves_the_cfg3_trace_as_it_is(pkg):
    md = pkg.Modulator(mode=1, max_frames=5)
    try:
        stages = DC.configure(pkg, md, "cfg3")
        md.trace(True)
        md.chain(DC.case_bits(1, 5, 28800), stages)
        tr = md.last_variant()
        assert len(tr) == 1 and tr[0].startswith("tf_kernel<logn=11 bits=1 gain=1 guard=1 fir=1 nt=45 cfr=0"), tr
        md.set_monitor(True)
        md.set_monitor(False)
        md.chain(DC.case_bits(1, 5, 28800), stages)
        assert md.last_variant() == tr
    finally:
        md.close()


def test_monitor_on_the_eti_entry_uses_the_front_ends_bits(pkg):
    eti = DC.eti_frames(5)

    def run(md, stages):
        md.frontend_configure(eti[0])
        return md.chain_eti(eti, stages)

    outs, traces, md = _monitored_pair(pkg, "cfg3", run)
    try:
        assert np.array_equal(outs[0], outs[1])
        assert len(traces[1]) == len(traces[0]) + 1 and traces[1][-1].startswith("demod_kernel<11>")
        assert all(md.monitor_stats(f)["bit_errors"] == 0 and md.monitor_stats(f)["n_bits"] == 8 * 28800 for f in range(5))
    finally:
        md.close()


def test_monitor_on_a_two_lane_context_stays_on_lane_0(pkg):
    import torch
    bits = DC.case_bits(1, 5, 28800)
    outs = []
    md = None
    try:
        for on in (False, True):
            if md is not None:
                md.close()
            md = pkg.Modulator(mode=1, max_frames=5)
            md.set_lanes(2)
            stages = DC.configure(pkg, md, "cfg3")
            md.set_monitor(on)
            d_bits = torch.from_numpy(bits.copy()).cuda()
            torch.cuda.synchronize()
            d_out = [torch.empty((5, md.out_samples_per_frame(stages)), dtype=torch.complex64, device="cuda") for _ in range(2)]
            for o in d_out:                      # two calls in a row: with the monitor off they rotate over the lanes
                md.chain_dev_queued(d_bits, 5, stages, o)
            md.synchronize()
            outs.append([o.cpu().numpy() for o in d_out])
        for k in range(2):
            assert np.array_equal(outs[0][k].view(np.uint8), outs[1][k].view(np.uint8))
        assert all(md.monitor_stats(f)["bit_errors"] == 0 and md.monitor_stats(f)["n_bits"] == 8 * 28800 for f in range(5))
        assert md.lanes_info()[0] == 1          # (no second lane was ever created by the monitored calls)
    finally:
        if md is not None:
            md.close()


def test_monitor_refuses_what_it_cannot_decode_and_leaves_state_and_statistics_alone(pkg):
    bits = DC.case_bits(1, 5, 28800)
    md = pkg.Modulator(mode=1, max_frames=5)
    try:
        stages = DC.configure(pkg, md, "cfg3")
        md.set_resampler(2048000, 4096000)
        md.set_monitor(True)
        md.chain(bits, stages)                   # (no Resampler in the mask: monitored)
        before = [md.monitor_stats(f) for f in range(5)]
        state = md.stream_state()
        with pytest.raises(pkg.DabGpuError) as e:
            md.chain(bits, stages | pkg.STAGE_RESAMPLE)
        assert "Resampler is not monitored" in str(e.value)
        with pytest.raises(pkg.DabGpuError) as e:
            md.submit(bits, stages)
        assert "dabgpu_chain_submit* is not monitored" in str(e.value)
        md.set_output_format("u8")
        with pytest.raises(pkg.DabGpuError) as e:
            md.chain(bits, stages)
        assert "u8 / s8 output is not monitored" in str(e.value)
        md.set_output_format(None)
        assert md.stream_state() == state
        assert [md.monitor_stats(f) for f in range(5)] == before
        with pytest.raises(pkg.DabGpuError) as e:
            md.set_monitor(True, 505)            # (the setter's own range test)
        assert "cyclic prefix" in str(e.value)
    finally:
        md.close()


# --------------------------------------------------------------------------- 6. dabmod_file --monitor
@pytest.mark.parametrize("extra", [[], ["--gpu-frontend", "--batch", "32"], ["--batch", "4", "--contexts", "2"]])
def test_dabmod_file_monitor_prints_totals_and_writes_the_same_file(tmp_path, extra):
    fin = str(tmp_path / "in.eti")
    synth_eti(40).tofile(fin)                    # ten transmission frames
    opts = ["--fir", "default", "--normalise", str(1.0 / 50000.0)] + extra
    outs = []
    for mon in ([], ["--monitor"]):
        fout = str(tmp_path / ("out%d" % len(outs)))
        r = subprocess.run([os.path.join(HOST, "dabmod_file"), fin, fout] + opts + mon, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        assert r.stdout.split() == ["40", "10", "10"]
        outs.append(np.fromfile(fout, np.uint8))
        assert ("monitor: 10 frames decoded, 0 bit errors in %d bits, MER worst" % (10 * 8 * 28800) in r.stderr) == bool(mon), r.stderr
    assert outs[0].size == 10 * 196608 * 8 and np.array_equal(outs[0], outs[1])
