"""The channel emulator on the device (channel.hip; include/dabgpu.h, "the channel"): every case of
tests/channel_cases.py against the float64 model (tests/channel_model.py) below the project's bar for float paths; one stream in
any chunking and run geometry, the same bytes; identity; formats; refusals that queue nothing; set and reset; the whole loop on
device tensors at the operating point tests/test_channel_cpu.py found; multipath and a carrier offset through the synchroniser;
dabmod_file's options."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import channel_cases as CC
from tests import channel_model as CM
from tests import decode_model as M
from tests import soft_cases as SC
from tests.conftest import ROOT, record_bound
from tests.sync_model import extract_slots, geometry, sync_model

pytestmark = pytest.mark.gpu
HOST = os.path.join(ROOT, "odr-dabmod_amd", "host")
E_INVALID = -1
S16 = 1


@pytest.fixture(scope="module")
def md(pkg):
    m = pkg.Modulator(mode=2, max_frames=2)
    yield m
    m.close()


def _run(md, x, lengths=None, out="complexf", position=0, alternate=False):
    """reset at `position`, then the stream x (complex64, or int16 pairs) in calls of these lengths -> the output as numpy.
    alternate: x holds int16 values; every second call gets them as complex64."""
    import torch
    n = x.size // 2 if x.dtype == np.int16 else x.size
    d_x = torch.from_numpy(np.array(x)).cuda()
    d_c = torch.from_numpy(CM.as_samples(x).astype(np.complex64)).cuda() if alternate else None
    d_y = torch.zeros(n, dtype=torch.complex64, device="cuda") if out == "complexf" else torch.zeros(2 * n, dtype=torch.int16, device="cuda")
    md.channel_reset(position)
    at = 0
    for k, m in enumerate(lengths or [n]):
        if alternate and k % 2:
            d_in = d_c[at:at + m]
        else:
            d_in = d_x[2 * at:2 * (at + m)] if x.dtype == np.int16 else d_x[at:at + m]
        d_out = d_y[at:at + m] if out == "complexf" else d_y[2 * at:2 * (at + m)]
        md.channel_dev(d_in, d_out)
        at += m
    assert at == n and md.channel_position() == (position + n) % 2 ** 64
    torch.cuda.synchronize()
    return d_y.cpu().numpy()


def _set(md, c):
    md.set_channel(c["paths"], c["sigma"], c["seed"], c["rate_hz"])


def _block_deviation(got, want, floor=None):
    """worst relative RMS of the difference over the blocks of CC.BLOCK outputs (floor: the RMS to judge against instead)"""
    worst = 0.0
    for b in range(0, want.size, CC.BLOCK):
        w = want[b:b + CC.BLOCK]
        ref = floor if floor is not None else float(np.sqrt(np.mean(np.abs(w) ** 2)))
        assert ref > 0.0
        worst = max(worst, float(np.sqrt(np.mean(np.abs(got[b:b + CC.BLOCK] - w) ** 2))) / ref)
    return worst


# --------------------------------------------------------------------------- 1. against the model
@pytest.mark.parametrize("name", list(CC.KERNEL_CASES))
def test_every_case_follows_the_float64_model(md, name):
    c = CC.kernel_case(name)
    x = CC.signal(c["n"], 1, c["s16"])
    _set(md, c)
    got = _run(md, x, position=c["position"])
    model = CM.Channel(c["paths"], c["sigma"], c["seed"], c["rate_hz"])
    model.reset(c["position"])
    want = model(x)
    assert got.shape == want.shape and np.isfinite(got.view(np.float32)).all()
    dev = _block_deviation(got.astype(np.complex128), want, c["sigma"] * np.sqrt(2.0) if not c["paths"] else None)
    print("%s: worst relative RMS per block of %d: %.3g" % (name, CC.BLOCK, dev))
    assert record_bound("channel against the float64 model, %s" % name, dev, CC.BAR)


# --------------------------------------------------------------------------- 2. one stream, any chunking, the same bytes
def test_any_chunking_and_run_geometry_gives_the_bytes_of_one_call(md):
    c = CC.kernel_case("everything")
    _set(md, c)
    x = CC.signal(CC.N_STREAM, 2)
    q = CC.signal(CC.N_STREAM, 3, s16=True)
    try:
        md.set_channel_run_samples(0)
        whole = _run(md, x, position=CC.STREAM_POSITION)
        whole_q = _run(md, q, position=CC.STREAM_POSITION)
        assert len(np.unique(whole.view(np.uint32))) > CC.N_STREAM
        assert np.array_equal(_run(md, x, position=CC.STREAM_POSITION).view(np.uint32), whole.view(np.uint32))
        for run in CC.RUN_SAMPLES:
            md.set_channel_run_samples(run)
            for name, lengths in CC.splits().items():
                got = _run(md, x, lengths, position=CC.STREAM_POSITION)
                assert np.array_equal(got.view(np.uint32), whole.view(np.uint32)), (run, name)
            got = _run(md, q, CC.splits()["sevens"], position=CC.STREAM_POSITION, alternate=True)
            assert np.array_equal(got.view(np.uint32), whole_q.view(np.uint32)), (run, "alternating formats")
        # the history is handed over by one kernel for every input format: each of them cut into sevens (every call shorter
        # than the history) and at [1, n - 1], at one run geometry
        md.set_channel_run_samples(0)
        for fmt, stream, want in (("complexf", x, whole), ("s16", q, whole_q)):
            for name in ("sevens", "one_rest"):
                got = _run(md, stream, CC.splits()[name], position=CC.STREAM_POSITION)
                assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (fmt, name)
    finally:
        md.set_channel_run_samples(0)


# --------------------------------------------------------------------------- 3. identity
def test_one_path_of_gain_one_without_noise_is_the_input(md):
    md.set_channel([(0, 1.0, 0.0)])
    x = CC.signal(CC.N_BASE, 4)
    assert np.array_equal(_run(md, x), x)
    # the host-pointer form, on a stream of its own position
    md.channel_reset(0)
    assert np.array_equal(md.channel(x[:100]), x[:100]) and md.channel_position() == 100


# --------------------------------------------------------------------------- 4. formats
def test_s16_output_is_the_format_converters_and_s16_input_is_its_values(md):
    import torch
    c = CC.kernel_case("s16_input")
    _set(md, c)
    q = CC.signal(c["n"], 5, s16=True)
    q[:8] = (32767, -32768, 30000, -30000, 1, -1, 0, 12345)
    for gain in (0.1, 3.0):                                            # (0.1: nothing saturates; 3.0: a good share does)
        md.set_channel([(d, g * gain, f) for d, g, f in c["paths"]], c["sigma"], c["seed"], c["rate_hz"])
        y = _run(md, q)
        y16 = _run(md, q, out="s16")
        d_conv = torch.zeros(2 * c["n"], dtype=torch.int16, device="cuda")
        md.format_convert_dev(torch.from_numpy(y).cuda(), "s16", d_conv)
        torch.cuda.synchronize()
        conv = d_conv.cpu().numpy()
        assert np.array_equal(y16, conv), gain
        assert np.array_equal(conv, CM.to_s16(y.astype(np.complex128)))
        saturated = int((np.abs(conv.astype(np.int32)) >= 32767).sum())
        assert saturated > 100 if gain == 3.0 else saturated == 0, (gain, saturated)
        as_float = CM.as_samples(q).astype(np.complex64)
        assert np.array_equal(_run(md, as_float).view(np.uint32), y.view(np.uint32)), gain
        assert np.array_equal(_run(md, as_float, out="s16"), y16), gain


# --------------------------------------------------------------------------- 5. refusals queue nothing
def test_refusals_return_invalid_and_leave_position_output_and_the_next_call_alone(md, pkg):
    import torch
    lib, h = md._lib, md._h
    c = CC.kernel_case("everything")
    x = CC.signal(3000, 6)
    _set(md, c)
    want = _run(md, x, [1000, 2000], position=77)
    d_x = torch.from_numpy(x).cuda()
    d_y = torch.full((3000,), 7.0, dtype=torch.complex64, device="cuda")
    d_b = torch.zeros(64, dtype=torch.uint8, device="cuda")
    md.channel_reset(77)
    md.channel_dev(d_x[:1000], d_y[:1000])
    first = d_y.cpu().numpy().copy()
    px, py = d_x.data_ptr(), d_y.data_ptr()

    def dev(p_in, f_in, n, p_out, f_out):
        return lib.dabgpu_channel_dev(h, p_in, f_in, n, p_out, f_out, None)

    calls = {
        "null input": (lambda: dev(None, 0, 10, py, 0), "null argument"),
        "null output": (lambda: dev(px, 0, 10, None, 0), "null argument"),
        "misaligned input": (lambda: dev(px + 4, 0, 10, py, 0), "aligned to a sample"),
        "misaligned output": (lambda: dev(px, 0, 10, py + 4, 0), "aligned to a sample"),
        "misaligned s16": (lambda: dev(px + 2, S16, 10, py, 0), "aligned to a sample"),
        "no samples": (lambda: dev(px, 0, 0, py, 0), "n_samples must not be 0"),
        "in place": (lambda: dev(py, 0, 10, py, 0), "must not overlap"),
        "overlap": (lambda: dev(py, 0, 100, py + 99 * 8, 0), "must not overlap"),
        "overlap s16": (lambda: dev(py + 396, S16, 100, py, 0), "must not overlap"),
        "u8 input": (lambda: dev(px, 2, 10, py, 0), "formats are complexf"),
        "s8 output": (lambda: dev(px, 0, 10, py, 3), "formats are complexf"),
        "host form, u8": (lambda: lib.dabgpu_channel(h, x.ctypes.data, 2, 10, first.ctypes.data, 0), "formats are complexf"),
        "host form, no samples": (lambda: lib.dabgpu_channel(h, x.ctypes.data, 0, 0, first.ctypes.data, 0), "n_samples must not be 0"),
    }
    for name, (call, message) in calls.items():
        assert call() == E_INVALID, name
        assert message in lib.dabgpu_last_error(h).decode(), (name, lib.dabgpu_last_error(h))
    # the settings: refused by set_channel as by channel_check, the installed configuration stays
    for kw, message in ((dict(paths=[(2048, 1.0, 0.0)]), "delay is 0 ... 2047"), (dict(paths=[], sigma=-1.0), "negative"),
                        (dict(paths=[(0, complex(np.nan, 0), 0.0)]), "finite"), (dict(paths=[], sigma=np.inf), "finite"),
                        (dict(paths=[], rate_hz=0.0), "rate_hz must be positive"),
                        (dict(paths=[(0, 1.0, -1024000.0)]), "below rate_hz / 2")):
        with pytest.raises(pkg.DabGpuError, match=message):
            md.set_channel(**kw)
    cfg = pkg._ChannelConfig()
    cfg.n_paths, cfg.rate_hz = 65, 2048000.0
    assert lib.dabgpu_set_channel(h, C.byref(cfg)) == E_INVALID and b"at most 64 paths" in lib.dabgpu_last_error(h)
    # the wrappers' own checks
    with pytest.raises(pkg.DabGpuError):
        md.channel_dev(d_x[:10], d_y[:11])
    with pytest.raises(pkg.DabGpuError):
        md.channel_dev(d_b[:20], d_y[:10])
    with pytest.raises(pkg.DabGpuError):
        md.channel(np.zeros(10, np.uint8))
    assert md.channel_position() == 77 + 1000
    torch.cuda.synchronize()
    assert np.array_equal(d_y.cpu().numpy().view(np.uint32), first.view(np.uint32))
    md.channel_dev(d_x[1000:], d_y[1000:])
    torch.cuda.synchronize()
    assert np.array_equal(d_y.cpu().numpy().view(np.uint32), want.view(np.uint32))
    # a context without a configuration
    fresh = pkg.Modulator(mode=3, max_frames=1)
    try:
        with pytest.raises(pkg.DabGpuError, match="no configuration"):
            fresh.channel_dev(d_x[:10], d_y[:10])
        with pytest.raises(pkg.DabGpuError, match="no configuration"):
            fresh.channel(x[:10])
        assert fresh.channel_position() == 0
    finally:
        fresh.close()


# --------------------------------------------------------------------------- 6. set and reset
def test_a_new_configuration_affects_the_next_call_only_and_a_reset_zeroes_the_history(md):
    import torch
    x = CC.signal(6000, 8)
    a, b = CC.kernel_case("everything"), CC.kernel_case("paths64")
    model = CM.Channel(a["paths"], a["sigma"], a["seed"])
    want1 = model(x[:3000])
    model.set(b["paths"], 0.2, 99)                                     # history and position stay
    want2 = model(x[3000:])
    d_x = torch.from_numpy(x).cuda()
    d_y = torch.zeros(6000, dtype=torch.complex64, device="cuda")
    ts = torch.cuda.Stream()
    torch.cuda.synchronize()
    md.channel_reset(0)
    _set(md, a)
    md.channel_dev(d_x[:3000], d_y[:3000], stream=ts.cuda_stream)      # queued; the new table must not reach it
    md.set_channel(b["paths"], 0.2, 99)
    md.channel_dev(d_x[3000:], d_y[3000:], stream=ts.cuda_stream)
    ts.synchronize()
    got = d_y.cpu().numpy().astype(np.complex128)
    assert _block_deviation(got[:3000], want1) < CC.BAR and _block_deviation(got[3000:], want2) < CC.BAR
    assert md.channel_position() == 6000
    # reset: a delayed path alone, with noise -- the first 2047 outputs are the noise alone, whatever came before
    md.set_channel([(2047, 1.0, 0.0)], 0.25, 5)
    y = _run(md, x[:4096], position=6000)
    noise = 0.25 * CM.unit_noise(5, 6000, 4096)
    assert _block_deviation(y[:2047].astype(np.complex128), noise[:2047], 0.25 * np.sqrt(2.0)) < CC.BAR
    assert _block_deviation(y[2047:].astype(np.complex128), noise[2047:] + x[:2049], None) < CC.BAR


# --------------------------------------------------------------------------- 7. the loop, on device tensors throughout
def test_at_the_operating_point_the_soft_loop_decodes_what_the_hard_loop_loses(pkg):
    """ETI -> chain_eti (cfg 3) -> channel_dev at the recorded level and seed -> demod_dev / demod_soft_dev -> decode_dev /
    decode_soft_dev: the hard loop has a payload bit error in every returned frame, the soft loop none, at L and 1 dB below."""
    import torch
    eti, bits, ref = SC.op_stream()
    n = SC.OP_FRAMES
    m = pkg.Modulator(mode=SC.OP_MODE, max_frames=n)
    try:
        m.set_gain(2, 1.0, 1.0 / 50000.0, 4.0)
        m.set_fir_taps(None)
        m.frontend_configure(eti[0])
        per = m.geometry["tf_input_bytes"]
        d_eti = torch.from_numpy(eti).cuda()
        d_cod = torch.zeros((n, per), dtype=torch.uint8, device="cuda")
        d_iq = torch.zeros(n * m.geometry["tf_samples"], dtype=torch.complex64, device="cuda")
        m.chain_eti_dev_queued(d_eti, eti.shape[0], 3, d_cod, d_iq)
        m.synchronize()
        power = CC.data_power(d_iq.cpu().numpy(), SC.OP_MODE)
        d_rx = torch.zeros_like(d_iq)
        d_bits = torch.zeros((n, per), dtype=torch.uint8, device="cuda")
        d_soft = torch.zeros((n, 8 * per), dtype=torch.int8, device="cuda")
        d_ref = torch.from_numpy(ref).cuda()
        d_out = torch.zeros(n * 6144, dtype=torch.uint8, device="cuda")
        keep = M.payload_mask(pkg.Modulator.frontend_describe(eti[0]))
        for back in (0.0, 1.0):
            m.set_channel([(0, 1.0, 0.0)], pkg.channel_sigma(power, CC.OP_LEVEL_DB - back), CC.OP_SEED)
            m.channel_reset(0)
            m.decode_reset()
            m.channel_dev(d_iq, d_rx)
            m.demod_dev(d_rx, n, SC.OP_EARLY, d_bits)
            m.decode_dev(d_bits, n, d_out, d_ref)
            hard = [m.decode_stats(i)["bit_errors"] for i in range(15, n)]
            m.demod_soft_dev(d_rx, n, d_soft, SC.OP_EARLY)
            m.decode_soft_dev(d_soft, n, d_out, d_ref)
            torch.cuda.synchronize()
            soft = [m.decode_soft_stats(i) for i in range(15, n)]
            print("C/N %.1f dB, seed %d: hard payload bit errors %s, soft %s" % (CC.OP_LEVEL_DB - back, CC.OP_SEED, hard, [s["bit_errors"] for s in soft]))
            assert all(e > 0 for e in hard)
            assert all(s["bit_errors"] == 0 and s["n_bits"] > 0 for s in soft)
            images = d_out.cpu().numpy().reshape(n, 6144)
            assert np.array_equal(images[15:][:, keep], eti[:n - 15][:, keep])
    finally:
        m.close()


# --------------------------------------------------------------------------- 8. multipath and carrier offset through the synchroniser
@pytest.mark.parametrize("name", sorted(CC.CAPTURES))
def test_two_paths_and_a_carrier_offset_through_the_synchroniser(pkg, name):
    """channel_dev -> sync_dev -> sync_extract_dev -> demod_dev: the integers of tests/sync_model.py on the channel model's
    output, shift + eps within 1e-3 spacings of the offset, no bit error."""
    import torch
    x, mode, bits, _ = CC.capture_input(name)
    early = CC.CAPTURES[name][9]
    paths, sigma, seed = CC.capture_channel(name, pkg.channel_sigma)
    want = sync_model(CM.Channel(paths, sigma, seed)(x), mode, 31, 2)
    m = pkg.Modulator(mode=mode, max_frames=2)
    try:
        m.set_channel(paths, sigma, seed)
        d_x = torch.from_numpy(np.array(x)).cuda()
        d_y = torch.zeros_like(d_x)
        m.channel_dev(d_x, d_y)
        m.sync_dev(d_y, 31)
        d_frames = torch.zeros((extract_slots(x.size, mode, 2), geometry(mode)["tf"]), dtype=torch.complex64, device="cuda")
        m.sync_extract_dev(d_y, d_frames)
        got = m.sync_result()
        assert len(got) == want["n_frames"] == 2
        for k, (a, b) in enumerate(zip(got, want["frames"])):
            assert (a["start"], a["shift"], a["valid"]) == (b["start"], b["shift"], b["valid"]), (k, a, b)
            assert a["valid"] == 1 and abs(a["shift"] + a["eps"] - CC.CFO) <= 1e-3, (k, a)
        d_bits = torch.zeros((2, m.geometry["tf_input_bytes"]), dtype=torch.uint8, device="cuda")
        m.demod_dev(d_frames[:2].contiguous(), 2, early, d_bits, torch.from_numpy(bits.copy()).cuda())
        torch.cuda.synchronize()
        stats = [m.monitor_stats(f) for f in range(2)]
        print("%s: starts %s, shift + eps %s, bit errors %s" % (name, [a["start"] for a in got], [a["shift"] + a["eps"] for a in got],
                                                                [s["bit_errors"] for s in stats]))
        assert all(s["bit_errors"] == 0 and s["n_bits"] == 8 * bits.shape[1] for s in stats)
        assert np.array_equal(d_bits.cpu().numpy(), bits)
    finally:
        m.close()


# --------------------------------------------------------------------------- 9. dabmod_file
def _dabmod_file(fin, fout, opts):
    return subprocess.run([os.path.join(HOST, "dabmod_file"), fin, fout] + opts, capture_output=True, text=True, timeout=300)


def test_dabmod_file_channel_options(tmp_path):
    """--gpu-frontend --loopback --soft --channel-cn at the recorded level decodes (exit 0) with a non-zero metric; without
    --soft the hard loop loses bits (exit 2); an echo beyond the cyclic prefix less `early` is refused."""
    from tests import decode_cases as K
    fin = str(tmp_path / "in.eti")
    eti, _ = K.stream(SC.OP_FRAMES, SC.OP_SUBCHANNELS, SC.OP_MODE)
    eti.tofile(fin)
    base = ["--gpu-frontend", "--mode", "%d" % SC.OP_MODE, "--batch", "%d" % SC.OP_FRAMES, "--fir", "default", "--loopback", "--channel-cn", "%.1f" % CC.OP_LEVEL_DB, "--channel-seed", "%d" % CC.OP_SEED]
    r = _dabmod_file(fin, str(tmp_path / "soft"), base + ["--soft"])
    print(r.stderr[-600:])
    assert r.returncode == 0, r.stderr[-2000:]
    line = [ln for ln in r.stderr.splitlines() if "soft decisions" in ln][0]
    assert int(line.split("metric ")[1].split(" ")[0]) > 0
    assert "channel: C/N %.1f dB, seed %d, 1 path" % (CC.OP_LEVEL_DB, CC.OP_SEED) in r.stderr
    r = _dabmod_file(fin, str(tmp_path / "hard"), base)
    assert r.returncode == 2, r.stderr[-2000:]
    r = _dabmod_file(fin, str(tmp_path / "echo"), base + ["--soft", "--channel-echo", "30,-6,1.0"])
    assert r.returncode in (0, 2) and "channel: C/N %.1f dB, seed %d, 2 paths" % (CC.OP_LEVEL_DB, CC.OP_SEED) in r.stderr
    fout = str(tmp_path / "refused")
    r = _dabmod_file(fin, fout, base + ["--soft", "--channel-echo", "%d,-6,1.0" % (126 - 44 + 1)])
    assert r.returncode == 1 and "--channel-echo: a delay of 83 samples lies beyond the cyclic prefix less the window's lead (82)" in r.stderr
    r = _dabmod_file(fin, fout + "2", ["--gpu-frontend", "--mode", "2", "--channel-cn", "5"])
    assert r.returncode == 2 and "--channel-cn" in r.stderr and not os.path.exists(fout + "2")
