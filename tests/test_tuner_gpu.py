"""The tuner on the device (tuner.hip; include/dabgpu.h, "the tuner"): every case of tests/tuner_cases.py against
the float64 model (tests/tuner_model.py) below the project's bar for float paths; one stream in any chunking and run geometry,
the same bytes and the same counts; positions and formats; refusals that queue nothing; the whole loop on device tensors --
resampled chain, interferers, tuner, synchroniser, receiver -- at the operating points tests/test_tuner_cpu.py establishes;
queued calls behind the lanes."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import tuner_cases as TC
from tests import tuner_model as TM
from tests.conftest import load_pkg, record_bound

pytestmark = pytest.mark.gpu
E_INVALID, E_CAPACITY = -1, -4
S16, U8, S8 = 1, 2, 3


@pytest.fixture(scope="module")
def pkg():
    return load_pkg()


@pytest.fixture(scope="module", params=[2, 3], ids=["mode2", "mode3"])
def md(pkg, request):
    m = pkg.Modulator(mode=request.param, max_frames=2)
    yield m
    m.close()


@pytest.fixture(scope="module")
def md2(pkg):
    m = pkg.Modulator(mode=2, max_frames=2)
    yield m
    m.close()


def _n(x):
    return x.size if x.dtype == np.complex64 else x.size // 2


def _run(md, pkg, setting, x, lengths=None, out="complexf", position=0):
    """reset at `position`, then the stream x (complex64, or integer pairs) in calls of these lengths -> (the outputs joined, as
    numpy; the counts of the calls).  setting: (in_rate, selectivity), for the capacities."""
    import torch
    n = _n(x)
    w = 1 if x.dtype == np.complex64 else 2
    d_x = torch.from_numpy(np.array(x)).cuda()
    cap = pkg.tuner_out_max(setting[0], setting[1], n) + len(lengths or [0]) + 8
    d_y = torch.zeros(cap, dtype=torch.complex64, device="cuda") if out == "complexf" else torch.zeros(2 * cap, dtype=torch.int16, device="cuda")
    wo = 1 if out == "complexf" else 2
    md.tuner_reset(position)
    at, made, counts = 0, 0, []
    for m in lengths or [n]:
        room = pkg.tuner_out_max(setting[0], setting[1], m)
        got = md.tuner_dev(d_x[w * at:w * (at + m)], d_y[wo * made:wo * (made + room)])
        counts.append(got)
        at += m
        made += got
    assert at == n and md.tuner_position() == position + n
    torch.cuda.synchronize()
    y = d_y.cpu().numpy()
    assert not y[wo * made:].any()                                      # nothing behind the counts was written
    return y[:wo * made], counts


@functools.lru_cache(maxsize=None)
def _model(pkg, rate, sel, off, seed, position=0, n=TC.N_STREAM):
    """the model's outputs for TC.signal(n, seed), once per process"""
    y, counts = TM.run(pkg, rate, sel, off, TC.signal(n, seed), position=position)
    y.setflags(write=False)
    return y, counts


def _block_error(got, want, x_rms):
    """worst RMS of the difference per block of TC.BLOCK outputs, relative to the input's RMS"""
    d = np.abs(got.astype(np.complex128) - want)
    return max(float(np.sqrt(np.mean(d[b:b + TC.BLOCK] ** 2))) for b in range(0, want.size, TC.BLOCK)) / x_rms


# --------------------------------------------------------------------------- 1. against the model
@pytest.mark.parametrize("name", list(TC.KERNEL_CASES))
def test_every_case_follows_the_float64_model(md, pkg, name):
    """Worst RMS of the difference per block of 2048 outputs, held to 1e-6 of the input's RMS (a decimator legitimately drops
    most of a white input's power).  Expected from P roundings of 2^-24 on partial sums: 2e-7 at P = 128, 6e-7 at P = 768."""
    rate, sel, off = TC.KERNEL_CASES[name]
    x = TC.signal(TC.N_STREAM, 1)
    want, want_counts = _model(pkg, rate, sel, off, 1)
    md.set_tuner(rate, sel, off)
    got, counts = _run(md, pkg, (rate, sel), x)
    assert counts == want_counts == [pkg.tuner_count(rate, sel, TC.N_STREAM)]
    assert got.shape == want.shape and np.isfinite(got.view(np.float32)).all()
    x_rms = float(np.sqrt(np.mean(np.abs(x.astype(np.complex128)) ** 2)))
    dev = _block_error(got, want, x_rms)
    print("%s: %d outputs, P = %d, worst RMS of the error per block of %d: %.3g of the input's RMS"
          % (name, want.size, pkg.tuner_geometry(rate, sel)[2], TC.BLOCK, dev))
    assert record_bound("tuner against the float64 model, %s" % name, dev, TC.BAR)


# --------------------------------------------------------------------------- 2. one stream, any chunking, the same bytes
@pytest.mark.parametrize("name", list(TC.STREAM_CASES))
def test_any_chunking_and_run_geometry_gives_the_bytes_and_counts_of_one_call(md2, pkg, name):
    md = md2
    rate, sel, off = TC.STREAM_CASES[name]
    P = pkg.tuner_geometry(rate, sel)[2]
    md.set_tuner(rate, sel, off)
    x = TC.signal(TC.N_STREAM, 2)
    position = TC.STREAM_POSITION
    try:
        md.set_tuner_run_samples(0)
        whole, counts = _run(md, pkg, (rate, sel), x, position=position)
        total = pkg.tuner_count(rate, sel, position + TC.N_STREAM) - pkg.tuner_count(rate, sel, position)
        assert counts == [total] and len(np.unique(whole.view(np.uint32))) > total
        want = TM.run(pkg, rate, sel, off, x, position=position)[0]
        assert _block_error(whole, want, np.sqrt(2.0)) <= TC.BAR
        for run in TC.RUN_SAMPLES:
            md.set_tuner_run_samples(run)
            for split, lengths in TC.splits(P).items():
                got, counts = _run(md, pkg, (rate, sel), x, lengths, position=position)
                assert np.array_equal(got.view(np.uint32), whole.view(np.uint32)), (run, split)
                at, expect = position, []
                for m in lengths:
                    expect.append(pkg.tuner_count(rate, sel, at + m) - pkg.tuner_count(rate, sel, at))
                    at += m
                assert counts == expect, (run, split)
        # the history is handed over by one kernel for every input format: each of them cut into sevens (every call shorter
        # than the history) and at [1, n - 1], at one run geometry
        md.set_tuner_run_samples(0)
        streams = {"complexf": x, "s16": TC.signal(TC.N_STREAM, 3, s16=True), "u8": TC.signal_u8(TC.N_STREAM, 4),
                   "s8": TC.signal_u8(TC.N_STREAM, 5, signed=True)}
        for fmt, stream in streams.items():
            want, _ = _run(md, pkg, (rate, sel), stream, position=position)
            assert len(np.unique(want.view(np.uint32))) > total // 2, fmt
            for split in ("sevens", "one_rest"):
                got, _ = _run(md, pkg, (rate, sel), stream, TC.splits(P)[split], position=position)
                assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (fmt, split)
    finally:
        md.set_tuner_run_samples(0)


# --------------------------------------------------------------------------- 3. positions and formats
@pytest.mark.parametrize("name", list(TC.POSITION_CASES))
def test_a_reset_position_moves_outputs_and_mixer_phase_as_the_model_says(md, pkg, name):
    rate, sel, off, position = TC.POSITION_CASES[name]
    x = TC.signal(TC.N_POSITION, 3)
    want, want_counts = _model(pkg, rate, sel, off, 3, position, TC.N_POSITION)
    md.set_tuner(rate, sel, off)
    got, counts = _run(md, pkg, (rate, sel), x, position=position)
    assert counts == want_counts and want.size > 0
    dev = _block_error(got, want, np.sqrt(2.0))
    print("%s: worst RMS of the error per block: %.3g of the input's RMS" % (name, dev))
    assert record_bound("tuner against the float64 model, %s" % name, dev, TC.BAR)
    # the phase is the absolute index's: the same stream from position 0 differs
    other, _ = _run(md, pkg, (rate, sel), x, position=0)
    n = min(other.size, got.size)
    assert not np.allclose(other[other.size - n:], got[got.size - n:], atol=1e-3)


def test_ratio_1_wide_offset_0_returns_the_input_bytes_trailing_by_16(md, pkg):
    md.set_tuner(2048000, 0, 0.0)
    x = TC.signal(TC.N_STREAM, 4)
    got, counts = _run(md, pkg, (2048000, 0), x)
    assert counts == [TC.N_STREAM - 16] and np.array_equal(got.view(np.uint32), x[:TC.N_STREAM - 16].view(np.uint32))
    # from a reset at P the output starts at M(P) = P - 16: sixteen outputs on the zero history, then the input
    got, counts = _run(md, pkg, (2048000, 0), x, [1, 16, 17, TC.N_STREAM - 34], position=2 ** 40)
    assert counts == [1, 16, 17, TC.N_STREAM - 34] and not got[:16].any()
    assert np.array_equal(got[16:].view(np.uint32), x[:TC.N_STREAM - 16].view(np.uint32))
    # the host-pointer form, on a stream of its own position
    md.tuner_reset(0)
    y = md.tuner(x[:100])
    assert np.array_equal(y, x[:84]) and md.tuner_position() == 100
    assert np.array_equal(md.tuner(x[100:107]), x[84:91]) and md.tuner_position() == 107


def test_integer_inputs_are_their_values_and_s16_output_is_the_format_converters(md, pkg):
    import torch
    rate, sel, off = 2400000, 1, 222222.2
    md.set_tuner(rate, sel, off)
    q = TC.signal(TC.N_STREAM, 5, s16=True)
    q[4000:8000] = np.where(q[4000:8000] >= 0, 32767, -32768)            # a stretch at full scale: the filter overshoots it
    for name, x in (("s16", q), ("u8", TC.signal_u8(TC.N_STREAM, 6)), ("s8", TC.signal_u8(TC.N_STREAM, 7, signed=True))):
        as_float = TC.as_float_samples(x)
        y, counts = _run(md, pkg, (rate, sel), x)
        # the integer input gives the bytes of its values as complexf
        yf, counts_f = _run(md, pkg, (rate, sel), as_float.astype(np.complex64))
        assert counts == counts_f and np.array_equal(y.view(np.uint32), yf.view(np.uint32)), name
        want = TM.run(pkg, rate, sel, off, as_float)[0]
        x_rms = float(np.sqrt(np.mean(np.abs(as_float) ** 2)))
        dev = _block_error(y, want, x_rms)
        print("%s input: worst RMS of the error per block: %.3g of the input's RMS" % (name, dev))
        assert record_bound("tuner against the float64 model, %s input" % name, dev, TC.BAR)
        md.tuner_reset(0)
        assert np.array_equal(md.tuner(x).view(np.uint32), y.view(np.uint32)), name
    # s16 output: dabgpu_format_process's conversion of the complexf output, byte for byte
    y, counts = _run(md, pkg, (rate, sel), q)
    y16, counts16 = _run(md, pkg, (rate, sel), q, out="s16")
    assert counts == counts16
    d_conv = torch.zeros(2 * y.size, dtype=torch.int16, device="cuda")
    md.format_convert_dev(torch.from_numpy(y).cuda(), "s16", d_conv)
    torch.cuda.synchronize()
    conv = d_conv.cpu().numpy()
    assert np.array_equal(y16, conv) and np.array_equal(conv, TM.to_s16(y.astype(np.complex128)))
    assert int((np.abs(conv.astype(np.int32)) >= 32767).sum()) > 100
    md.tuner_reset(0)
    assert np.array_equal(md.tuner(q, out="s16"), y16)


# --------------------------------------------------------------------------- 4. refusals
def test_refusals_queue_nothing_and_leave_the_stream_alone(pkg):
    import torch
    md = pkg.Modulator(mode=2, max_frames=2)
    try:
        lib, h = md._lib, md._h
        rate, sel = 2400000, 0
        x = TC.signal(4096, 8)
        d_x = torch.from_numpy(x).cuda()
        d_y = torch.zeros(6000, dtype=torch.complex64, device="cuda")
        got = C.c_size_t(77)

        def call(d_in, fi, n, d_out, fo, cap, n_out=got):
            return lib.dabgpu_tuner_dev(h, d_in, fi, n, d_out, fo, cap, C.byref(n_out) if n_out is not None else None, None)

        def refused(rc, words, code=E_INVALID):
            assert rc == code and words in lib.dabgpu_last_error(h).decode(), (rc, lib.dabgpu_last_error(h))

        refused(call(d_x.data_ptr(), 0, 100, d_y.data_ptr(), 0, 6000), "no setting (no dabgpu_set_tuner call yet)")
        for (r, s, o), words in TC.REFUSED:
            with pytest.raises(pkg.DabGpuError) as e:
                md.set_tuner(r, s, o)
            assert words in str(e.value)
        refused(lib.dabgpu_set_tuner(h, None), "null argument")
        refused(call(d_x.data_ptr(), 0, 100, d_y.data_ptr(), 0, 6000), "no setting")
        md.set_tuner(rate, sel, 150000.0)
        want, _ = _run(md, pkg, (rate, sel), x)
        md.tuner_reset(0)
        first = pkg.tuner_count(rate, sel, 1000)
        assert md.tuner_dev(d_x[:1000], d_y) == first
        torch.cuda.synchronize()
        before = d_y.clone()
        a, b = d_x[1000:].data_ptr(), d_y[2000:].data_ptr()
        # a refused setting leaves the installed one, the position and the history alone
        for (r, s, o), words in TC.REFUSED[:4]:
            with pytest.raises(pkg.DabGpuError):
                md.set_tuner(r, s, o)
        refused(call(a, 4, 100, b, 0, 3000), "input format is complexf (0), DABGPU_FMT_S16, DABGPU_FMT_U8 or DABGPU_FMT_S8")
        refused(call(a, -1, 100, b, 0, 3000), "input format is")
        refused(call(a, 0, 100, b, U8, 3000), "output format is complexf (0) or DABGPU_FMT_S16")
        refused(call(a, 0, 100, b, S8, 3000), "output format is complexf (0) or DABGPU_FMT_S16")
        refused(call(None, 0, 100, b, 0, 3000), "null argument")
        refused(call(a, 0, 100, None, 0, 3000), "null argument")
        assert lib.dabgpu_tuner_dev(h, a, 0, 100, b, 0, 3000, None, None) == E_INVALID
        refused(call(a + 4, 0, 100, b, 0, 3000), "aligned to a sample")
        refused(call(a, 0, 100, b + 2, S16, 3000), "aligned to a sample")
        refused(call(a + 1, U8, 100, b, 0, 3000), "aligned to a sample")
        refused(call(a, 0, 0, b, 0, 3000), "n_in must not be 0")
        refused(call(a, 0, 2 ** 40 + 1, b, 0, 2 ** 41), "n_in must not exceed 2^40")
        refused(call(a, 0, 200, a + 8 * 150, 0, 3000), "must not overlap")
        refused(call(a, 0, 200, a - 8 * 50, 0, 3000), "must not overlap")
        refused(lib.dabgpu_tuner_reset(h, 2 ** 50 + 1), "position must not exceed 2^50")
        refused(lib.dabgpu_debug_tuner_run_samples(h, -1), "must not be negative")
        # a short out_cap: the count comes back, nothing else happens
        count = pkg.tuner_count(rate, sel, 4096) - first
        got.value = 77
        refused(call(a, 0, 3096, b, 0, count - 1), "output buffer too small", E_CAPACITY)
        assert got.value == count
        with pytest.raises(pkg.DabGpuError, match="output buffer too small"):
            md.tuner_dev(d_x[1000:], d_y[2000:2000 + count - 1])
        assert md.tuner_position() == 1000
        torch.cuda.synchronize()
        assert torch.equal(d_y, before)
        # the stream goes on as if nothing had been asked
        assert md.tuner_dev(d_x[1000:], d_y[2000:]) == count
        torch.cuda.synchronize()
        tail = d_y[2000:2000 + count].cpu().numpy()
        assert np.array_equal(tail.view(np.uint32), want[want.size - count:].view(np.uint32))
        # the host-pointer form refuses the same way
        md.tuner_reset(0)
        with pytest.raises(pkg.DabGpuError, match="n_in must not be 0"):
            md.tuner(np.zeros(0, np.complex64))
        assert md.tuner_position() == 0
    finally:
        md.close()


# --------------------------------------------------------------------------- 5. the loop on device tensors
def _device_capture(pkg, md, rate):
    """set_resampler(2048000, rate), chain_dev of the capture's bits as a lead-in frame, the two frames and a tail frame; the
    stream from where the model's capture starts (its lead-in's first sample), with the zeros the cases put behind it -> a
    complex64 tensor at `rate`"""
    import torch
    from tests import channel_cases as CC
    from tests.sync_cases import case_bits
    from tests.sync_model import geometry
    mode = 2
    g = geometry(mode)
    lead, delay = CC.CAPTURES[TC.CAPTURE][3], CC.CAPTURES[TC.CAPTURE][4]
    tail = max(2 * g["B"] + g["N"], g["null"] - lead) + delay
    bits = case_bits(mode, 2)
    L, M = TC.LISTED[rate]
    md.set_resampler(2048000, rate)
    stages = pkg.STAGE_RESAMPLE
    per = md.out_samples_per_frame(stages)
    assert per == g["tf"] * M // L
    d_bits = torch.from_numpy(np.ascontiguousarray(bits[[2, 0, 1, 2]])).cuda()
    d_out = torch.zeros((4, per), dtype=torch.complex64, device="cuda")
    md.chain_dev(d_bits, 4, stages, d_out)
    # native sample k of the four frames lies at (k + 512) M / L behind the Resampler's delay; the model's capture is native
    # samples tf - lead ... 3 tf + tail, so its stream starts at output (tf - lead) M / L (rounded up) with the delay inside
    first = -(-(g["tf"] - lead) * M // L)
    n = (lead + 2 * g["tf"] + tail) * M // L
    stream = d_out.reshape(-1)[first:first + n]
    return torch.cat([stream, torch.zeros(4096 * M // L + M, dtype=torch.complex64, device="cuda")]).contiguous()


def _torch_tones(d_y, rate, freqs, span):
    import torch
    power = float((d_y[span[0]:span[1]].abs().double() ** 2).mean())
    k = torch.arange(d_y.numel(), dtype=torch.float64, device="cuda")
    t = torch.zeros(d_y.numel(), dtype=torch.complex128, device="cuda")
    for f in freqs:
        t += torch.polar(torch.full_like(k, TC.tone_amplitude(power)), 2.0 * np.pi * torch.remainder(f / rate * k, 1.0))
    return (d_y.to(torch.complex128) + t).to(torch.complex64)


def _torch_second_block(d_y, rate):
    import torch
    late = TC.SECOND_BLOCK_LATE
    copy = torch.cat([d_y[1000:1000 + late], d_y[:d_y.numel() - late]]).to(torch.complex128)
    k = torch.arange(d_y.numel(), dtype=torch.float64, device="cuda")
    rot = torch.polar(torch.ones_like(k), 2.0 * np.pi * torch.remainder(TC.SECOND_BLOCK_HZ / rate * k, 1.0))
    return (d_y.to(torch.complex128) + copy * rot).to(torch.complex64)


LOOP_CASES = {
    "clean_8192000": (8192000, None, [(0, 0.0)]),
    "clean_2400000": (2400000, None, [(0, 0.0)]),
    "near_tones_8192000": (8192000, "near", [(1, 0.0)]),
    "far_tones_8192000": (8192000, "far", [(0, 0.0)]),
    "two_blocks_8192000": (8192000, "two", [(1, 0.0), (1, TC.SECOND_BLOCK_HZ)]),
}


@pytest.mark.parametrize("name", list(LOOP_CASES))
def test_the_loop_on_device_tensors(pkg, name):
    """set_resampler -> chain_dev -> interferers (torch) -> tuner_dev -> sync_dev -> sync_extract_dev -> demod_dev, against the
    model on the very samples the device tuned: no bit error, starts, shifts and validity the model's, the MER not more than
    1 dB below the model's (fp32's floor lies some 60 dB under these figures; a wrong tap or phase costs tens of dB)."""
    import torch
    from tests.sync_model import extract_slots, geometry
    rate, interferers, tunings = LOOP_CASES[name]
    _, mode, bits, early = TC.capture()
    tf = geometry(mode)["tf"]
    m = pkg.Modulator(mode=mode, max_frames=4)
    try:
        d_cap = _device_capture(pkg, m, rate)
        if interferers == "near":
            d_cap = _torch_tones(d_cap, rate, TC.NEAR_TONES, TC.data_span(rate, mode))
        elif interferers == "far":
            d_cap = _torch_tones(d_cap, rate, TC.FAR_TONES, TC.data_span(rate, mode))
        elif interferers == "two":
            d_cap = _torch_second_block(d_cap, rate)
        d_cap = d_cap.contiguous()
        cap = d_cap.cpu().numpy()
        d_ref = torch.from_numpy(np.ascontiguousarray(bits)).cuda()
        d_bits = torch.zeros((2, m.geometry["tf_input_bytes"]), dtype=torch.uint8, device="cuda")
        for sel, off in tunings:
            want = TM.receive(TM.run(pkg, rate, sel, off, cap)[0], mode, early, bits)
            m.set_tuner(rate, sel, off)
            d_iq = torch.zeros(pkg.tuner_out_max(rate, sel, d_cap.numel()), dtype=torch.complex64, device="cuda")
            n = m.tuner_dev(d_cap, d_iq)
            assert n == pkg.tuner_count(rate, sel, d_cap.numel())
            d_iq = d_iq[:n].contiguous()
            m.sync_dev(d_iq, 31)
            d_frames = torch.zeros((extract_slots(n, mode, 4), tf), dtype=torch.complex64, device="cuda")
            m.sync_extract_dev(d_iq, d_frames)
            found = m.sync_result()
            m.demod_dev(d_frames[:2].contiguous(), 2, early, d_bits, d_ref)
            torch.cuda.synchronize()
            st = [m.monitor_stats(f) for f in range(2)]
            got = dict(starts=[f["start"] for f in found][:2], shifts=[f["shift"] for f in found][:2],
                       valid=[f["valid"] for f in found][:2], bit_errors=[s["bit_errors"] for s in st],
                       mer_db=10.0 * np.log10(sum(s["sum_signal"] for s in st) / sum(s["sum_quadrature"] for s in st)))
            print("%s offset %.0f: starts %s shifts %s bit errors %s MER %.2f dB (model: %s %s %s %.2f dB)"
                  % (name, off, got["starts"], got["shifts"], got["bit_errors"], got["mer_db"], want["starts"], want["shifts"],
                     want["bit_errors"], want["mer_db"]))
            assert want["bit_errors"] == [0, 0] and want["valid"][:2] == [1, 1]
            for key in ("starts", "shifts", "valid"):
                assert got[key] == want[key][:2], (key, got[key], want[key])
            assert got["bit_errors"] == [0, 0]
            assert got["mer_db"] >= want["mer_db"] - 1.0
            if rate == 8192000:                     # (the stream starts on a whole native sample: the cases' own starts)
                assert got["starts"] == (TC.SECOND_BLOCK_STARTS if off else TC.EXPECTED_STARTS)
    finally:
        m.close()


# --------------------------------------------------------------------------- 6. behind the lanes
B, STAGES, MODE = 256, 3, 2                        # (frames per chain call, GainControl and FIRFilter: tests/receive_lanes_ops.py)


def _directed(pkg, d_bits, lanes):
    """As tests/test_clock_gpu.py: a rehearsal, every step waited for; then three chain calls (the third, on lane 2, writes the
    capture), tuner_dev queued on it, a chain call on lane 0 and one on lane 1 that overwrites the capture.  With one lane every
    step is waited for.  -> (the tuner's output bytes and count, lanes the calls went over, the capture's bytes)"""
    import torch
    md = pkg.Modulator(mode=MODE, max_frames=B)
    try:
        tf = md.geometry["tf_samples"]
        md.set_lanes(lanes)
        md.set_gain(2, 1.0, 0.5, 4.0)
        md.set_tuner(2400000, 1, 100000.0)              # (the capture read as if it were at 2.4 MS/s: the bytes are what counts)
        cap, spare0, spare1 = (torch.zeros(B * tf, dtype=torch.complex64, device="cuda") for _ in range(3))
        rx = torch.zeros(pkg.tuner_out_max(2400000, 1, B * tf), dtype=torch.complex64, device="cuda")
        torch.cuda.synchronize()
        md.chain_dev_queued(d_bits[1], B, STAGES, spare0)
        md.synchronize()
        md.tuner_dev(spare0, rx, queued=True)
        md.synchronize()
        md.tuner_reset(0)
        rx.zero_()
        torch.cuda.synchronize()
        md.set_lanes(lanes)
        step = md.synchronize if lanes == 1 else (lambda: None)
        for src, dst in ((1, spare0), (2, spare1), (0, cap)):
            md.chain_dev_queued(d_bits[src], B, STAGES, dst)
            step()
        created = md.lanes_info()[0]
        count = md.tuner_dev(cap, rx, queued=True)
        step()
        md.chain_dev_queued(d_bits[3], B, STAGES, spare0)
        step()
        md.chain_dev_queued(d_bits[4], B, STAGES, cap)
        md.synchronize()
        return torch.view_as_real(rx).clone(), count, created, torch.view_as_real(cap).clone()
    finally:
        md.close()


def test_a_queued_call_between_the_chain_call_it_reads_and_the_one_that_overwrites(pkg):
    import torch
    md = pkg.Modulator(mode=MODE, max_frames=1)
    per = md.geometry["tf_input_bytes"]
    md.close()
    d_bits = torch.from_numpy(np.random.RandomState(9).randint(0, 256, (5, B, per)).astype(np.uint8)).cuda()
    want, n1, one, cap1 = _directed(pkg, d_bits, 1)
    got, n3, three, cap3 = _directed(pkg, d_bits, 3)
    assert (one, three) == (1, 3) and n1 == n3 > 0
    assert bool(want.any()) and torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert torch.equal(cap3.view(torch.int32), cap1.view(torch.int32))
