"""The clock's resampler on the device (clock.hip; include/dabgpu.h, "the clock"): every case of
tests/clock_cases.py against the float64 model (tests/clock_model.py) below the project's bar for float paths; one stream in any
chunking and run geometry, the same bytes and the same counts; identity; formats; refusals that queue nothing; the estimator against its
model; the whole loop on device tensors at the operating points tests/test_clock_cpu.py establishes; queued calls behind the
lanes."""
import ctypes as C

import numpy as np
import pytest

from tests import clock_cases as KC
from tests import clock_model as KM
from tests.conftest import load_pkg, record_bound

pytestmark = pytest.mark.gpu
E_INVALID, E_CAPACITY = -1, -4
S16 = 1


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
    return x.size // 2 if x.dtype == np.int16 else x.size


def _run(md, pkg, x, lengths=None, out="complexf", position=0, alternate=False):
    """reset at `position`, then the stream x (complex64, or int16 pairs) in calls of these lengths -> (the outputs joined, as
    numpy; the counts of the calls).  alternate: x holds int16 values; every second call gets them as complex64."""
    import torch
    n = _n(x)
    d_x = torch.from_numpy(np.array(x)).cuda()
    d_c = torch.from_numpy(KM.as_samples(x).astype(np.complex64)).cuda() if alternate else None
    cap = pkg.clock_out_max(n) + 8
    d_y = torch.zeros(cap, dtype=torch.complex64, device="cuda") if out == "complexf" else torch.zeros(2 * cap, dtype=torch.int16, device="cuda")
    md.clock_reset(position)
    at, made, counts = 0, 0, []
    for k, m in enumerate(lengths or [n]):
        if alternate and k % 2:
            d_in = d_c[at:at + m]
        else:
            d_in = d_x[2 * at:2 * (at + m)] if x.dtype == np.int16 else d_x[at:at + m]
        room = pkg.clock_out_max(m)
        d_out = d_y[made:made + room] if out == "complexf" else d_y[2 * made:2 * (made + room)]
        got = md.clock_dev(d_in, d_out)
        counts.append(got)
        at += m
        made += got
    assert at == n and md.clock_position() == position + n
    torch.cuda.synchronize()
    y = d_y.cpu().numpy()
    assert not y[made if out == "complexf" else 2 * made:].any()          # nothing behind the counts was written
    return y[:made if out == "complexf" else 2 * made], counts


def _block_deviation(dist, want):
    """worst relative RMS per block of KC.BLOCK outputs; dist: |difference| per sample"""
    worst = 0.0
    for b in range(0, want.size, KC.BLOCK):
        ref = float(np.sqrt(np.mean(np.abs(want[b:b + KC.BLOCK]) ** 2)))
        assert ref > 0.0
        worst = max(worst, float(np.sqrt(np.mean(dist[b:b + KC.BLOCK] ** 2))) / ref)
    return worst


def _distance_to_preimage(q, v):
    """per component: how far the model's value v lies from the values that dabgpu_format_process turns into the integer q
    (toward zero, saturating) -- the smallest error the value in front of the conversion can have had"""
    q = q.astype(np.float64)
    lo = np.where(q > 0, q, q - 1.0)                # q > 0: [q, q + 1); q < 0: (q - 1, q]; 0: (-1, 1)
    hi = np.where(q < 0, q, q + 1.0)
    lo = np.where(q <= -32768, -np.inf, lo)
    hi = np.where(q >= 32767, np.inf, hi)
    return np.maximum(np.maximum(lo - v, v - hi), 0.0)


# --------------------------------------------------------------------------- 1. against the model
@pytest.mark.parametrize("name", list(KC.KERNEL_CASES))
def test_every_case_follows_the_float64_model(md, pkg, name):
    """Worst relative RMS of the difference per block of 2048 outputs, held to 1e-6.  An s16 output cannot lie that near a
    float: there the figure is taken on the distance of the model's value from the interval of values that the format
    conversion turns into the integer the device wrote (zero when the model's value itself converts to it)."""
    c = KC.kernel_case(name)
    n = sum(c["lengths"])
    x = KC.signal(n, 1, c["s16"])
    md.set_clock(c["ppm"])
    got, counts = _run(md, pkg, x, c["lengths"], c["out"], c["position"])
    want, want_counts = KM.run(pkg, c["ppm"], x, c["lengths"], c["position"])
    assert counts == want_counts
    total = pkg.clock_count(c["ppm"], c["position"] + n) - pkg.clock_count(c["ppm"], c["position"])
    assert sum(counts) == total
    if total == 0:
        assert got.size == 0
        return
    if c["out"] == "s16":
        q = got.reshape(-1, 2)
        dist = np.hypot(_distance_to_preimage(q[:, 0], want.real), _distance_to_preimage(q[:, 1], want.imag))
        inside = np.abs(q.astype(np.int32)) < 32767                     # (the components the conversion did not saturate)
        assert inside.mean() > 0.5 and not inside.all()
        assert np.abs(q.astype(np.float64) - np.stack([want.real, want.imag], 1))[inside].max() < 1.0 + 1e-2
    else:
        assert got.shape == want.shape and np.isfinite(got.view(np.float32)).all()
        dist = np.abs(got.astype(np.complex128) - want)
    dev = _block_deviation(dist, want)
    print("%s: %d outputs, worst relative RMS per block of %d: %.3g" % (name, total, KC.BLOCK, dev))
    assert record_bound("clock against the float64 model, %s" % name, dev, KC.BAR)


# --------------------------------------------------------------------------- 2. one stream, any chunking, the same bytes
@pytest.mark.parametrize("ppm", KC.STREAM_PPM)
def test_any_chunking_and_run_geometry_gives_the_bytes_and_counts_of_one_call(md2, pkg, ppm):
    md = md2
    step = pkg.clock_step(ppm)
    md.set_clock(ppm)
    x = KC.signal(KC.N_STREAM, 2)
    q = KC.signal(KC.N_STREAM, 3, s16=True)
    position = 12345
    try:
        md.set_clock_run_samples(0)
        whole, counts = _run(md, pkg, x, position=position)
        whole_q, _ = _run(md, pkg, q, position=position)
        total = pkg.clock_count(ppm, position + KC.N_STREAM) - pkg.clock_count(ppm, position)
        assert counts == [total] and len(np.unique(whole.view(np.uint32))) > KC.N_STREAM
        again, _ = _run(md, pkg, x, position=position)
        assert np.array_equal(again.view(np.uint32), whole.view(np.uint32))
        # (the cuts are placed for a stream from 0; from 12345 they fall elsewhere, so the stream from 0 is walked as well)
        whole0, counts0 = _run(md, pkg, x)
        for run in KC.RUN_SAMPLES:
            md.set_clock_run_samples(run)
            for name, lengths in KC.splits(step).items():
                got, counts = _run(md, pkg, x, lengths, position=position)
                assert np.array_equal(got.view(np.uint32), whole.view(np.uint32)), (run, name)
                at, want = position, []
                for m in lengths:
                    want.append(pkg.clock_count(ppm, at + m) - pkg.clock_count(ppm, at))
                    at += m
                assert counts == want, (run, name)
            got, counts = _run(md, pkg, x, KC.splits(step)["on_a_slip_and_beside"])
            assert np.array_equal(got.view(np.uint32), whole0.view(np.uint32)) and sum(counts) == counts0[0], run
            got, _ = _run(md, pkg, q, KC.splits(step)["sevens"], position=position, alternate=True)
            assert np.array_equal(got.view(np.uint32), whole_q.view(np.uint32)), (run, "alternating formats")
        # the history is handed over by one kernel for every input format: each of them cut into sevens (every call shorter
        # than the history) and at [1, n - 1], at one run geometry
        md.set_clock_run_samples(0)
        for fmt, stream, want in (("complexf", x, whole), ("s16", q, whole_q)):
            for name in ("sevens", "one_rest"):
                got, _ = _run(md, pkg, stream, KC.splits(step)[name], position=position)
                assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (fmt, name)
    finally:
        md.set_clock_run_samples(0)


# --------------------------------------------------------------------------- 3. identity and formats
def test_ppm_0_returns_the_input_bytes(md, pkg):
    md.set_clock(0.0)
    x = KC.signal(KC.N_STREAM, 4)
    got, counts = _run(md, pkg, x)
    assert counts == [KC.N_STREAM - 16] and np.array_equal(got.view(np.uint32), x[:KC.N_STREAM - 16].view(np.uint32))
    # from a reset at P the output starts at M(P) = P - 16: sixteen outputs on the zero history, then the input
    got, counts = _run(md, pkg, x, [1, 16, 17, KC.N_STREAM - 34], position=2 ** 40)
    assert counts == [1, 16, 17, KC.N_STREAM - 34] and not got[:16].any()
    assert np.array_equal(got[16:].view(np.uint32), x[:KC.N_STREAM - 16].view(np.uint32))
    # the host-pointer form, on a stream of its own position
    md.clock_reset(0)
    y = md.clock(x[:100])
    assert np.array_equal(y, x[:84]) and md.clock_position() == 100
    assert np.array_equal(md.clock(x[100:107]), x[84:91]) and md.clock_position() == 107


def test_s16_output_is_the_format_converters_and_s16_input_is_its_values(md, pkg):
    import torch
    q = KC.signal(KC.N_STREAM, 5, s16=True)
    q[:8] = (32767, -32768, 30000, -30000, 1, -1, 0, 12345)
    q[4000:8000] = np.where(q[4000:8000] >= 0, 32767, -32768)            # a stretch at full scale: the interpolator overshoots it
    for ppm in (1000.0, -37.5):
        md.set_clock(ppm)
        y, counts = _run(md, pkg, q)
        y16, counts16 = _run(md, pkg, q, out="s16")
        assert counts == counts16
        d_conv = torch.zeros(2 * y.size, dtype=torch.int16, device="cuda")
        md.format_convert_dev(torch.from_numpy(y).cuda(), "s16", d_conv)
        torch.cuda.synchronize()
        conv = d_conv.cpu().numpy()
        assert np.array_equal(y16, conv), ppm
        assert np.array_equal(conv, KM.to_s16(y.astype(np.complex128)))
        assert int((np.abs(conv.astype(np.int32)) >= 32767).sum()) > 100, ppm
        as_float = KM.as_samples(q).astype(np.complex64)
        assert np.array_equal(_run(md, pkg, as_float)[0].view(np.uint32), y.view(np.uint32)), ppm
        md.clock_reset(0)
        assert np.array_equal(md.clock(q, out="s16"), y16)


# --------------------------------------------------------------------------- 4. refusals
def test_refusals_queue_nothing_and_leave_the_stream_alone(pkg):
    import torch
    md = pkg.Modulator(mode=2, max_frames=2)
    try:
        lib, h = md._lib, md._h
        x = KC.signal(4096, 6)
        d_x = torch.from_numpy(x).cuda()
        d_y = torch.zeros(6000, dtype=torch.complex64, device="cuda")
        got = C.c_size_t(77)

        def call(d_in, fi, n, d_out, fo, cap, n_out=got):
            return lib.dabgpu_clock_dev(h, d_in, fi, n, d_out, fo, cap, C.byref(n_out) if n_out is not None else None, None)

        def refused(rc, words, code=E_INVALID):
            assert rc == code and words in lib.dabgpu_last_error(h).decode(), (rc, lib.dabgpu_last_error(h))

        refused(call(d_x.data_ptr(), 0, 100, d_y.data_ptr(), 0, 6000), "no setting (no dabgpu_set_clock call yet)")
        for bad, words in ((float("nan"), "ppm must be finite"), (1000.5, "|ppm| must not exceed 1000")):
            refused(lib.dabgpu_set_clock(h, bad), words)
        refused(call(d_x.data_ptr(), 0, 100, d_y.data_ptr(), 0, 6000), "no setting")
        md.set_clock(1000.0)
        want, _ = _run(md, pkg, x)
        md.clock_reset(0)
        assert md.clock_dev(d_x[:1000], d_y) == pkg.clock_count(1000.0, 1000)
        torch.cuda.synchronize()
        before = d_y.clone()
        a, b = d_x[1000:].data_ptr(), d_y[2000:].data_ptr()
        refused(call(a, 2, 100, b, 0, 3000), "formats are complexf (0) or DABGPU_FMT_S16")
        refused(call(a, 0, 100, b, 3, 3000), "formats are complexf (0) or DABGPU_FMT_S16")
        refused(call(None, 0, 100, b, 0, 3000), "null argument")
        refused(call(a, 0, 100, None, 0, 3000), "null argument")
        assert lib.dabgpu_clock_dev(h, a, 0, 100, b, 0, 3000, None, None) == E_INVALID
        refused(call(a + 4, 0, 100, b, 0, 3000), "aligned to a sample")
        refused(call(a, 0, 100, b + 2, S16, 3000), "aligned to a sample")
        refused(call(a, 0, 0, b, 0, 3000), "n_in must not be 0")
        refused(call(a, 0, 2 ** 40 + 1, b, 0, 2 ** 41), "n_in must not exceed 2^40")
        refused(call(a, 0, 200, a + 8 * 150, 0, 3000), "must not overlap")
        refused(call(a, 0, 200, a - 8 * 50, 0, 3000), "must not overlap")
        refused(lib.dabgpu_clock_reset(h, 2 ** 62 + 1), "position must not exceed 2^62")
        refused(lib.dabgpu_debug_clock_run_samples(h, -1), "must not be negative")
        # a short out_cap: the count comes back, nothing else happens
        count = pkg.clock_count(1000.0, 4096) - pkg.clock_count(1000.0, 1000)
        got.value = 77
        refused(call(a, 0, 3096, b, 0, count - 1), "output buffer too small", E_CAPACITY)
        assert got.value == count
        with pytest.raises(pkg.DabGpuError, match="output buffer too small"):
            md.clock_dev(d_x[1000:], d_y[2000:2000 + count - 1])
        assert md.clock_position() == 1000
        torch.cuda.synchronize()
        assert torch.equal(d_y, before)
        # the stream goes on as if nothing had been asked
        assert md.clock_dev(d_x[1000:], d_y[2000:]) == count
        torch.cuda.synchronize()
        tail = d_y[2000:2000 + count].cpu().numpy()
        assert np.array_equal(tail.view(np.uint32), want[want.size - count:].view(np.uint32))
        # the host-pointer form refuses the same way
        md.clock_reset(0)
        with pytest.raises(pkg.DabGpuError, match="n_in must not be 0"):
            md.clock(np.zeros(0, np.complex64))
        assert md.clock_position() == 0
    finally:
        md.close()


# --------------------------------------------------------------------------- 5. the estimator against the model
_FRAMES = {}


def _frames_of(pkg, mode):
    """whole frames with a clock offset on them, per mode (1: 20 ppm, 2 and 3: 100 ppm), as the model extracts them; once"""
    from tests import channel_model as CM
    from tests.sync_model import extract_model, extract_slots, geometry, sync_model
    if mode not in _FRAMES:
        if mode == 3:
            import oracle as O
            from tests.sync_cases import case_bits
            g = geometry(3)
            y = np.asarray(O.Chain(mode=3, stages=0).process(case_bits(3, 2))).reshape(-1)[:2 * g["tf"]].astype(np.complex64)
            x = np.concatenate([y, y[:g["null"] + 4 * g["sym"]]])
            cap = KM.run(pkg, 100.0, x)[0].astype(np.complex64)
            # the frames where they lie: the second one starts tf / (1 + delta) in, rounded
            s1 = int(round(g["tf"] / (1.0 + 100e-6)))
            frames, early = np.stack([cap[:g["tf"]], cap[s1:s1 + g["tf"]]]), g["CP"] // 2
        else:
            x, m, bits, early, ppm, (paths, sigma, seed) = KC.loop_case({1: "m1_p20", 2: "m2_p100"}[mode], pkg.channel_sigma)
            cap = KM.run(pkg, ppm, CM.Channel(paths, sigma, seed)(x).astype(np.complex64))[0].astype(np.complex64)
            r = sync_model(cap, mode, 31, 2)
            frames = extract_model(cap, mode, r["frames"], extract_slots(cap.size, mode, 2)).astype(np.complex64)
        frames.setflags(write=False)
        _FRAMES[mode] = (frames, early)
    return _FRAMES[mode]


@pytest.mark.parametrize("mode", [2, 3, 1])
def test_estimator_follows_the_model_and_repeats_byte_for_byte(pkg, mode):
    """Raw sums within 1e-6 of |A| (A_hi and A_lo against their own magnitude, S against itself), ppm within the bound that
    follows, 2e-6 / (2 pi (sym / N) (K/2 + 1)) rad turned into ppm; the records' bytes for every run geometry and on repetition,
    complexf and the host form alike; s16 frames against the model on their values; a frame of zeros: valid = 0, all figures 0."""
    import torch
    from tests.receiver import MODES
    N, K, nsym, null, sym = MODES[mode]
    frames, early = _frames_of(pkg, mode)
    per, total = KM.sco_model(frames, mode, early)
    md = pkg.Modulator(mode=mode, max_frames=2)
    try:
        d = torch.from_numpy(np.array(frames)).cuda()
        md.sco_dev(d, 2, early)
        got = [md.sco_result(f) for f in (0, 1, -1)]
        bound_ppm = 1e6 * 2e-6 / (2.0 * np.pi * (sym / N) * (K // 2 + 1))
        worst_sum = worst_ppm = 0.0
        for g, w in zip(got, per + [total]):
            assert g["valid"] == w["valid"] == 1
            worst_sum = max(worst_sum, abs(g["a_hi"] - w["a_hi"]) / abs(w["a_hi"]), abs(g["a_lo"] - w["a_lo"]) / abs(w["a_lo"]),
                            abs(g["s"] - w["s"]) / w["s"])
            worst_ppm = max(worst_ppm, abs(g["ppm"] - w["ppm"]))
            assert abs(g["residual_cfo"] - w["residual_cfo"]) <= 2e-6 / (2.0 * np.pi * sym / N)
            assert abs(g["quality"] - w["quality"]) <= 2e-6
        print("mode %d: estimates %s ppm (model %s); sums off by %.3g of |A|, ppm by %.3g (bound %.3g)"
              % (mode, [round(g["ppm"], 4) for g in got], [round(w["ppm"], 4) for w in per + [total]], worst_sum, worst_ppm, bound_ppm))
        assert record_bound("sco raw sums against the float64 model, mode %d" % mode, worst_sum, 1e-6)
        assert record_bound("sco ppm against the float64 model, mode %d" % mode, worst_ppm, bound_ppm)
        # frame -1 is the frames' sums added in frame order
        assert got[2]["a_hi"] == got[0]["a_hi"] + got[1]["a_hi"] and got[2]["s"] == got[0]["s"] + got[1]["s"]
        raw = [g["raw"] for g in got]
        try:
            for run in (0, 1, 5, 1000):
                md.set_demod_run_symbols(run)
                for _ in range(2):
                    md.sco_dev(d, 2, early)
                    assert [md.sco_result(f)["raw"] for f in (0, 1, -1)] == raw, run
        finally:
            md.set_demod_run_symbols(0)
        md.sco(frames, early)
        assert [md.sco_result(f)["raw"] for f in (0, 1, -1)] == raw
        md.sco_dev(d[1:].contiguous(), 1, early)
        assert md.sco_result(0)["raw"] == raw[1] and md.sco_result(-1)["raw"] == raw[1]
        with pytest.raises(pkg.DabGpuError, match="no clock estimate for this frame"):
            md.sco_result(1)
        # s16: the values, scaled into the format's range first
        scale = 20000.0 / float(np.abs(frames.view(np.float32)).max())
        q = np.trunc(frames.view(np.float32).reshape(2, -1) * scale).astype(np.int16)
        md.sco_dev(torch.from_numpy(q.reshape(-1)).cuda(), 2, early)
        wq = KM.sco_model(q, mode, early)[1]
        gq = md.sco_result(-1)
        assert abs(gq["a_hi"] - wq["a_hi"]) <= 1e-6 * abs(wq["a_hi"]) and abs(gq["ppm"] - wq["ppm"]) <= bound_ppm
        # a frame of zeros between two calls: not valid, every figure 0, and left out of the sums of frame -1
        z = torch.zeros_like(d)
        z[1] = d[1]
        md.sco_dev(z, 2, early)
        zero = md.sco_result(0)
        assert zero["valid"] == 0 and not any(zero["raw"])
        assert md.sco_result(1)["raw"] == raw[1] and md.sco_result(-1)["raw"] == raw[1]
        # refusals: the receiver's, nothing queued, the records stay
        lib, h = md._lib, md._h
        for args, words in (((d.data_ptr(), 2, 2, early, None), "input format is complexf (0) or DABGPU_FMT_S16"),
                            ((d.data_ptr(), 0, 2, sym - N + 1, None), "early must lie inside the cyclic prefix"),
                            ((d.data_ptr(), 0, 2, -1, None), "early must lie inside the cyclic prefix"),
                            ((d.data_ptr(), 0, 0, early, None), "n_frames must not be 0"),
                            ((d.data_ptr(), 0, 3, early, None), "n_frames exceeds max_frames"),
                            ((None, 0, 2, early, None), "null argument"),
                            ((d.data_ptr() + 4, 0, 1, early, None), "aligned to a sample")):
            assert lib.dabgpu_sco_dev(h, *args) != 0 and words in lib.dabgpu_last_error(h).decode(), words
        assert md.sco_result(1)["raw"] == raw[1]
    finally:
        md.close()


# --------------------------------------------------------------------------- 6. the loop on device tensors
@pytest.mark.parametrize("name", list(KC.LOOP_CASES))
def test_the_loop_on_device_tensors(pkg, name):
    """channel_dev -> clock_dev(+p) -> sync_dev -> sync_extract_dev -> sco_dev; then clock_dev(clock_inverse_ppm(estimate)) on
    that capture -> sync -> extract -> demod_dev and sco_dev, at the operating points tests/test_clock_cpu.py establishes."""
    import torch
    from tests import channel_model as CM
    from tests.sync_model import extract_slots, geometry
    x, mode, bits, early, ppm, (paths, sigma, seed) = KC.loop_case(name, pkg.channel_sigma)
    want = KM.loop_model(pkg, x, mode, ppm, early, bits, CM.Channel(paths, sigma, seed))
    tf = geometry(mode)["tf"]
    m = pkg.Modulator(mode=mode, max_frames=2)
    try:
        m.set_channel(paths, sigma, seed)
        d_x = torch.from_numpy(np.array(x)).cuda()
        d_rx = torch.zeros_like(d_x)
        m.channel_dev(d_x, d_rx)
        d_ref = torch.from_numpy(bits.copy()).cuda()
        d_bits = torch.zeros((2, m.geometry["tf_input_bytes"]), dtype=torch.uint8, device="cuda")

        def receive(d_cap):
            m.sync_dev(d_cap, 31)
            d_frames = torch.zeros((extract_slots(d_cap.numel(), mode, 2), tf), dtype=torch.complex64, device="cuda")
            m.sync_extract_dev(d_cap, d_frames)
            found = m.sync_result()
            m.demod_dev(d_frames[:2].contiguous(), 2, early, d_bits, d_ref)
            m.sco_dev(d_frames[:2].contiguous(), 2, early)
            torch.cuda.synchronize()
            st = [m.monitor_stats(f) for f in range(2)]
            return dict(starts=[f["start"] for f in found], shifts=[f["shift"] for f in found], valid=[f["valid"] for f in found],
                        bit_errors=[s["bit_errors"] for s in st],
                        ratio=sum(s["sum_quadrature"] for s in st) / sum(s["sum_signal"] for s in st),
                        estimate=m.sco_result(-1)["ppm"])

        def through_clock(d_in, p):
            m.set_clock(p)
            d_out = torch.zeros(pkg.clock_out_max(d_in.numel()), dtype=torch.complex64, device="cuda")
            n = m.clock_dev(d_in, d_out)
            assert n == pkg.clock_count(p, d_in.numel())
            return d_out[:n].contiguous()

        d_cap = through_clock(d_rx, ppm)
        first = receive(d_cap)
        second = receive(through_clock(d_cap, pkg.clock_inverse_ppm(first["estimate"])))
        for k, got in (("first", first), ("second", second)):
            w = want[k]
            print("%s %s: starts %s shifts %s bit errors %s, sum_quadrature / sum_signal %.6g (model %.6g), estimate %.4f ppm (model %.4f)"
                  % (name, k, got["starts"], got["shifts"], got["bit_errors"], got["ratio"], w["ratio"], got["estimate"], w["estimate"]))
            for key in ("starts", "shifts", "valid", "bit_errors"):
                assert got[key] == w[key], (k, key, got[key], w[key])
        assert abs(first["estimate"] - ppm) <= max(0.5, 0.01 * abs(ppm))
        assert abs(second["estimate"]) <= 0.5
        assert second["bit_errors"] == [0, 0]
        assert abs(second["ratio"] - want["second"]["ratio"]) <= 1e-3 * want["second"]["ratio"]
        assert second["ratio"] < first["ratio"]
    finally:
        m.close()


# --------------------------------------------------------------------------- 7. behind the lanes
B, STAGES, MODE = 256, 3, 2                        # (frames per chain call, GainControl and FIRFilter: tests/receive_lanes_ops.py)


def _directed(pkg, d_bits, lanes):
    """As tests/test_receive_lanes_gpu.py: a rehearsal, every step waited for; then three chain calls (the third, on lane 2,
    writes the capture), clock_dev and sco_dev (early 44: behind FIRFilter) queued on it, a chain call on lane 0 and one on lane 1 that overwrites the capture.  With one
    lane every step is waited for.  -> (the clock's output bytes and count, lanes the calls went over, the capture's bytes)"""
    import torch
    md = pkg.Modulator(mode=MODE, max_frames=B)
    try:
        tf = md.geometry["tf_samples"]
        md.set_lanes(lanes)
        md.set_gain(2, 1.0, 0.5, 4.0)
        md.set_clock(100.0)
        cap, spare0, spare1 = (torch.zeros(B * tf, dtype=torch.complex64, device="cuda") for _ in range(3))
        rx = torch.zeros(pkg.clock_out_max(B * tf), dtype=torch.complex64, device="cuda")
        torch.cuda.synchronize()
        md.chain_dev_queued(d_bits[1], B, STAGES, spare0)
        md.synchronize()
        md.clock_dev(spare0, rx, queued=True)
        md.sco_dev(spare0, B, 44, queued=True)
        md.synchronize()
        md.clock_reset(0)
        rx.zero_()
        torch.cuda.synchronize()
        md.set_lanes(lanes)
        step = md.synchronize if lanes == 1 else (lambda: None)
        for src, dst in ((1, spare0), (2, spare1), (0, cap)):
            md.chain_dev_queued(d_bits[src], B, STAGES, dst)
            step()
        created = md.lanes_info()[0]
        count = md.clock_dev(cap, rx, queued=True)
        step()
        md.sco_dev(cap, B, 44, queued=True)
        step()
        md.chain_dev_queued(d_bits[3], B, STAGES, spare0)
        step()
        md.chain_dev_queued(d_bits[4], B, STAGES, cap)
        md.synchronize()
        records = [md.sco_result(f)["raw"] for f in (0, B - 1, -1)]
        return torch.view_as_real(rx).clone(), count, created, torch.view_as_real(cap).clone(), records
    finally:
        md.close()


def test_a_queued_call_between_the_chain_call_it_reads_and_the_one_that_overwrites(pkg):
    import torch
    md = pkg.Modulator(mode=MODE, max_frames=1)
    per = md.geometry["tf_input_bytes"]
    md.close()
    d_bits = torch.from_numpy(np.random.RandomState(9).randint(0, 256, (5, B, per)).astype(np.uint8)).cuda()
    want, n1, one, cap1, rec1 = _directed(pkg, d_bits, 1)
    got, n3, three, cap3, rec3 = _directed(pkg, d_bits, 3)
    assert rec3 == rec1 and all(any(r) for r in rec1)
    assert (one, three) == (1, 3) and n1 == n3 > 0
    assert bool(want.any()) and torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert torch.equal(cap3.view(torch.int32), cap1.view(torch.int32))
