"""Batches in flight inside ONE context (the lanes of include/dabgpu.h; idiom: PipelinedModCodec,
/root/reference/src/ModPlugin.cpp:90-154) and the hand-over FIRFilter -> Resampler in cache-sized pieces
(order of /root/reference/src/DabModulator.cpp:403-406; arithmetic of /root/reference/src/Resampler.cpp:142-192).

The bar for both is the strictest there is: the same BYTES as the serial, one-piece path -- frames are independent
units and the resampler's state runs through the pieces, so neither may change a single sample -- and the serial
path is the one the parity tests hold against the oracle (the first case below checks that directly as well).
"""
import numpy as np
import pytest

import oracle as O
from tests.conftest import load_pkg
from tests.golden.synth import POLY_AM, POLY_PM, synth_bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    return load_pkg()


def rel_rms(y, ref):
    return float(np.linalg.norm(y.astype(np.complex128) - ref) / max(np.linalg.norm(ref), 1e-30))


def _u32(t):
    import torch
    return torch.view_as_real(t).view(torch.int32) if t.is_complex() else t.view(torch.int32)


@pytest.mark.parametrize("lanes", [2, 3, 4])
def test_64_alternating_batches_equal_the_serial_result_frame_for_frame(pkg, lanes):
    """64 batches of 16 frames handed to ONE context on its own stream, rotating over the lanes, against the same 64
    batches with one lane (every call in order on one stream): identical bytes, batch for batch; and the first and last
    batch against the oracle."""
    import torch
    nb, B, stages = 64, 16, pkg.STAGE_GAIN | pkg.STAGE_FIR
    per = O.tf_input_bytes(1)
    rs = np.random.RandomState(77)
    bits = np.frombuffer(rs.bytes(nb * B * per), np.uint8).reshape(nb, B, per)
    d_bits = torch.from_numpy(bits.copy()).cuda()
    outs = {}
    for n in (1, lanes):
        md = pkg.Modulator(mode=1, max_frames=B)
        try:
            md.set_gain(pkg.GAIN_VAR, 1.0, 1.0 / 50000.0, 4.0)
            md.set_lanes(n)
            d_out = torch.zeros((nb, B, 196608), dtype=torch.complex64, device="cuda")
            torch.cuda.synchronize()
            for i in range(nb):
                md.chain_dev_queued(d_bits[i], B, stages, d_out[i])
            md.synchronize()
            outs[n] = d_out
        finally:
            md.close()
    assert bool((_u32(outs[1]) == _u32(outs[lanes])).all())
    ch = O.Chain(mode=1, stages=3, gain_mode=2, normalise=1.0 / 50000.0)
    for i in (0, nb - 1):
        ref = ch.process(bits[i])
        y = outs[lanes][i].cpu().numpy()
        for f in range(B):
            assert rel_rms(y[f], ref[f]) < 1e-6


def test_lanes_are_ordered_against_a_caller_stream_by_the_two_fences(pkg):
    """Input written on the caller's stream right before the calls, output read on it right after: correct through
    dabgpu_wait_for_stream / dabgpu_stream_wait_for alone, without any host synchronisation in between."""
    import torch
    B, stages = 8, pkg.STAGE_GAIN | pkg.STAGE_FIR
    per = O.tf_input_bytes(1)
    bits = np.stack([synth_bits(per, seed=3100 + i) for i in range(4 * B)]).reshape(4, B, per)
    md = pkg.Modulator(mode=1, max_frames=B)
    try:
        md.set_gain(pkg.GAIN_VAR, 1.0, 1.0 / 50000.0, 4.0)
        st = torch.cuda.Stream()
        src = torch.from_numpy(bits).cuda()
        torch.cuda.synchronize()
        with torch.cuda.stream(st):
            d_bits = torch.zeros_like(src)
            d_out = torch.zeros((4, B, 196608), dtype=torch.complex64, device="cuda")
            acc = torch.zeros((4, B), dtype=torch.float32, device="cuda")
            for rep in range(3):
                # (a long-running filler in front, so that an unordered lane would certainly overtake it)
                big = torch.empty(1 << 28, dtype=torch.float32, device="cuda")
                for _ in range(3):
                    big.fill_(1.0)
                d_bits.copy_(src if rep == 2 else src.flip(0), non_blocking=True)
                md.wait_for_stream(st.cuda_stream)
                for i in range(4):
                    md.chain_dev_queued(d_bits[i], B, stages, d_out[i])
                md.stream_wait_for(st.cuda_stream)
                acc.copy_(d_out.abs().sum(dim=-1))
            got = d_out.clone()
        st.synchronize()
        y = got.cpu().numpy()
        ch = O.Chain(mode=1, stages=3, gain_mode=2, normalise=1.0 / 50000.0)
        for i in range(4):
            ref = ch.process(bits[i])
            for f in range(B):
                assert rel_rms(y[i, f], ref[f]) < 1e-6
        assert np.allclose(acc.cpu().numpy(), np.abs(y).sum(axis=-1), rtol=1e-4)
    finally:
        md.close()


def test_lane_scratch_is_per_lane_for_the_chains_that_need_some(pkg):
    """Chains with per-call scratch (s16 through the separate FormatConverter kernel, TII with per-frame gains, CFR
    statistics, the windowed guard interval): rotating over four lanes gives the bytes of one lane, and the clip count /
    CFR statistics asked for afterwards are those of the LAST call."""
    import torch
    B = 4
    per = O.tf_input_bytes(1)
    bits = np.stack([synth_bits(per, seed=3300 + i) for i in range(6 * B)]).reshape(6, B, per)
    d_bits = torch.from_numpy(bits).cuda()

    def run(lanes, setup, fmt=None):
        md = pkg.Modulator(mode=1, max_frames=B)
        try:
            md.set_gain(pkg.GAIN_VAR, 1.0, 1.0 if fmt else 1.0 / 50000.0, 4.0)
            setup(md)
            md.set_output_format(fmt)
            md.set_lanes(lanes)
            stages = pkg.STAGE_GAIN | pkg.STAGE_FIR
            ns = md.out_samples_per_frame(stages)
            d_out = torch.zeros((6, B, ns), dtype=torch.complex64 if fmt is None else torch.int32, device="cuda")
            torch.cuda.synchronize()
            for i in range(6):
                md.chain_dev_queued(d_bits[i], B, stages, d_out[i])
            md.synchronize()
            extra = md.num_clipped() if fmt else None
            return d_out, extra
        finally:
            md.close()

    cases = {
        "s16 + windowed guard (FormatConverter kernel, d_fmt + d_b)": (lambda md: md.set_window_overlap(24), "s16"),
        "TII + max gain (per-frame gain of symbol 1)": (lambda md: (md.set_tii(True, 3, 5), md.set_gain(1, 1.0, 1.0, 4.0)), None),
        "long filter (IFFT kernel -> guard_fir_kernel through d_b)": (lambda md: md.set_fir_taps(np.hanning(201).astype(np.float32) / 100), None),
    }
    for name, (setup, fmt) in cases.items():
        a, ca = run(1, setup, fmt)
        b, cb = run(4, setup, fmt)
        assert bool((_u32(a) == _u32(b)).all()), name
        assert ca == cb, name

    # CFR: the statistics of the most recent call, whichever lane ran it
    def cfr_stats(lanes):
        md = pkg.Modulator(mode=1, max_frames=B)
        try:
            md.set_gain(pkg.GAIN_VAR, 1.0, 1.0 / 50000.0, 4.0)
            md.set_cfr(True, 50.0, 0.1)
            md.set_lanes(lanes)
            d_out = torch.zeros((6, B, 196608), dtype=torch.complex64, device="cuda")
            for i in range(6):
                md.chain_dev_queued(d_bits[i], B, 3, d_out[i])
            st = [md.cfr_stats(f) for f in range(B)]
            md.synchronize()
            return d_out, st
        finally:
            md.close()
    a, sa = cfr_stats(1)
    b, sb = cfr_stats(3)
    assert bool((_u32(a) == _u32(b)).all())
    for x, y in zip(sa, sb):
        assert x["num_clip"] == y["num_clip"] and x["num_error_clip"] == y["num_error_clip"] and x["mer_symbol"] == y["mer_symbol"]
        assert np.array_equal(x["papr_after"], y["papr_after"])


def test_submit_collect_on_two_lanes_equals_the_synchronous_call(pkg):
    """The asynchronous host path keeps its two batches on two lanes now: same bytes as dabgpu_chain_process, in order."""
    B = 6
    per = O.tf_input_bytes(1)
    bits = np.stack([synth_bits(per, seed=3500 + i) for i in range(5 * B)]).reshape(5, B, per)
    md = pkg.Modulator(mode=1, max_frames=B)
    try:
        md.set_gain(pkg.GAIN_VAR, 1.0, 1.0 / 50000.0, 4.0)
        want = [md.chain(bits[i], 3).copy() for i in range(5)]
        got = []
        md.submit(bits[0], 3)
        for i in range(1, 5):
            md.submit(bits[i], 3)
            got.append(md.collect())
        got.append(md.collect())
        for i in range(5):
            assert np.array_equal(got[i].view(np.uint32).ravel(), want[i].view(np.uint32).ravel()), i
    finally:
        md.close()


@pytest.mark.parametrize("fmt", [None, "s16"])
@pytest.mark.parametrize("piece", [2, 6, 10])
def test_cfg4_handover_in_pieces_equals_one_piece_byte_for_byte(pkg, piece, fmt):
    """cfg 4 (FIRFilter -> Resampler x4 -> MemlessPoly) with the native-rate stream handed over in pieces of 2 / 6 / 10
    frames through the two-piece ring, against the one-piece path: 23 frames (ragged last piece), two consecutive calls
    (the resampler's state crosses pieces AND calls) -- the same bytes; and the one-piece path against the oracle."""
    import torch
    B = 23
    per = O.tf_input_bytes(1)
    bits = np.stack([synth_bits(per, seed=3700 + i) for i in range(2 * B)]).reshape(2, B, per)
    d_bits = torch.from_numpy(bits).cuda()
    stages = pkg.STAGE_GAIN | pkg.STAGE_FIR | pkg.STAGE_RESAMPLE | pkg.STAGE_POLY
    res = {}
    for p in (0, piece):
        md = pkg.Modulator(mode=1, max_frames=B)
        try:
            md.set_gain(pkg.GAIN_VAR, 1.0, 0.6 if fmt else 1.0 / 50000.0, 4.0)
            md.set_resampler(2048000, 8192000)
            md.set_poly(POLY_AM, POLY_PM)
            md.set_output_format(fmt)
            md.set_handover_frames(p)
            ns = md.out_samples_per_frame(stages)
            d_out = torch.zeros((2, B, ns), dtype=torch.complex64 if fmt is None else torch.int32, device="cuda")
            md.trace(True)
            for i in range(2):
                md.chain_dev(d_bits[i], B, stages, d_out[i])
            torch.cuda.synchronize()
            kernels = md.last_variant()
            res[p] = (d_out, md.num_clipped() if fmt else None, kernels)
        finally:
            md.close()
    assert bool((_u32(res[0][0]) == _u32(res[piece][0])).all())
    assert res[0][1] == res[piece][1]
    # the pieces really ran: one frame kernel + one resampler per piece
    npieces = -(-B // piece)
    assert sum(k.startswith("tf_kernel") for k in res[piece][2]) == npieces
    assert sum(k.startswith("resampler16_kernel") for k in res[piece][2]) == npieces
    assert sum(k.startswith("tf_kernel") for k in res[0][2]) == 1
    if fmt is None:
        ch = O.Chain(mode=1, stages=15, gain_mode=2, normalise=1.0 / 50000.0, out_rate=8192000, am=POLY_AM, pm=POLY_PM)
        y = res[piece][0].cpu().numpy()
        for i in range(2):
            ref = ch.process(bits[i])
            for f in (0, 1, piece, B - 1):
                assert rel_rms(y[i, f], ref[f]) < 1e-6


def test_handover_pieces_from_carriers_and_x2(pkg):
    """The same through the carriers entry point (SignalMultiplexer output) and the x2 ratio without predistorter."""
    import torch
    B = 9
    md0 = pkg.Modulator(mode=1, max_frames=B)
    K = md0.geometry["carriers"]
    md0.close()
    rs = np.random.RandomState(5)
    q = rs.randint(0, 4, size=(B, 77 * K))
    car = np.exp(1j * (2 * q + 1) * np.pi / 4).astype(np.complex64)
    car[:, :K] = 0
    d_car = torch.from_numpy(car).cuda()
    stages = pkg.STAGE_GAIN | pkg.STAGE_FIR | pkg.STAGE_RESAMPLE
    res = {}
    for p in (0, 4):
        md = pkg.Modulator(mode=1, max_frames=B)
        try:
            md.set_gain(pkg.GAIN_VAR, 1.0, 1.0 / 50000.0, 4.0)
            md.set_resampler(2048000, 4096000)
            md.set_handover_frames(p)
            d_out = torch.zeros((B, 2 * 196608), dtype=torch.complex64, device="cuda")
            md.symbols_dev(d_car, B, stages, d_out)
            torch.cuda.synchronize()
            res[p] = d_out
        finally:
            md.close()
    assert bool((_u32(res[0]) == _u32(res[4])).all())


def test_post_process_dev_is_the_tail_of_the_chain(pkg):
    """dabgpu_post_process_dev (cifRes -> cifPoly on a device-resident native-rate stream) after the native chain ==
    the fused chain with the same stages, byte for byte, state carried across two calls; bad arguments are refused."""
    import torch
    B = 3
    per = O.tf_input_bytes(1)
    bits = np.stack([synth_bits(per, seed=3900 + i) for i in range(2 * B)]).reshape(2, B, per)
    d_bits = torch.from_numpy(bits).cuda()
    full = pkg.STAGE_GAIN | pkg.STAGE_FIR | pkg.STAGE_RESAMPLE | pkg.STAGE_POLY

    def make():
        md = pkg.Modulator(mode=1, max_frames=B)
        md.set_gain(pkg.GAIN_VAR, 1.0, 1.0 / 50000.0, 4.0)
        md.set_resampler(2048000, 8192000)
        md.set_poly(POLY_AM, POLY_PM)
        return md
    a, b = make(), make()
    try:
        for i in range(2):
            want = torch.zeros((B, 4 * 196608), dtype=torch.complex64, device="cuda")
            a.chain_dev(d_bits[i], B, full, want)
            native = torch.zeros((B, 196608), dtype=torch.complex64, device="cuda")
            b.chain_dev(d_bits[i], B, pkg.STAGE_GAIN | pkg.STAGE_FIR, native)
            got = torch.zeros_like(want)
            b.post_process_dev(native, pkg.STAGE_RESAMPLE | pkg.STAGE_POLY, got)
            torch.cuda.synchronize()
            assert bool((_u32(want) == _u32(got)).all()), i
        with pytest.raises(pkg.DabGpuError, match="post-processing"):
            b.post_process_dev(native, pkg.STAGE_FIR, got)
        with pytest.raises(pkg.DabGpuError, match="input size not valid"):
            b.post_process_dev(native.reshape(-1)[:1000], pkg.STAGE_RESAMPLE, got)
    finally:
        a.close()
        b.close()


def test_set_lanes_and_handover_arguments(pkg):
    md = pkg.Modulator(mode=1, max_frames=1)
    try:
        for bad in (0, 5, -1):
            with pytest.raises(pkg.DabGpuError, match="lanes"):
                md.set_lanes(bad)
        for bad in (-2, 3):
            with pytest.raises(pkg.DabGpuError, match="hand-over"):
                md.set_handover_frames(bad)
        md.set_lanes(4)
        md.set_handover_frames(64)
    finally:
        md.close()


def test_chain_out_buffer_must_be_the_callers_memory(pkg):
    """Modulator.chain(out=...): a non-contiguous or mistyped reuse buffer is refused BEFORE any reshape could silently copy
    it (advisor, round 4: the result used to land in the copy and the caller's buffer stayed empty)."""
    md = pkg.Modulator(mode=2, max_frames=2)
    try:
        md.set_gain(pkg.GAIN_VAR, 1.0, 1.0 / 50000.0, 4.0)
        per = md.geometry["tf_input_bytes"]
        bits = np.stack([synth_bits(per, seed=4100 + i) for i in range(2)])
        ns = md.out_samples_per_frame(3)
        good = np.zeros((2, ns), np.complex64)
        y = md.chain(bits, 3, out=good)
        assert np.shares_memory(y, good) and np.abs(good).max() > 0
        wide = np.zeros((2, 2 * ns), np.complex64)
        for bad in (wide[:, ::2], np.zeros((2, ns), np.complex128), np.zeros((2, ns + 1), np.complex64)):
            with pytest.raises(pkg.DabGpuError, match="output buffer does not match"):
                md.chain(bits, 3, out=bad)
        assert np.abs(wide).max() == 0
    finally:
        md.close()


def test_lanes_get_hardware_queues_of_their_own_whatever_came_before(pkg):
    """The HIP runtime puts a new stream on whichever of its (four) hardware queues holds the fewest, so three streams created
    in a row share queues or not depending on the process's history -- and lanes that share one run in order.  Lane streams
    are probed and replaced until they overlap with one another: after contexts have come and gone in uneven numbers, a
    fresh context still reports a queue of its own for each of its three lanes."""
    import torch
    junk = [torch.cuda.Stream() for _ in range(5)]                    # an uneven number of other streams in the process
    for n in (1, 2, 3, 2):
        md = pkg.Modulator(mode=1, max_frames=2)
        try:
            md.set_gain(pkg.GAIN_VAR, 1.0, 1.0 / 50000.0, 4.0)
            md.set_lanes(3)
            d_bits = torch.zeros((2, 28800), dtype=torch.uint8, device="cuda")
            d_out = torch.zeros((2, 196608), dtype=torch.complex64, device="cuda")
            for _ in range(2 * n):
                md.chain_dev_queued(d_bits, 2, 3, d_out)
            md.synchronize()
            count, own = md.lanes_info()
            assert count == min(3, 2 * n) and all(own), (n, count, own)
        finally:
            md.close()
    del junk


def test_setters_from_another_thread_while_batches_are_in_flight_on_the_lanes(pkg):
    """The remote-control contract with the lanes: a thread toggles digital gain and the taps (a table that
    is rewritten on the device) while the processing thread keeps three batches in flight.  Every frame must come out under ONE
    consistent snapshot -- scale 1, 1/2 or 1/4 of the base frame, never a mixture -- which also proves that a table is only
    rewritten once every lane has drained."""
    import threading
    import torch
    md = pkg.Modulator(mode=2, max_frames=2)
    try:
        md.set_gain(2, 1.0, 1.0 / 50000.0, 4.0)
        per = md.geometry["tf_input_bytes"]
        bits = np.stack([synth_bits(per, seed=4300), synth_bits(per, seed=4301)])
        taps = O.fir_default_taps()
        base = O.Chain(mode=2, stages=3, gain_mode=2, normalise=1.0 / 50000.0).process(bits)
        ns = md.out_samples_per_frame(3)
        d_bits = torch.from_numpy(bits).cuda()
        outs = [torch.zeros((2, ns), dtype=torch.complex64, device="cuda") for _ in range(6)]
        stop = threading.Event()

        def rc_thread():
            i = 0
            while not stop.is_set():
                md.set_gain(2, 1.0 if i & 1 else 0.5, 1.0 / 50000.0, 4.0)
                md.set_fir_taps(taps if i & 2 else taps * np.float32(0.5))
                i += 1

        t = threading.Thread(target=rc_thread)
        t.start()
        seen = set()
        try:
            for _ in range(60):
                for o in outs:
                    md.chain_dev_queued(d_bits, 2, 3, o)
                md.synchronize()
                for o in outs:
                    y = o.cpu().numpy()
                    for f in range(2):
                        k = float(np.vdot(base[f], y[f]).real / np.vdot(base[f], base[f]).real)
                        scale = min((1.0, 0.5, 0.25), key=lambda c: abs(c - k))
                        assert rel_rms(y[f], base[f] * np.float32(scale)) < 2e-6, k
                        seen.add(scale)
        finally:
            stop.set()
            t.join()
        assert len(seen) >= 2
    finally:
        md.close()


@pytest.mark.parametrize("case", ["cfg4", "cfg4_s16", "x2_lut", "tii_cfr", "rational"])
def test_resampler_chains_on_the_contexts_own_stream_are_one_stream(pkg, case):
    """A chain with the Resampler on the context's own stream stays on lane 0, in call order (its state runs from call to call)
    -- whatever dabgpu_set_lanes says.  Twelve calls of five frames as ONE stream (the halo crosses every call; the x2 / x4
    kernel writes it itself, into the other of two buffers) with three lanes set against one: the same bytes, for cfg 4, its
    s16 form, x2 with the LUT predistorter (a separate kernel behind the resampler), TII + CFR in front, and a rational ratio
    (the general kernel, halo copied behind it); cfg 4 also against the oracle's stream."""
    import torch
    B, calls = 5, 12
    per = O.tf_input_bytes(1)
    bits = np.stack([synth_bits(per, seed=4500 + i) for i in range(B * calls)]).reshape(calls, B, per)
    d_bits = torch.from_numpy(bits).cuda()
    stages = pkg.STAGE_GAIN | pkg.STAGE_FIR | pkg.STAGE_RESAMPLE | pkg.STAGE_POLY
    fmt = "s16" if case == "cfg4_s16" else None
    outs, extra = {}, {}
    for lanes in (1, 3):
        md = pkg.Modulator(mode=1, max_frames=B)
        try:
            md.set_gain(pkg.GAIN_VAR, 1.0, 0.6 if fmt else 1.0 / 50000.0, 4.0)
            rate = {"x2_lut": 4096000, "rational": 3072000}.get(case, 8192000)
            md.set_resampler(2048000, rate)
            if case == "x2_lut":
                md.set_lut(1.0 / 32768, np.linspace(1.0, 1.2, 32).astype(np.float32))
            else:
                md.set_poly(POLY_AM, POLY_PM)
            if case == "tii_cfr":
                md.set_tii(True, 3, 5)
                md.set_cfr(True, 50.0, 0.1)
            md.set_output_format(fmt)
            md.set_lanes(lanes)
            ns = md.out_samples_per_frame(stages)
            d_out = torch.zeros((calls, B, ns), dtype=torch.complex64 if fmt is None else torch.int32, device="cuda")
            torch.cuda.synchronize()
            for i in range(calls):
                md.chain_dev_queued(d_bits[i], B, stages, d_out[i])
            md.synchronize()
            outs[lanes] = d_out
            extra[lanes] = (md.num_clipped() if fmt else None, md.cfr_stats(B - 1)["num_clip"] if case == "tii_cfr" else None)
        finally:
            md.close()
    assert bool((_u32(outs[1]) == _u32(outs[3])).all())
    assert extra[1] == extra[3]
    if case == "cfg4":
        ch = O.Chain(mode=1, stages=15, gain_mode=2, normalise=1.0 / 50000.0, out_rate=8192000, am=POLY_AM, pm=POLY_PM)
        ref = ch.process(bits.reshape(calls * B, per))
        y = outs[3].cpu().numpy().reshape(calls * B, -1)
        for f in (0, 1, B, 3 * B + 2, calls * B - 1):
            assert rel_rms(y[f], ref[f]) < 1e-6, f


def test_three_threads_three_contexts_each_on_its_own_lanes(pkg):
    """A head-end with several multiplexes: three host threads, one context each, every context with three lanes (nine internal
    streams probed for hardware queues while the other threads are already launching), different settings per context, twenty
    calls of four frames each on the context's own stream -- every frame against the oracle."""
    import threading
    import torch
    per = O.tf_input_bytes(1)
    B, calls = 4, 20
    kws = [dict(gain_mode=2, normalise=1.0 / 50000.0), dict(gain_mode=1, normalise=1.0), dict(gain_mode=0, normalise=1.0 / 4000.0)]
    bits = [np.stack([synth_bits(per, seed=4700 + 100 * k + i) for i in range(B)]) for k in range(3)]
    refs = [O.Chain(mode=1, stages=3, **kws[k]).process(bits[k]) for k in range(3)]
    results, errors = [None] * 3, []

    def run(k):
        try:
            md = pkg.Modulator(mode=1, max_frames=B)
            md.set_gain(kws[k]["gain_mode"], 1.0, kws[k]["normalise"], 4.0)
            d_bits = torch.from_numpy(bits[k]).cuda()
            outs = [torch.zeros((B, 196608), dtype=torch.complex64, device="cuda") for _ in range(4)]
            torch.cuda.synchronize()
            for i in range(calls):
                md.chain_dev_queued(d_bits, B, 3, outs[i & 3])
            md.synchronize()
            results[k] = ([o.cpu().numpy() for o in outs], md.lanes_info())
            md.close()
        except Exception as e:          # surfaced in the main thread below
            errors.append(repr(e))

    threads = [threading.Thread(target=run, args=(k,)) for k in range(3)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for k in range(3):
        outs, (n, own) = results[k]
        assert n == 3
        for o in outs:
            for f in range(B):
                assert rel_rms(o[f], refs[k][f]) < 1e-6, (k, f)


# ---- advisor findings of round 5: ordering and shared state between the lanes --------------------------------------------
def test_null_stream_tail_calls_are_ordered_behind_the_lanes(pkg):
    """C-ABI callers (no Python wrapper that synchronises in between): chain_process_dev(GAIN | FIR -> native, NULL) rotates
    over the lanes, post_process_dev(native, NULL) / format_process_dev(native, NULL) run on the context's own stream --
    they must start after the chain call that produced `native`, whichever lane it went to, and a later chain call that
    reuses the buffer must start after them.  Same bytes as one lane."""
    import torch
    B, R = 16, 9
    per = O.tf_input_bytes(1)
    bits = np.stack([synth_bits(per, seed=5100 + i) for i in range(R * B)]).reshape(R, B, per)
    d_bits = torch.from_numpy(bits).cuda()

    def run(lanes):
        md = pkg.Modulator(mode=1, max_frames=B)
        try:
            md.set_lanes(lanes)
            md.set_gain(pkg.GAIN_VAR, 1.0, 1.0 / 50000.0, 4.0)
            md.set_resampler(2048000, 8192000)
            md.set_poly(POLY_AM, POLY_PM)
            native = torch.zeros((B, 196608), dtype=torch.complex64, device="cuda")       # ONE buffer, reused by every round
            outs = [torch.zeros((B, 4 * 196608), dtype=torch.complex64, device="cuda") for _ in range(R)]
            ints = [torch.zeros((B, 2 * 196608), dtype=torch.int16, device="cuda") for _ in range(R)]
            torch.cuda.synchronize()
            for i in range(R):
                md.chain_dev_queued(d_bits[i], B, pkg.STAGE_GAIN | pkg.STAGE_FIR, native)
                md.post_process_dev_queued(native, pkg.STAGE_RESAMPLE | pkg.STAGE_POLY, outs[i])
                md.format_convert_dev_queued(native, "s16", ints[i])
            md.synchronize()
            return [o.clone() for o in outs], [o.clone() for o in ints]
        finally:
            md.close()
    want_o, want_i = run(1)
    got_o, got_i = run(3)
    for i in range(R):
        assert bool((_u32(want_o[i]) == _u32(got_o[i])).all()), i
        assert bool((want_i[i] == got_i[i]).all()), i
    # ... and the one-lane result is the oracle's
    ref = O.Chain(mode=1, stages=O.STAGE_GAIN | O.STAGE_FIR | O.STAGE_RESAMPLE | O.STAGE_POLY, normalise=1.0 / 50000.0,
                  out_rate=8192000, am=POLY_AM, pm=POLY_PM).process(bits[0][:2])
    y = want_o[0][:2].cpu().numpy()
    for f in range(2):
        assert rel_rms(y[f], ref[f]) < 1e-6


def test_tii_settings_toggled_while_batches_are_in_flight(pkg):
    """The TII segment (d_acp / d_tii_car / d_tii_frame) is ONE set of buffers shared by the lanes; a new comb / pattern
    rebuilds it.  While a thread toggles the pattern, every TII-carrying frame must be the frame of ONE of the two
    patterns -- never a torn segment."""
    import threading
    import torch
    md = pkg.Modulator(mode=1, max_frames=2)
    try:
        md.set_gain(2, 1.0, 1.0 / 50000.0, 4.0)
        per = md.geometry["tf_input_bytes"]
        bits = np.stack([synth_bits(per, seed=5200), synth_bits(per, seed=5201)])
        cands = [O.Chain(mode=1, stages=3, gain_mode=2, normalise=1.0 / 50000.0, tii=(3, p, False)).process(bits) for p in (5, 44)]
        assert rel_rms(cands[0][0], cands[1][0]) > 1e-3          # (the two patterns differ in the TII frame)
        ns = md.out_samples_per_frame(3)
        d_bits = torch.from_numpy(bits).cuda()
        outs = [torch.zeros((2, ns), dtype=torch.complex64, device="cuda") for _ in range(6)]
        md.set_tii(True, 3, 5)
        stop = threading.Event()

        def rc_thread():
            i = 0
            while not stop.is_set():
                md.set_tii(True, 3, 44 if i & 1 else 5)
                i += 1

        t = threading.Thread(target=rc_thread)
        t.start()
        seen = set()
        try:
            for _ in range(40):
                for o in outs:
                    md.chain_dev_queued(d_bits, 2, 3, o)          # two frames per call: the TII parity is the same for every call
                md.synchronize()
                for o in outs:
                    y = o.cpu().numpy()
                    errs = [rel_rms(y[0], c[0]) for c in cands]
                    assert min(errs) < 2e-6, errs
                    seen.add(int(np.argmin(errs)))
                    assert rel_rms(y[1], cands[0][1]) < 2e-6      # (the frame without TII)
        finally:
            stop.set()
            t.join()
        assert seen == {0, 1}
    finally:
        md.close()


def test_zero_length_resampler_call_leaves_the_stream_state_alone(pkg):
    """Resampler::process on an empty buffer (src/Resampler.cpp:131-140: nothing in, nothing out): the halo of the next
    call is still the one of the call before."""
    rng = np.random.RandomState(53)
    x = (rng.randn(3, 8 * 2048) + 1j * rng.randn(3, 8 * 2048)).astype(np.complex64) * np.float32(0.1)
    def run(with_empty):
        md = pkg.Modulator(mode=1, max_frames=1)
        try:
            md.set_resampler(2048000, 8192000)
            ys = []
            for i in range(3):
                ys.append(md.resample(x[i]).copy())
                if with_empty:
                    assert md.resample(np.zeros(0, np.complex64)).size == 0
            return np.concatenate(ys)
        finally:
            md.close()
    assert np.array_equal(run(False).view(np.uint32), run(True).view(np.uint32))


def test_cfr_statistics_are_those_of_the_most_recent_call_whichever_lane(pkg):
    """dabgpu_get_cfr_stats after the OfdmGenerator stage wrapper (lane 0) that follows chain calls on lanes 1 and 2: the
    wrapper's statistics, not the stale lane's."""
    import torch
    per = O.tf_input_bytes(1)
    bits = np.stack([synth_bits(per, seed=5400 + i) for i in range(2)])
    rng = np.random.RandomState(54)
    car = np.exp(1j * (np.pi / 4) * (2 * rng.randint(0, 4, size=(77, 1536)) + 1)).astype(np.complex64)
    car[0] = 0
    def stats(after_chain_calls):
        md = pkg.Modulator(mode=1, max_frames=2)
        try:
            md.set_gain(2, 1.0, 1.0 / 50000.0, 4.0)
            md.set_cfr(True, 45.0, 0.15)
            if after_chain_calls:
                d_bits = torch.from_numpy(bits).cuda()
                out = [torch.zeros((2, 196608), dtype=torch.complex64, device="cuda") for _ in range(2)]
                md.chain_dev_queued(d_bits, 2, 3, out[0])     # lane 0
                md.chain_dev_queued(d_bits, 2, 3, out[1])     # lane 1: the most recent chain call
                md.synchronize()
            md.ofdm(car)
            return md.cfr_stats(0)
        finally:
            md.close()
    a, b = stats(False), stats(True)
    assert a["num_clip"] > 0 and a["num_clip"] == b["num_clip"] and a["num_error_clip"] == b["num_error_clip"]
    assert np.array_equal(a["papr_before"], b["papr_before"]) and np.array_equal(a["papr_after"], b["papr_after"])
    # (the MER symbol rotates with the frames a context has seen, src/OfdmGenerator.cpp:198,250: another symbol of the same
    # frame after four chain frames -- the same power to a few ulps, not the same sum)
    assert abs(a["mer_sum_iq"] - b["mer_sum_iq"]) < 1e-5 * a["mer_sum_iq"]


_STRESS_OPS = int(__import__("os").environ.get("DABGPU_STRESS_OPS", "600"))     # (a one-off hunt: DABGPU_STRESS_OPS=3000)


def _stress_settings(rs):
    """One remote-control action of the kind that rewrites device tables or changes which kernels run."""
    k = rs.randint(8)
    if k == 0:
        gm, dg = int(rs.choice([0, 1, 2])), float(rs.choice([1.0, 0.8]))
        return "gain %d %.1f" % (gm, dg), lambda md: md.set_gain(gm, dg, 0.5, 4.0)
    if k == 1:
        on, comb, pat = bool(rs.randint(2)), int(rs.randint(1, 24)), int(rs.randint(0, 70))
        return "tii %d %d %d" % (on, comb, pat), lambda md: md.set_tii(on, comb, pat, False)
    if k == 2:
        on, clip = bool(rs.randint(2)), float(rs.choice([45.0, 60.0]))
        return "cfr %d %.0f" % (on, clip), lambda md: md.set_cfr(on, clip, 0.2)
    if k == 3:
        w = int(rs.choice([0, 0, 10, 24]))
        return "window %d" % w, lambda md: md.set_window_overlap(w)
    if k == 4:
        fmt = rs.choice([None, "s16", "u8"])
        fmt = None if fmt is None else str(fmt)
        return "format %s" % fmt, lambda md: md.set_output_format(fmt)
    if k == 5:
        n = int(rs.choice([45, 13, 101]))
        taps = None if n == 45 else (np.hanning(n) / np.hanning(n).sum()).astype(np.float32)
        return "taps %d" % n, lambda md: md.set_fir_taps(taps)
    if k == 6:
        ref = bool(rs.randint(2))
        return "gain rounding %d" % ref, lambda md: md.set_gain_rounding(ref)
    direct = bool(rs.randint(2))
    return "boundary mode %d" % direct, lambda md: md.set_fir_boundary_mode(direct)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_operation_sequences_on_three_lanes_equal_the_serial_context(pkg, seed):
    """A differential stress of the ordering rules of section 4.5: ONE random sequence of chain calls (1 ... 16 frames, with and
    without FIRFilter), of the entry points that stay on the context's own stream (dabgpu_post_process_dev with the resampler's
    stream state, dabgpu_format_process_dev) reading what an earlier call may still be writing on another lane, and of
    remote-control actions (gain, TII, CFR, window, output format, taps, gain rounding, boundary mode)
    runs twice -- on a context with three lanes, every call queued on the context's own stream and nothing waited for until
    the end; and on a one-lane context that is synchronised after every call.  Every call must leave the same BYTES: a
    setting changed while batches are in flight on other lanes (tables rewritten, the TII segment rebuilt, scratch reused)
    may neither tear an earlier batch nor miss a later one, and the stream state (TII frame parity, the CFR statistics'
    rotating symbol) must advance call by call."""
    import torch
    rs = np.random.RandomState(9000 + seed)
    per = O.tf_input_bytes(1)
    pool = torch.from_numpy(np.frombuffer(rs.bytes(16 * per), np.uint8).reshape(16, per).copy()).cuda()
    ops = []
    for _ in range(_STRESS_OPS):
        u = rs.rand()
        if u < 0.3:
            ops.append(("set",) + _stress_settings(rs))
        elif u < 0.4:
            # the entry points that do NOT rotate, fed with the most recent complexf output of a chain call -- which may still be
            # in flight on another lane: cifRes -> cifPoly on it (stream state: the resampler's two hops), or FormatConverter
            ops.append(("post",) if rs.rand() < 0.5 else ("convert", str(rs.choice(["s16", "u8"]))))
        else:
            B = int(rs.choice([1, 1, 2, 3, 5, 16]))
            ops.append(("call", B, int(rs.randint(0, 16 - B + 1)), int(rs.choice([1, 3, 3]))))
    results = {}
    for lanes in (3, 1):
        md = pkg.Modulator(mode=1, max_frames=16)
        try:
            md.set_lanes(lanes)
            md.set_gain(2, 1.0, 0.5, 4.0)
            # every output buffer first, and torch's zero fills DONE before the first call: the library's lanes are streams of
            # their own, which torch's stream is not ordered against (dabgpu_wait_for_stream exists for callers that need it)
            md.set_resampler(2048000, 8192000)               # (for "post": cifRes x4 -> cifPoly; the chain calls stay at the native rate)
            md.set_poly(POLY_AM, POLY_PM)
            outs, fmt, plan, last = [], None, [], None       # plan: per op, (kind, index of its output, index of its input)
            for op in ops:
                if op[0] == "set":
                    if op[1].startswith("format"):
                        fmt = None if op[1].endswith("None") else op[1].split()[1]
                    plan.append(None)
                    continue
                if op[0] == "call":
                    n = op[1] * 196608
                    outs.append(torch.zeros(n, dtype=torch.complex64, device="cuda") if fmt is None else
                                torch.zeros(2 * n, dtype=torch.int16 if fmt == "s16" else torch.uint8, device="cuda"))
                    plan.append(("call", len(outs) - 1, None))
                    if fmt is None and op[1] <= 3:
                        last = len(outs) - 1
                    continue
                if last is None:
                    plan.append(None)
                    continue
                n = outs[last].numel()
                if op[0] == "post":
                    outs.append(torch.zeros(4 * n, dtype=torch.complex64, device="cuda"))
                else:
                    outs.append(torch.zeros(2 * n, dtype=torch.int16 if op[1] == "s16" else torch.uint8, device="cuda"))
                plan.append((op[0], len(outs) - 1, last))
            torch.cuda.synchronize()
            for op, pl in zip(ops, plan):
                if op[0] == "set":
                    op[2](md)
                    continue
                if pl is None:
                    continue
                if pl[0] == "call":
                    _, B, at, stages = op
                    md.chain_dev_queued(pool[at:at + B], B, stages, outs[pl[1]])
                elif pl[0] == "post":
                    md.post_process_dev_queued(outs[pl[2]], pkg.STAGE_RESAMPLE | pkg.STAGE_POLY, outs[pl[1]])
                else:
                    md.format_convert_dev_queued(outs[pl[2]], op[1], outs[pl[1]])
                if lanes == 1:
                    md.synchronize()
            md.synchronize()
            results[lanes] = outs
        finally:
            md.close()
    assert len(results[1]) == len(results[3]) > 0
    for j, (a, b) in enumerate(zip(results[3], results[1])):
        assert a.dtype == b.dtype and a.numel() == b.numel()
        assert bool((_u32(a) == _u32(b)).all()) if a.dtype == torch.complex64 else bool((a == b).all()), j
    # ... and the work was real: the outputs are not the zeros they were allocated as
    assert sum(int(bool(o.view(torch.uint8).any())) for o in results[3]) >= len(results[3]) - 1


@pytest.mark.parametrize("case", ["gain_replay_s16_poly", "mode3_101_taps"])
def test_calls_whose_scratch_exceeds_the_lane_bound_stay_on_lane_0(pkg, case):
    """A call rotates over the lanes only while the per-lane scratch IT reserves stays within kLaneScratchBytes (256 MiB):
    the bound is the call's own plan, not an estimate.  Sizes per frame, from the chain's plan (arithmetic, bytes):
      gain_replay_s16_poly (Mode I; gain mode var by the reference's recurrence, s16, GAIN | FIR | POLY): the symbols in
        front of the guard kernel 77 x 2048 x 8, the native-rate stream in front of the predistorter and the complexf stream in
        front of FormatConverter 196608 x 8 each, 77 multipliers x 4 = 4 407 604: 282 MB at 64 frames (a two-buffer estimate says
        201 MB), 71 MB at 16;
      mode3_101_taps (Mode III, GAIN | FIR with a filter that fits the fused kernel's tap limit but not the cyclic prefix of
        63 samples): the symbols in front of the guard / FIRFilter kernel 154 x 256 x 8 = 315 392: 323 MB at 1024 frames, 5 MB at 16.
    Three calls on the context's own stream: the large ones leave no lane stream beyond the context's own behind, the
    small ones (the control) create the other two.
    (The third case the lane bound used to miss on paper, CFR from carriers without FIRFilter, has no separating batch size:
    it reserves 1.26 MB per frame where the old estimate assumed 3.1 MB -- it rotated less than it may, never more.)"""
    import torch
    mode, big, stages = (1, 64, pkg.STAGE_GAIN | pkg.STAGE_FIR | pkg.STAGE_POLY) if case == "gain_replay_s16_poly" \
        else (3, 1024, pkg.STAGE_GAIN | pkg.STAGE_FIR)
    for B, lanes_created in ((big, 1), (16, 3)):
        md = pkg.Modulator(mode=mode, max_frames=B)
        try:
            md.set_gain(pkg.GAIN_VAR, 1.0, 1.0, 4.0)
            if case == "gain_replay_s16_poly":
                md.set_gain_rounding(True)
                md.set_poly(POLY_AM, POLY_PM)
                md.set_output_format("s16")
            else:
                md.set_fir_taps(np.hanning(101).astype(np.float32) / 50)
            md.set_lanes(3)
            d_bits = torch.zeros((B, O.tf_input_bytes(mode)), dtype=torch.uint8, device="cuda")
            d_out = torch.zeros((B, md.out_samples_per_frame(stages)), dtype=torch.int32 if mode == 1 else torch.complex64,
                                device="cuda")
            for _ in range(3):
                md.chain_dev_queued(d_bits, B, stages, d_out)
            md.synchronize()
            assert md.lanes_info()[0] == lanes_created, (case, B, md.lanes_info())
        finally:
            md.close()
