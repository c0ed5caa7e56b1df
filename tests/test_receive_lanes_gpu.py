"""The receive-side `_dev` entries behind the lanes (include/dabgpu.h, "batches in flight"; DevCall in
odr-dabmod_amd/csrc/dabgpu_ctx.h): with stream == NULL every one of the thirteen runs on the context's own stream, behind
everything queued on any lane before it (own_stream_joins_lanes), and the chain calls queued after it start behind it
(own_epoch / lane_joins_own_stream).  Nothing else in the suite leaves a chain output in flight on lane 1 or 2 when a receive
stage reads it, or hands a buffer that queued receive work still reads to the next chain call: the Python wrappers wait after
every NULL-stream call unless they are told queued=True, which is what these tests do.

The bar is the strictest there is, as in tests/test_lanes_gpu.py: the same BYTES as a one-lane context that is synchronised
after every step -- the serial path is the one the stage tests hold against their models.  One exception, stated by the header:
the receiver's two float64 sums are added with atomics in no fixed order, so sum_signal and sum_quadrature of monitor_stats are
compared to 1e-13 (a frame's sum has one addend per run of symbols, at most 75 of them, all positive: reordering moves it by
at most 74 x 2^-53 = 8.2e-15 of its value); its integer figures and min_margin are compared exactly.

profiles/receive_lane_stress_mutations.txt records what these tests do to two builds with one event wait removed each, and
the sizes below come from that protocol."""
import os

import numpy as np
import pytest

from tests import decode_model as M
from tests import receive_lanes_ops as G
from tests.conftest import load_pkg
from tests.golden.synth import synth_eti

pytestmark = pytest.mark.gpu

_STRESS_OPS = int(os.environ.get("DABGPU_STRESS_OPS", str(G.DEFAULT_OPS)))          # (a one-off hunt: DABGPU_STRESS_OPS=3000)
# frames per call of the directed tests, and transmission frames per generated frame of the stress (the mutation protocol's
# size ladder sets the two variables; the defaults are the sizes it settled on)
_DIRECTED_FRAMES = int(os.environ.get("DABGPU_RECEIVE_DIRECTED_FRAMES", str(G.DIRECTED_FRAMES)))
_UNIT = int(os.environ.get("DABGPU_RECEIVE_STRESS_UNIT", str(G.STRESS_UNIT)))
STAGES = G.GAIN | G.FIR
EARLY = 44                                   # tests/demod_cases.py: 45 - 1 behind FIRFilter, no window overlap
PATHS = [(0, 1.0 + 0.0j, 0.0), (37, 0.3 - 0.2j, 5.0)]


@pytest.fixture(scope="module")
def pkg():
    return load_pkg()


def _bytes(t):
    import torch
    return (torch.view_as_real(t) if t.is_complex() else t).contiguous().view(torch.uint8)


def _same(a, b):
    return a.dtype == b.dtype and a.numel() == b.numel() and bool((_bytes(a) == _bytes(b)).all())


def _spectrum_blob(md):
    st = md.spectrum_stats()
    return st["raw"].tobytes() + np.int64(st["segments"]).tobytes()


def _xspectrum_blob(md):
    r = md.dpd_xspectrum_result()
    return r["S"].tobytes() + r["p_tx"].tobytes() + r["p_rx"].tobytes() + np.int64(r["segments"]).tobytes()


def _dpd_blob(md):
    st = md.dpd_stats()
    return st["raw"].tobytes() + np.array([st["overflow"], st["samples_used"], st["n_bins"]], np.int64).tobytes()


def _alignment_blob(al):
    g = complex(al["gain"])
    return np.array([al["lag"], al["tau"], g.real, g.imag, al["coherence"]], np.float64).tobytes()


# ------------------------------------------------------------------------------------------------ a. one entry at a time
@pytest.fixture(scope="module")
def stream(pkg):
    """Five calls' worth of one ETI stream from FP = 0 (the suite's synthetic multiplex) and its coded bits, on the device;
    the first call's worth is the capture of every directed test.  Computed once, left unchanged."""
    import torch
    B = _DIRECTED_FRAMES
    assert B >= 16, "the decoder returns its first frame behind fifteen"
    eti = synth_eti(5 * B, mid=G.MODE)
    md = pkg.Modulator(mode=G.MODE, max_frames=5 * B)
    try:
        assert {k: md.geometry[k] for k in G.GEOM} == G.GEOM
        md.frontend_configure(eti[0])
        bits = md.eti_to_bits(eti)
    finally:
        md.close()
    assert bits.shape == (5 * B, G.GEOM["tf_input_bytes"])
    return dict(B=B, eti=eti, d_bits=torch.from_numpy(bits.reshape(5, B, -1).copy()).cuda(),
                keep=M.payload_mask(pkg.Modulator.frontend_describe(eti[0])))


def _directed(pkg, stream, entry, lanes):
    """A rehearsal first, every step waited for: the entry and what it needs in front of it once on a finished chain output,
    so that what a stage does on first use (device buffers, tables: calls that hold the host up) is behind it, then every
    stream state back at its start.  Then three chain calls (the third, on lane 2, writes the capture); the same steps with
    queued=True; a chain call on lane 0 and one on lane 1 that overwrites the capture; synchronize.  With one lane: the same,
    every step waited for.  -> (the entry's output as a tensor of bytes or its result blob, lanes the three calls went over, the
    capture's bytes)"""
    import torch
    B, tf, per = stream["B"], G.GEOM["tf_samples"], G.GEOM["tf_input_bytes"]
    d_bits = stream["d_bits"]
    md = pkg.Modulator(mode=G.MODE, max_frames=B)
    try:
        md.set_lanes(lanes)
        md.set_gain(2, 1.0, 0.5, 4.0)
        md.set_tii(True, 3, 5)
        md.frontend_configure(stream["eti"][0])
        md.set_channel(PATHS, 30.0, 77)
        cf = lambda n: torch.zeros(n, dtype=torch.complex64, device="cuda")        # noqa: E731
        cap, spare0, spare1, rx, frames = (cf(B * tf) for _ in range(5))
        bits = torch.zeros(B * per, dtype=torch.uint8, device="cuda")
        soft = torch.zeros(8 * B * per, dtype=torch.int8, device="cuda")
        img = torch.zeros(B * 6144, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()         # (torch's fills are done before the first call: the lanes are not ordered against torch's stream)
        result = {}

        def queue(src, step):
            """the entry on `src`, behind what it needs; -> its output tensor, or the getter of its result blob"""
            if entry == "channel":
                md.channel_dev(src, rx, queued=True)
                return rx
            if entry in ("sync", "sync_extract"):
                md.sync_dev(src, queued=True)
                if entry == "sync":
                    return md.sync_result_bytes
                step()
                md.sync_extract_dev(src, frames, queued=True)
                return frames
            if entry == "demod":
                md.demod_dev(src, B, EARLY, bits, d_bits[0], queued=True)
                return bits
            if entry in ("demod_soft", "decode_soft"):
                md.demod_soft_dev(src, B, soft, EARLY, queued=True)
                if entry == "demod_soft":
                    return soft
                step()
                md.decode_soft_dev(soft, B, img, queued=True)
                return img
            if entry == "decode":
                md.demod_dev(src, B, EARLY, bits, queued=True)
                step()
                md.decode_dev(bits, B, img, queued=True)
                return img
            if entry == "tii_scan":
                md.tii_scan_dev(src, B, EARLY, queued=True)
                return md.tii_scan_result_bytes
            if entry == "cir":
                md.cir_dev(src, B, EARLY, queued=True)
                return md.cir_result_bytes
            if entry == "spectrum":
                md.spectrum_dev(src, 2, True, queued=True)
                return lambda: _spectrum_blob(md)
            md.channel_dev(src, rx, queued=True)
            step()
            if entry == "dpd_xspectrum":
                md.dpd_xspectrum_dev(src, rx, 3, queued=True)
                return lambda: _xspectrum_blob(md)
            if entry == "dpd_align":             # (host data: the call itself waits for its own work)
                result["blob"] = _alignment_blob(md.dpd_align_dev(src, rx, queued=True))
                return lambda: result["blob"]
            assert entry == "dpd_measure"
            md.dpd_measure_dev(src, rx, None, G.DPD_PEAK, G.DPD_BINS, True, queued=True)
            return lambda: _dpd_blob(md)

        md.chain_dev_queued(d_bits[1], B, STAGES, spare0)
        md.synchronize()
        queue(spare0, md.synchronize)
        md.synchronize()
        md.decode_reset()
        md.channel_reset(0)
        md.reset_spectrum()              # (not the DPD sums: forgetting their peak would hold the host up again)
        for t in (rx, frames, bits, soft, img):
            t.zero_()
        torch.cuda.synchronize()
        md.set_lanes(lanes)              # (waits, and the rotation starts over: the next call goes to lane 0)

        step = md.synchronize if lanes == 1 else (lambda: None)
        for src, dst in ((1, spare0), (2, spare1), (0, cap)):
            md.chain_dev_queued(d_bits[src], B, STAGES, dst)
            step()
        created = md.lanes_info()[0]
        out = queue(cap, step)
        step()
        md.chain_dev_queued(d_bits[3], B, STAGES, spare0)                            # lane 0
        step()
        md.chain_dev_queued(d_bits[4], B, STAGES, cap)                               # lane 1: overwrites the capture
        md.synchronize()
        return (out() if callable(out) else _bytes(out).clone()), created, _bytes(cap).clone()
    finally:
        md.close()


@pytest.mark.parametrize("entry", G.ENTRIES)
def test_a_queued_entry_between_the_chain_call_it_reads_and_the_one_that_overwrites(pkg, stream, entry):
    """Per entry: the capture is still being written on lane 2 when the entry is queued, and the next call on lane 1 overwrites
    it while the entry may still read it -- nothing is waited for in between.  The entry's output (or result blob) is the
    serial context's, byte for byte, and not the zeros it was allocated as; the capture ends as the overwriting call's output."""
    import torch
    want, one, cap1 = _directed(pkg, stream, entry, 1)
    got, three, cap3 = _directed(pkg, stream, entry, 3)
    assert (one, three) == (1, 3), entry           # the calls rotated: the third, the capture's, went to lane 2
    if isinstance(want, bytes):
        assert len(got) == len(want) > 0 and any(want), entry
        assert got == want, "%s: the queued entry's result differs from the serial context's" % entry
    else:
        assert got.numel() == want.numel() > 0 and bool(want.any()), entry
        assert torch.equal(got, want), "%s: the queued entry's result differs from the serial context's" % entry
    assert torch.equal(cap3, cap1), "%s: the capture does not end as the overwriting call's output" % entry
    B = stream["B"]
    if entry == "demod":
        assert torch.equal(got, stream["d_bits"][0].reshape(-1))
    if entry == "decode":
        # the model, once: the payload behind the fifteen-frame lead-in is the ETI stream's (as tests/test_decode_gpu.py)
        images = got.cpu().numpy().reshape(B, 6144)
        keep = stream["keep"]
        assert np.array_equal(images[15:][:, keep], stream["eti"][:B - 15][:, keep])
        assert not images[:15].any() and not images[:, ~keep].any()


# ------------------------------------------------------------------------------------------------ b. the differential stress
def _iq_view(ring_buffer, frames, fmt):
    """the first `frames` frames of an IQ ring buffer (float32 storage) as the complex64 or int16 tensor a call writes"""
    import torch
    tf = G.GEOM["tf_samples"]
    if fmt == "cf":
        return torch.view_as_complex(ring_buffer[:2 * frames * tf].view(-1, 2))
    return ring_buffer[:frames * tf].view(torch.int16)


def _run_plan(pkg, plan, host, lanes, unit):
    """the sequence on a context with `lanes` lanes, every call on the context's own stream and queued; with one lane every
    operation is waited for.  -> dict(tensors, ring, fetched, final)"""
    import torch
    tf, per = G.GEOM["tf_samples"], G.GEOM["tf_input_bytes"]
    md = pkg.Modulator(mode=G.MODE, max_frames=G.MAX_FRAMES * unit)
    try:
        md.set_lanes(lanes)
        md.set_gain(2, 1.0, 0.5, 4.0)
        md.frontend_configure(host["eti"][0])
        md.set_channel(PATHS, 30.0, 77)
        # every buffer first, and torch's fills and copies DONE before the first call (tests/test_lanes_gpu.py explains)
        pool = torch.from_numpy(host["bits"]).cuda()
        d_eti = torch.from_numpy(host["eti"]).cuda()
        d_cod = torch.zeros((G.MAX_FRAMES * unit, per), dtype=torch.uint8, device="cuda")
        ring = [torch.zeros(2 * G.MAX_FRAMES * unit * tf, dtype=torch.float32, device="cuda") for _ in range(G.RING)]
        tens = [torch.zeros(n * unit, dtype=getattr(torch, dt), device="cuda") for dt, n in plan.tensors]
        nmax = G.MAX_FRAMES * unit
        prime = torch.zeros(8 * nmax * per, dtype=torch.int8, device="cuda")
        scratch = torch.zeros(nmax * 6144, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()

        def prime_decoders():
            """both decoders past their fifteen-frame lead-in, so that what they return afterwards is payload"""
            for _ in range(G.DECODER_PRIME):
                md.decode_dev(prime.view(torch.uint8)[:nmax * per], nmax, scratch, queued=True)
                md.decode_soft_dev(prime, nmax, scratch, queued=True)

        prime_decoders()
        md.synchronize()

        def buf(handle, meta=None):
            if handle[0] == "iq":
                return _iq_view(ring[handle[1]], meta["frames"] * unit, meta["fmt"])
            return tens[handle[1]]

        fetched, cur_fmt = [], "cf"
        for i, op in enumerate(plan.ops):
            k = op["kind"]
            if k == "drop":
                continue
            if k == "call":
                n = op["frames"] * unit
                if op["fmt"] != cur_fmt:
                    cur_fmt = op["fmt"]
                    md.set_output_format(None if cur_fmt == "cf" else "s16")
                out = _iq_view(ring[op["ring"]], n, cur_fmt)
                at = op["at"] * unit
                if op["eti"]:
                    md.chain_eti_dev_queued(d_eti[at:at + n], n, op["stages"], d_cod[:n], out)
                else:
                    md.chain_dev_queued(pool[at:at + n], n, op["stages"], out)
            elif k == "set":
                w = op["what"]
                if w == "set_channel":
                    md.set_channel(op["paths"], op["sigma"], op["seed"])
                elif w == "channel_reset":
                    md.channel_reset(op["position"])
                elif w == "decode_reset":
                    md.decode_reset()
                    prime_decoders()
                else:
                    md.set_tii(op["on"], op["comb"], op["pattern"], False)
            elif k == "fetch":
                w = op["what"]
                if w == "sync":
                    v = md.sync_result_bytes()
                elif w == "tii_scan":
                    v = md.tii_scan_result_bytes()
                elif w == "cir":
                    v = md.cir_result_bytes()
                elif w == "monitor":
                    v = md.monitor_stats(op["frame"])
                elif w == "spectrum":
                    v = _spectrum_blob(md)
                elif w == "dpd_xspectrum":
                    v = _xspectrum_blob(md)
                elif w == "dpd_stats":
                    v = _dpd_blob(md)
                elif w == "decode_stats":
                    v = md.decode_stats(op["frame"])
                else:
                    assert w == "decode_soft_stats"
                    v = md.decode_soft_stats(op["frame"])
                fetched.append((i, w, v))
            else:
                e = op["entry"]
                out = buf(op["out"]) if op["out"] is not None else None
                if e.startswith("dpd_"):
                    tx, rx = buf(op["tx"]["buf"], op["tx"]), buf(op["rx"])
                    if e == "dpd_xspectrum":
                        md.dpd_xspectrum_dev(tx, rx, op["rx_offset"], queued=True)
                    elif e == "dpd_align":
                        try:                 # (host data, the call waits for its own work; a refused alignment is a result too)
                            v = _alignment_blob(md.dpd_align_dev(tx, rx, queued=True))
                        except pkg.DabGpuError as err:
                            v = str(err)
                        fetched.append((i, e, v))
                    else:
                        md.dpd_measure_dev(tx, rx, op["alignment"], G.DPD_PEAK, G.DPD_BINS, True, queued=True)
                else:
                    src, n = buf(op["src"]["buf"], op["src"]), op["src"]["frames"] * unit
                    if e == "channel":
                        md.channel_dev(src, out, queued=True)
                    elif e == "sync":
                        md.sync_dev(src, op["max_shift"], queued=True)
                    elif e == "sync_extract":
                        md.sync_extract_dev(src, out, queued=True)
                    elif e == "demod":
                        md.demod_dev(src, n, op["early"], out, queued=True)
                    elif e == "demod_soft":
                        md.demod_soft_dev(src, n, out, op["early"], buf(op["bits"]) if op["bits"] is not None else None, queued=True)
                    elif e in ("decode", "decode_soft"):
                        (md.decode_dev if e == "decode" else md.decode_soft_dev)(src, n, out, queued=True)
                    elif e == "tii_scan":
                        md.tii_scan_dev(src, n, op["early"], queued=True)
                    elif e == "cir":
                        md.cir_dev(src, n, op["early"], op["window"], queued=True)
                    else:
                        assert e == "spectrum"
                        md.spectrum_dev(src, 2, True, queued=True)
            if lanes == 1:
                md.synchronize()
        md.synchronize()
        final = dict(spectrum=_spectrum_blob(md), dpd=_dpd_blob(md), position=md.channel_position())
        for name, get in (("decode", md.decode_stats), ("decode_soft", md.decode_soft_stats)):
            last = [op for op in plan.ops if op["kind"] == "receive" and op["entry"] == name]
            final[name] = [get(f) for f in range(last[-1]["src"]["frames"] * unit)] if last else []
        return dict(tensors=tens, ring=ring, fetched=fetched, final=final)
    finally:
        md.close()


def _same_fetch(what, a, b):
    if what != "monitor":
        return a == b
    exact = ("bit_errors", "n_bits", "min_margin")
    return all(a[k] == b[k] for k in exact) and all(abs(a[k] - b[k]) <= 1e-13 * abs(b[k]) for k in ("sum_signal", "sum_quadrature"))


@pytest.fixture(scope="module")
def stress_host():
    """the pools the sequences draw from: coded bits (seeded bytes) and one ETI stream from FP = 0; left unchanged"""
    rs = np.random.RandomState(4242)
    per = G.GEOM["tf_input_bytes"]
    bits = np.frombuffer(rs.bytes(G.POOL_FRAMES * _UNIT * per), np.uint8).reshape(G.POOL_FRAMES * _UNIT, per).copy()
    return dict(bits=bits, eti=synth_eti(G.ETI_POOL * _UNIT, mid=G.MODE))


@pytest.mark.parametrize("seed", G.SEEDS)
def test_random_receive_sequences_on_three_lanes_equal_the_serial_context(pkg, stress_host, seed):
    """ONE generated sequence (tests/receive_lanes_ops.py: chain calls into a ring of four IQ buffers, the thirteen receive
    entries on whatever was written last, settings, result getters) runs twice: on three lanes with every call queued and only
    the getters waiting, and on one lane with a wait after every operation.  The same bytes in every tensor a receive
    operation wrote and in the ring, the same fetched results call by call, the same accumulated spectrum and DPD sums, channel
    position and decoder statistics at the end -- and the work was real."""
    plan = G.generate(seed, _STRESS_OPS)
    res = {lanes: _run_plan(pkg, plan, stress_host, lanes, _UNIT) for lanes in (3, 1)}
    a, b = res[3], res[1]
    assert len(a["tensors"]) == len(b["tensors"]) == len(plan.tensors) > 0
    writer = {}
    for i, op in enumerate(plan.ops):
        if op["kind"] == "receive":
            for h in (op["out"], op.get("bits")):
                if h is not None:
                    writer[h[1]] = (i, op["entry"])
    bad = [(j,) + writer[j] for j, (x, y) in enumerate(zip(a["tensors"], b["tensors"])) if not _same(x, y)]
    assert not bad, "tensors (index, operation, entry) that differ from the serial run: %s" % bad[:8]
    assert all(_same(x, y) for x, y in zip(a["ring"], b["ring"]))
    assert len(a["fetched"]) == len(b["fetched"])
    bad = [(i, w) for (i, w, x), (_, _, y) in zip(a["fetched"], b["fetched"]) if not _same_fetch(w, x, y)]
    assert not bad, "fetched results (operation, getter) that differ from the serial run: %s" % bad[:8]
    assert a["final"] == b["final"]
    # ... and the work was real: all outputs but at most one differ from the zeros they were allocated as
    assert sum(int(bool(_bytes(t).any())) for t in a["tensors"]) >= len(a["tensors"]) - 1
    assert any(a["final"]["spectrum"]) and any(a["final"]["dpd"])
