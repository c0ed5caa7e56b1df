"""The front-end's stream state (include/dabgpu.h, "front-end stream state"): the time interleaver's history read into a blob,
installed from one, and computed from the ETI frames in front of a position of the stream -- by itself and together with the
chain's seed -- so that an ETI-fed stream is handed over, continued by another process, or split over contexts.

Every comparison is BYTE equality: coded bits against the CPU front-end of this repository (odr-dabmod_amd.frontend.Frontend),
IQ against ONE context's uninterrupted chain_eti over the whole stream.  The streams are tests/golden/synth.synth_eti with a
running frame phase: 40 Mode I frames (10 transmission frames) of the five-sub-channel layout, 18 Mode III frames."""
import importlib
import os
import subprocess

import numpy as np
import pytest

from tests.conftest import ROOT
from tests.golden.frontend_cases import ETI_CASES
from tests.golden.synth import POLY_AM, POLY_PM, synth_eti

pytestmark = pytest.mark.gpu

HOST = os.path.join(ROOT, "odr-dabmod_amd", "host")
CIFS = {1: 4, 3: 1}
G, F, R, P = 1, 2, 4, 8
MULTI = ETI_CASES["multi"]["kw"]["subchannels"]
OTHER = ((400, 48, 0x22), (0, 24, 1), (200, 3, 0x23))            # another multiplex layout
# the three set-ups of the chain seed: cfg 4 (gain var + default FIR + resampler x4 + MemlessPoly, s16) with TII, cfg 3 (no
# resampler), Mode III cfg 3
SETUPS = {"cfg4_tii_s16": (1, 4), "cfg3": (1, 3), "mode3_cfg3": (3, 3)}


def same_bytes(a, b):
    a = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    b = np.ascontiguousarray(b).view(np.uint8).reshape(-1)
    return a.size == b.size and a.size > 0 and np.array_equal(a, b)


@pytest.fixture(scope="module")
def streams():
    """mode -> (ETI frames, the CPU front-end's coded bits), computed once and never written to"""
    fe = importlib.import_module("odr-dabmod_amd.frontend").Frontend()
    out = {}
    for mode, eti in ((1, synth_eti(40, subchannels=MULTI, mid=1, seed=2024)),
                      (3, synth_eti(18, subchannels=ETI_CASES["mode3"]["kw"]["subchannels"], mid=3, seed=2025))):
        bits = fe.eti_to_bits(eti, mode)
        assert bits.shape[0] == eti.shape[0] // CIFS[mode]
        eti.setflags(write=False)
        bits.setflags(write=False)
        out[mode] = (eti, bits)
    return out


def chain_context(pkg, setup, max_frames=8):
    mode, cfg = SETUPS[setup]
    md = pkg.Modulator(mode=mode, max_frames=max_frames)
    try:
        fmt = "s16" if cfg == 4 else None
        md.set_gain(2, 1.0, (32767.0 if fmt else 1.0) / 50000.0, 4.0)
        if fmt:
            md.set_output_format(fmt)
        md.set_fir_taps(None)
        if cfg == 4:
            md.set_resampler(2048000, 8192000)
            md.set_poly(POLY_AM, POLY_PM)
            md.set_tii(True, 3, 5)
    except Exception:
        md.close()
        raise
    return md, {3: G | F, 4: G | F | R | P}[cfg]


def in_calls(md, fn, eti, max_frames, *args):
    """a run of whole transmission frames through fn in calls of at most max_frames"""
    step = max_frames * CIFS[md.geometry["mode"]]
    parts = [fn(eti[at:at + step], *args).copy() for at in range(0, eti.shape[0], step)]
    return np.concatenate(parts) if parts else np.empty((0, 0), np.uint8)


def front_end_context(pkg, eti0, mode=1, max_frames=8):
    md = pkg.Modulator(mode=mode, max_frames=max_frames)
    try:
        md.frontend_configure(eti0)
    except Exception:
        md.close()
        raise
    return md


@pytest.fixture(scope="module")
def whole(pkg, streams):
    """set-up -> one context's uninterrupted chain_eti over the whole stream (computed on first use, shared, left unchanged)"""
    cache = {}

    def get(setup):
        if setup not in cache:
            eti = streams[SETUPS[setup][0]][0]
            md, stages = chain_context(pkg, setup)
            try:
                md.frontend_configure(eti[0])
                y = in_calls(md, md.chain_eti, eti, 8, stages)
            finally:
                md.close()
            y.setflags(write=False)
            cache[setup] = y
        return cache[setup]
    return get


# --------------------------------------------------------------------------- 1. hand-over through the blob
@pytest.mark.parametrize("k", [2, 5])
def test_a_stream_handed_over_through_the_blob_continues_with_the_cpu_bits(pkg, streams, k):
    """A does transmission frames 0 ... k - 1, its blob goes to a fresh configured B: k = 2, eight frames of history and seven
    zero rows in front; k = 5, the history full."""
    eti, want = streams[1]
    a, b = front_end_context(pkg, eti[0]), front_end_context(pkg, eti[0])
    try:
        assert same_bytes(a.eti_to_bits(eti[:4 * k]), want[:k])
        blob = a.frontend_state()
        assert len(blob) == 540 + 15 * 6912 and blob[:4] == b"DGFS"
        rows = np.frombuffer(blob, np.uint8)[540:].reshape(15, 6912)
        assert bool(rows[:max(0, 15 - 4 * k)].any()) is False and all(r.any() for r in rows[max(0, 15 - 4 * k):])
        # without the blob B starts a stream: other bytes
        assert not same_bytes(b.eti_to_bits(eti[4 * k:4 * k + 4]), want[k:k + 1])
        b.set_frontend_state(blob)
        assert b.frontend_state() == blob
        assert same_bytes(b.eti_to_bits(eti[4 * k:]), want[k:])
        assert same_bytes(a.eti_to_bits(eti[4 * k:]), want[k:])             # (reading the state does not move it)
        assert a.frontend_state() == b.frontend_state()
    finally:
        a.close()
        b.close()


# --------------------------------------------------------------------------- 2. the front-end seed
@pytest.mark.parametrize("max_frames", [8, 1])
@pytest.mark.parametrize("e", [0, 8, 20])
def test_front_end_seed_gives_the_state_and_the_bits_of_the_uninterrupted_stream(pkg, streams, e, max_frames):
    """B is seeded from the min(e, 15) frames in front of e: its blob equals, byte for byte, the blob of a context that ran
    frames 0 ... e - 1, and the rest of the stream gives the CPU bits.  Also with one transmission frame of capacity: the seed
    needs no more rows than a call of one frame does."""
    eti, want = streams[1]
    a, b = front_end_context(pkg, eti[0]), front_end_context(pkg, eti[0], max_frames=max_frames)
    try:
        if e:
            a.eti_to_bits(eti[:e])
        b.eti_to_bits(eti[36:40])                    # B comes from somewhere else in the stream: the seed overwrites all of it
        b.frontend_seed(eti[max(0, e - 15):e], e)
        assert b.frontend_state() == a.frontend_state()
        assert same_bytes(in_calls(b, b.eti_to_bits, eti[e:], max_frames), want[e // 4:])
        a.eti_to_bits(eti[e:e + 8])
        b.frontend_seed(eti[max(0, e + 8 - 15):e + 8], e + 8)                # (a second seed on the same context)
        assert b.frontend_state() == a.frontend_state()
    finally:
        a.close()
        b.close()


# --------------------------------------------------------------------------- 3. the chain seed from ETI frames
def _seeded_run(pkg, streams, whole, setup, e, max_frames=8, device_form=False):
    mode = SETUPS[setup][0]
    eti, cifs = streams[mode][0], CIFS[mode]
    want = whole(setup)
    st = importlib.import_module("odr-dabmod_amd.streams")
    start, stop = st.eti_leadin(e, cifs)
    assert stop - start == min(e, 15 + cifs)
    b, stages = chain_context(pkg, setup, max_frames)
    try:
        b.frontend_configure(eti[0])
        if device_form:
            import torch
            d_eti = torch.from_numpy(eti[start:stop].copy()).to("cuda:0")
            b.seed_eti_dev(d_eti if stop > start else None, stop - start, stages, e)
        else:
            b.seed_eti(eti[start:stop], stages, e)
        got = in_calls(b, b.chain_eti, eti[e:], max_frames, stages)
        assert got.shape == want[e // cifs:].shape and same_bytes(got, want[e // cifs:])
    finally:
        b.close()


# k odd and even (both TII parities); e = 4 k reaches a full history at k = 4; in Mode III (one ETI frame per transmission
# frame) the sixteen-frame lead-in is reached at k = 16, 17
@pytest.mark.parametrize("setup,k", [(s, k) for s in ("cfg4_tii_s16", "cfg3") for k in (1, 3, 4, 6)] +
                         [("mode3_cfg3", k) for k in (1, 3, 4, 6, 16, 17)])
def test_chain_seeded_from_eti_continues_the_uninterrupted_stream(pkg, streams, whole, setup, k):
    _seeded_run(pkg, streams, whole, setup, k * CIFS[SETUPS[setup][0]])


def test_chain_seeded_from_eti_with_room_for_one_transmission_frame(pkg, streams, whole):
    _seeded_run(pkg, streams, whole, "cfg4_tii_s16", 24, max_frames=1)


@pytest.mark.parametrize("k", [0, 5])
def test_chain_seed_from_eti_in_device_memory(pkg, streams, whole, k):
    """the _dev form on torch's stream (k = 0: the start of a stream, no lead-in at all)"""
    _seeded_run(pkg, streams, whole, "cfg4_tii_s16", 4 * k, device_form=True)


# --------------------------------------------------------------------------- 4. one ETI stream over several contexts
@pytest.fixture(scope="module")
def three_contexts(pkg, streams):
    mods = []
    try:
        for _ in range(3):
            md, stages = chain_context(pkg, "cfg4_tii_s16")
            mods.append(md)
            md.frontend_configure(streams[1][0][0])
        yield mods, stages
    finally:
        for md in mods:
            md.close()


@pytest.mark.parametrize("chunk", [1, 2, 3])
@pytest.mark.parametrize("n", [2, 3])
def test_partitioned_stream_modulate_eti_equals_one_context(pkg, streams, whole, three_contexts, n, chunk):
    st = importlib.import_module("odr-dabmod_amd.streams")
    mods, stages = three_contexts
    got = st.PartitionedStream(mods[:n]).modulate_eti(streams[1][0].copy(), stages, chunk)
    want = whole("cfg4_tii_s16")
    assert got.shape == want.shape and same_bytes(got, want)


# --------------------------------------------------------------------------- 5. a seed is not a chain call
def test_a_seed_leaves_the_last_calls_diagnostics_alone(pkg, streams, whole):
    eti, want = streams[1][0], whole("cfg4_tii_s16")
    md, stages = chain_context(pkg, "cfg4_tii_s16")
    try:
        md.set_gain(2, 1.0, 4.0 * 32767.0 / 50000.0, 4.0)                   # (loud enough for the s16 conversion to clip)
        md.trace(True)
        md.frontend_configure(eti[0])
        md.chain_eti(eti[:8], stages)
        variant, clipped = md.last_variant(), md.num_clipped()
        assert variant and any("tf_kernel" in v for v in variant) and clipped > 0
        md.seed_eti(eti[1:20], stages, 20)
        assert md.last_variant() == variant and md.num_clipped() == clipped
        md.set_gain(2, 1.0, 32767.0 / 50000.0, 4.0)
        md.seed_eti(eti[1:20], stages, 20)                                   # (under the settings the frames run under)
        assert same_bytes(md.chain_eti(eti[20:], stages), want[5:])
    finally:
        md.close()


# --------------------------------------------------------------------------- 6. refusals
def test_refusals_leave_the_stream_where_it_was(pkg, streams, whole):
    """Each refusal is followed by the next transmission frame of the uninterrupted stream: neither the history nor the halo
    nor the TII parity has moved."""
    eti, want = streams[1][0], whole("cfg4_tii_s16")
    md, stages = chain_context(pkg, "cfg4_tii_s16")
    other = pkg.Modulator(mode=1, max_frames=1)
    third = pkg.Modulator(mode=3, max_frames=1)
    fresh, _ = chain_context(pkg, "cfg4_tii_s16")
    at = [0]

    def carries_on(n=1):
        k = at[0]
        got = md.chain_eti(eti[4 * k:4 * (k + n)], stages)
        assert same_bytes(got, want[k:k + n]), k
        at[0] += n
    try:
        md.frontend_configure(eti[0])
        carries_on(2)
        other.frontend_configure(synth_eti(1, subchannels=OTHER, mid=1)[0])
        with pytest.raises(pkg.DabGpuError, match="another multiplex layout"):
            md.set_frontend_state(other.frontend_state())
        carries_on()
        third.frontend_configure(streams[3][0][0])
        with pytest.raises(pkg.DabGpuError, match="another transmission mode"):
            md.set_frontend_state(third.frontend_state())
        carries_on()
        blob = md.frontend_state()
        for bad, word in ((blob[:-1], "size"), (blob + b"\0", "size"), (b"XXXX" + blob[4:], "magic"),
                          (blob[:4] + b"\2\0\0\0" + blob[8:], "version"), (blob[:16], "shorter than its header")):
            with pytest.raises(pkg.DabGpuError, match=word):
                md.set_frontend_state(bad)
        assert md.frontend_state() == blob
        carries_on()
        blob = md.frontend_state()
        e = 4 * at[0]                                                         # 20: the lead-in is frames 1 ... 19
        for lead, pos in ((eti[2:20], e), (eti[0:20], e), (eti[5:20], e), (eti[2:20], e - 1)):
            with pytest.raises(pkg.DabGpuError, match="frontend seed"):
                md.seed_eti(lead, stages, pos)
        with pytest.raises(pkg.DabGpuError, match="frontend seed"):
            md.frontend_seed(eti[4:20], e)                                   # sixteen frames where fifteen are asked for
        assert md.frontend_state() == blob
        carries_on()
        e = 4 * at[0]                                                         # 24
        changed = eti[e - 19:e].copy()
        changed[5, 9] ^= 1                                                   # SAD of the first sub-channel, in one lead-in frame
        with pytest.raises(pkg.DabGpuError, match="FrameMultiplexer detected a multiplex reconfiguration"):
            md.seed_eti(changed, stages, e)
        with pytest.raises(pkg.DabGpuError, match="FrameMultiplexer detected a multiplex reconfiguration"):
            md.frontend_seed(changed[4:], e)
        with pytest.raises(pkg.DabGpuError, match="closes a transmission frame"):
            md.seed_eti(eti[e - 20:e - 1], stages, e)                        # the right count, one frame early: FP = 6
        carries_on()
        # an unconfigured context: neither blob nor seed; then it is configured and starts its stream
        for call in (lambda: fresh.seed_eti(None, stages, 0), lambda: fresh.frontend_seed(None, 0), fresh.frontend_state,
                     lambda: fresh.set_frontend_state(blob)):
            with pytest.raises(pkg.DabGpuError, match="not configured"):
                call()
        fresh.frontend_configure(eti[0])
        assert same_bytes(fresh.chain_eti(eti[:4], stages), want[:1])
        # the chain's own seed keeps refusing a context with a front-end, in the words it had
        with pytest.raises(pkg.DabGpuError, match="front-end state"):
            md.seed(None, stages, 0)
        carries_on(3)
        assert at[0] == 10
    finally:
        for m in (md, other, third, fresh):
            m.close()


# --------------------------------------------------------------------------- 7. dabmod_file --state-out / --state-in
def test_dabmod_file_continues_a_stream_from_a_state_file(tmp_path):
    """cfg 4 as s16, four transmission frames per call: the file of one run over 40 frames equals the file of a run over the
    first 20 (--state-out) followed by the file of a run over the last 20 (--state-in), which starts at FP = 4."""
    import oracle as O
    eti = synth_eti(40, subchannels=MULTI, mid=1, seed=77)
    names = {n: str(tmp_path / n) for n in ("all.eti", "head.eti", "tail.eti", "all.iq", "head.iq", "tail.iq", "state", "poly.coef")}
    eti.tofile(names["all.eti"])
    eti[:20].tofile(names["head.eti"])
    eti[20:].tofile(names["tail.eti"])
    O.write_poly_file(names["poly.coef"], POLY_AM, POLY_PM)
    opts = ["--gpu-frontend", "--batch", "4", "--format", "s16", "--fir", "default", "--rate", "8192000", "--poly", names["poly.coef"],
            "--normalise", str(32767.0 / 50000.0), "--tii", "3,5"]

    def run(fin, fout, extra, counts):
        r = subprocess.run([os.path.join(HOST, "dabmod_file"), names[fin], names[fout]] + opts + extra, capture_output=True,
                           text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        assert r.stdout.split() == counts
        return np.fromfile(names[fout], np.uint8)
    one = run("all.eti", "all.iq", [], ["40", "10", "10"])
    head = run("head.eti", "head.iq", ["--state-out", names["state"]], ["20", "5", "5"])
    assert os.path.getsize(names["state"]) > 540 + 15 * 6912 + 40
    tail = run("tail.eti", "tail.iq", ["--state-in", names["state"]], ["20", "5", "5"])
    assert one.size == 10 * 4 * 196608 * 4 and same_bytes(np.concatenate([head, tail]), one)
    # without the state the tail is another file (and the gate skips to FP = 0: one transmission frame fewer)
    cold = run("tail.eti", "tail.iq", [], ["20", "4", "4"])
    assert not same_bytes(cold, tail[-cold.size:])
    # a tail that does not open a transmission frame is refused with the message
    eti[21:].tofile(names["tail.eti"])
    r = subprocess.run([os.path.join(HOST, "dabmod_file"), names["tail.eti"], names["tail.iq"]] + opts + ["--state-in", names["state"]],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "must open a transmission frame" in r.stderr and "FP = 5" in r.stderr
