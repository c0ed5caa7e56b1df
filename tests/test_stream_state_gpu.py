"""The stream state of a context -- the Resampler's halo and the TII frame parity -- read, installed and computed from a
lead-in frame (include/dabgpu.h, "stream state"): a stream that is moved to another context, or split over several, gives
the bytes of the stream that never moved.

Everything here is BYTE equality (outputs compared as raw bytes), not a tolerance: the state is input samples, hops and
symbols are independent work items, and no arithmetic changes with where a frame sits in a call.  The oracle-parity tests
pin the single-context bytes; these pin "moved or split equals unmoved"."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import oracle as O
from tests.conftest import ROOT
from tests.golden.synth import POLY_AM, POLY_PM, synth_eti

pytestmark = pytest.mark.gpu

HOST = os.path.join(ROOT, "odr-dabmod_amd", "host")
HEADER = 40
G, F, R, P = 1, 2, 4, 8
CHAIN = G | F | R | P


def coded_bits(mode, n, seed=20240):
    """n frames of random coded bits from a fixed seed."""
    return np.random.RandomState(seed + mode).randint(0, 256, (n, O.tf_input_bytes(mode))).astype(np.uint8)


def fir_taps(n):
    k = np.arange(n) - (n - 1) / 2.0
    h = 0.79 * np.sinc(0.79 * k) * np.hamming(n)
    return (h / h.sum()).astype(np.float32)


def context(pkg, mode=1, out_rate=8192000, fmt=None, tii=False, extra=None, max_frames=16):
    """Settings as in test_chain_rational_rate_with_poly (gain var at normalise 1 / 50000, the polynomial predistorter), at
    the rate, format and TII setting of the case; `extra` adds what the case varies."""
    md = pkg.Modulator(mode=mode, max_frames=max_frames)
    try:
        if fmt:
            md.set_gain(2, 1.0, (32767.0 if fmt == "s16" else 127.0) / 50000.0, 4.0)    # (integers worth comparing)
            md.set_output_format(fmt)
        else:
            md.set_gain(2, 1.0, 1.0 / 50000.0, 4.0)
        md.set_resampler(2048000, out_rate)
        md.set_poly(POLY_AM, POLY_PM)
        if tii:
            md.set_tii(True, 3, 5)
        if extra:
            extra(md)
    except Exception:
        md.close()
        raise
    return md


def raw(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


def same_bytes(a, b):
    a, b = raw(a), raw(b)
    return a.size == b.size and a.size > 0 and np.array_equal(a, b)


def parse(blob):
    h = np.frombuffer(blob[:HEADER], np.uint32)
    rates = np.frombuffer(blob[16:32], np.uint64)
    return dict(magic=int(h[0]), version=int(h[1]), mode=int(h[2]), insert=int(h[3]), rs_in=int(rates[0]), rs_out=int(rates[1]),
                nin=int(h[8]), reserved=int(h[9]), halo=np.frombuffer(blob[HEADER:], np.complex64))


# --------------------------------------------------------------------------- 1. hand-over
HANDOVER = [
    # mode, out_rate, format, stages, TII, K
    (1, 8192000, None, CHAIN, True, 1),        # x4: the kernel writes the halo itself into the double buffer
    (1, 8192000, None, CHAIN, True, 2),
    (1, 8192000, "s16", G | F | R, False, 2),  # the x4 kernel stores the integers
    (1, 4096000, None, CHAIN, False, 1),       # x2
    (2, 8192000, None, CHAIN, True, 3),
    (2, 2400000, None, CHAIN, True, 2),        # the rational kernel with the copy behind it
    (1, 2400000, None, CHAIN, False, 1),
    (3, 4096000, None, CHAIN, False, 2),
    (4, 1024000, None, CHAIN, False, 1),       # downsampling
]


@pytest.mark.parametrize("mode,out_rate,fmt,stages,tii,K", HANDOVER)
def test_handed_over_stream_equals_the_unmoved_stream(pkg, mode, out_rate, fmt, stages, tii, K):
    """Context A runs frames 0 ... K - 1 and gives its state; a fresh context B with the same settings installs it and runs
    frames K ...; context C runs the whole stream.  B's bytes are C's for the same frames."""
    n = K + 3
    bits = coded_bits(mode, n)
    a, b, c = (context(pkg, mode, out_rate, fmt, tii) for _ in range(3))
    try:
        a.chain(bits[:K], stages)
        blob = a.stream_state()
        st = parse(blob)
        assert st["mode"] == mode and st["rs_out"] == out_rate and st["nin"] == st["halo"].size == 2 * a.geometry["spacing"]
        assert st["insert"] == (1 if K % 2 == 0 else 0) and np.abs(st["halo"]).max() > 0
        b.set_stream_state(blob)
        yb = b.chain(bits[K:], stages)
        yc = c.chain(bits, stages)
        assert yb.shape == yc[K:].shape
        assert same_bytes(yb, yc[K:])
        # ... and B, having run them, is where C is
        assert b.stream_state() == c.stream_state()
    finally:
        for md in (a, b, c):
            md.close()


@pytest.mark.parametrize("out_rate", [8192000, 2400000])
def test_state_after_a_one_hop_resampler_call(pkg, out_rate):
    """The per-stage Resampler with ONE hop in a call (the halo shifts by a hop instead of being replaced): the blob is
    [the hop before | this hop], oldest first, and a context that installs it continues the stream."""
    hop = 2048
    rs = np.random.RandomState(7)
    x = (rs.randn(5 * hop) + 1j * rs.randn(5 * hop)).astype(np.complex64)
    a, b, c = (context(pkg, 1, out_rate) for _ in range(3))
    try:
        a.resample(x[:hop])
        st = parse(a.stream_state())
        assert same_bytes(st["halo"], np.concatenate([np.zeros(hop, np.complex64), x[:hop]]))
        a.resample(x[hop:2 * hop])
        blob = a.stream_state()
        assert same_bytes(parse(blob)["halo"], x[:2 * hop])
        b.set_stream_state(blob)
        yb = b.resample(x[2 * hop:])
        yc = c.resample(x)
        assert same_bytes(yb, yc[yc.size - yb.size:]) and yb.size * 5 == yc.size * 3
    finally:
        for md in (a, b, c):
            md.close()


def test_state_taken_while_two_submitted_batches_are_in_flight(pkg):
    """dabgpu_get_stream_state waits for the context: taken between submit and collect it describes the stream after both
    batches."""
    bits = coded_bits(1, 6)
    a, b, c = (context(pkg, 1, 8192000, tii=True) for _ in range(3))
    try:
        a.submit(bits[:2], CHAIN)
        a.submit(bits[2:4], CHAIN)
        blob = a.stream_state()
        ya = np.concatenate([a.collect().reshape(2, -1), a.collect().reshape(2, -1)])
        b.set_stream_state(blob)
        yb = b.chain(bits[4:], CHAIN)
        yc = c.chain(bits, CHAIN)
        assert same_bytes(ya, yc[:4]) and same_bytes(yb, yc[4:])
    finally:
        for md in (a, b, c):
            md.close()


# --------------------------------------------------------------------------- 2. seed
def _taps(n):
    return lambda md: md.set_fir_taps(fir_taps(n))


SEEDS = {
    # name: (mode, out_rate, stages, TII, K, extra settings)
    "no FIRFilter": (1, 8192000, G | R | P, False, 2, None),
    "default FIRFilter": (1, 8192000, CHAIN, False, 2, None),
    "101 taps": (1, 8192000, CHAIN, False, 1, _taps(101)),
    "300 taps, the unfused filter": (1, 8192000, CHAIN, False, 2, _taps(300)),
    "window 10": (1, 8192000, CHAIN, False, 2, lambda md: md.set_window_overlap(10)),
    "window 10 without FIRFilter": (3, 4096000, G | R | P, False, 2, lambda md: md.set_window_overlap(10)),
    "CFR": (1, 8192000, CHAIN, False, 2, lambda md: md.set_cfr(True, 50.0, 0.1)),
    "CFR + TII": (2, 8192000, CHAIN, True, 2, lambda md: md.set_cfr(True, 50.0, 0.1)),
    "gain rounding REFERENCE": (1, 8192000, CHAIN, False, 2, lambda md: md.set_gain_rounding(True)),
    "TII, mode 1, K odd": (1, 8192000, CHAIN, True, 1, None),
    "TII, mode 1, K even": (1, 8192000, CHAIN, True, 2, None),
    "TII, mode 2, K odd": (2, 8192000, CHAIN, True, 3, None),
    "TII, mode 2, K even": (2, 8192000, CHAIN, True, 2, None),
    "TII + max gain, added behind the frame kernel": (1, 8192000, CHAIN, True, 3, lambda md: md.set_gain(1, 1.0, 1.0 / 50000.0, 4.0)),
    "rational rate": (2, 2400000, CHAIN, True, 1, None),
    "downsampling, mode 4": (4, 1024000, CHAIN, False, 1, None),
    # the lead-in frame runs as complexf whatever the output format: the x4 kernel stores s16, a convert kernel u8
    "s16 output": (1, 8192000, G | F | R, True, 1, None, "s16"),
    "s16 output, rational rate": (2, 2400000, G | F | R, False, 2, None, "s16"),
    "u8 output": (1, 4096000, G | F | R, False, 2, None, "u8"),
}


@pytest.mark.parametrize("name", list(SEEDS))
def test_seeded_context_equals_the_unmoved_stream(pkg, name):
    """B is seeded with the coded bits of frame K - 1 and the index K, then runs frames K ...: the bytes of the stream that
    ran through frames 0 ... K - 1 first -- and B's state blob after the seed is that stream's blob after frame K - 1, byte
    for byte.  Over the variants of the native-rate part that differ."""
    mode, out_rate, stages, tii, K, extra = SEEDS[name][:6]
    fmt = SEEDS[name][6] if len(SEEDS[name]) > 6 else None
    bits = coded_bits(mode, K + 2)
    a, b = (context(pkg, mode, out_rate, fmt, tii, extra) for _ in range(2))
    try:
        a.chain(bits[:K], stages)
        blob = a.stream_state()
        ya = a.chain(bits[K:], stages)
        b.seed(bits[K - 1], stages, K)
        assert b.stream_state() == blob
        yb = b.chain(bits[K:], stages)
        assert same_bytes(yb, ya)
        # a used context seeded somewhere else in the same stream: frames 1 ... again
        b.seed(bits[0], stages, 1)
        if K == 1:
            assert same_bytes(b.chain(bits[1:], stages), ya)
        else:
            a.seed(None, stages, 0)
            y0 = a.chain(bits[:2], stages)
            assert same_bytes(b.chain(bits[1:2], stages), y0[1:2])
    finally:
        a.close()
        b.close()


def test_seed_with_index_zero_on_a_used_context_is_a_fresh_context(pkg):
    bits = coded_bits(1, 3)
    used, fresh = context(pkg, 1, 8192000, tii=True), context(pkg, 1, 8192000, tii=True)
    try:
        used.chain(bits, CHAIN)                     # (three frames: the parity is left flipped)
        used.seed(None, CHAIN, 0)
        blob = used.stream_state()
        assert blob == fresh.stream_state()
        st = parse(blob)
        assert st["insert"] == 1 and not st["halo"].any()
        assert same_bytes(used.chain(bits, CHAIN), fresh.chain(bits, CHAIN))
        with pytest.raises(pkg.DabGpuError):
            used.seed(None, CHAIN, 1)               # (a lead-in frame is needed anywhere else)
        # the device form without a lead-in frame, on a stream of the caller's (a handle, as for chain_dev) and on torch's
        import torch
        for stream in (torch.cuda.Stream().cuda_stream, None):
            used.chain(bits[:1], CHAIN)
            used.seed_dev(None, CHAIN, 0, stream=stream)
            torch.cuda.synchronize()
            assert used.stream_state() == blob
    finally:
        used.close()
        fresh.close()


def test_seed_leaves_the_diagnostics_of_the_last_chain_call(pkg):
    """The lead-in frame runs like the chain's internal runs: last_variant(), cfr_stats() and num_clipped() keep describing
    the last real chain call."""
    bits = coded_bits(1, 4)
    stages = G | F | R

    def extra(md):
        md.set_cfr(True, 50.0, 0.1)
        md.set_gain(2, 2.5, 32767.0 / 50000.0, 4.0)
        md.trace(True)
    md = context(pkg, 1, 8192000, "s16", True, extra)
    try:
        md.chain(bits[:2], stages)
        before = (md.last_variant(), md.num_clipped(), md.cfr_stats(0), md.cfr_stats(1))
        assert before[0] and before[1] > 0 and before[2]["num_clip"] > 0
        md.seed(bits[2], stages, 3)
        after = (md.last_variant(), md.num_clipped(), md.cfr_stats(0), md.cfr_stats(1))
        assert after[0] == before[0] and after[1] == before[1]
        for x, y in zip(before[2:], after[2:]):
            assert sorted(x) == sorted(y)
            for k in x:
                assert np.array_equal(np.asarray(x[k], np.float64), np.asarray(y[k], np.float64), equal_nan=True), k
    finally:
        md.close()


def test_seed_dev_on_a_stream_of_the_callers(pkg):
    import torch
    K = 3
    bits = coded_bits(1, K + 2)
    a, b = context(pkg, 1, 8192000, tii=True), context(pkg, 1, 8192000, tii=True)
    try:
        ya = a.chain(bits, CHAIN)
        d_bits = torch.from_numpy(bits).to("cuda:0")
        d_out = torch.empty((2, b.out_samples_per_frame(CHAIN)), dtype=torch.complex64, device="cuda:0")
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            b.seed_dev(d_bits[K - 1], CHAIN, K)
            b.chain_dev(d_bits[K:], 2, CHAIN, d_out)
        s.synchronize()
        assert same_bytes(d_out.cpu().numpy(), ya[K:])
        assert b.stream_state() == a.stream_state()
    finally:
        a.close()
        b.close()


# --------------------------------------------------------------------------- 3. the blob
def test_blob_of_a_fresh_context_and_after_set_resampler(pkg):
    md = context(pkg, 1, 8192000)
    try:
        assert md._lib.dabgpu_stream_state_bytes(md._h) == HEADER + 4096 * 8
        st = parse(md.stream_state())
        assert (st["magic"], st["version"], st["mode"], st["insert"], st["rs_in"], st["rs_out"], st["nin"], st["reserved"]) == \
            (0x53534744, 1, 1, 1, 2048000, 8192000, 4096, 0)
        assert st["halo"].size == 4096 and not st["halo"].any()
        md.chain(coded_bits(1, 2), CHAIN)
        assert parse(md.stream_state())["halo"].any()
        md.set_resampler(2048000, 8192000)                 # resets the halo, as ever -- and nothing else
        st = parse(md.stream_state())
        assert not st["halo"].any() and st["insert"] == 1
        md.chain(coded_bits(1, 1), CHAIN)
        md.set_resampler(2048000, 4096000)
        st = parse(md.stream_state())
        assert st["rs_out"] == 4096000 and not st["halo"].any() and st["insert"] == 0
    finally:
        md.close()


def test_blob_is_refused_where_it_does_not_belong(pkg):
    a = context(pkg, 1, 8192000)
    try:
        a.chain(coded_bits(1, 1), CHAIN)
        blob = a.stream_state()
        n = C.c_size_t()
        buf = C.create_string_buffer(len(blob))
        assert a._lib.dabgpu_get_stream_state(a._h, buf, len(blob) - 1, C.byref(n)) == -4 and n.value == len(blob)   # E_CAPACITY
        with pytest.raises(pkg.DabGpuError, match="too small"):
            a.stream_state(capacity=len(blob) - 1)
        assert a._lib.dabgpu_get_stream_state(a._h, None, len(blob), C.byref(n)) == -1
        assert a._lib.dabgpu_set_stream_state(a._h, None, len(blob)) == -1
        bad = {
            "another ratio": (context(pkg, 1, 4096000), blob, "ratio"),
            "another mode": (context(pkg, 2, 8192000), blob, "mode"),
            "one byte short": (context(pkg, 1, 8192000), blob[:-1], "size"),
            "one byte long": (context(pkg, 1, 8192000), blob + b"\0", "size"),
            "no header": (context(pkg, 1, 8192000), blob[:HEADER - 1], "header"),
            "magic": (context(pkg, 1, 8192000), b"XXXX" + blob[4:], "magic"),
            "version": (context(pkg, 1, 8192000), blob[:4] + b"\2\0\0\0" + blob[8:], "version"),
            "halo length": (context(pkg, 1, 8192000), blob[:32] + b"\0\0\0\0" + blob[36:], "halo length"),
        }
        try:
            for name, (md, data, word) in bad.items():
                fresh = md.stream_state()
                with pytest.raises(pkg.DabGpuError, match=word):
                    md.set_stream_state(data)
                assert md.stream_state() == fresh, name      # (a refused blob changes nothing)
        finally:
            for md, _, _ in bad.values():
                md.close()
    finally:
        a.close()


def test_blob_at_equal_rates_is_the_header_and_moves_the_tii_parity(pkg):
    """Native rate: no Resampler in the chain, the blob is the 40-byte header -- and it still carries the TII frame parity
    (K odd: frame K of the stream is one WITHOUT the TII symbol)."""
    K = 1
    bits = coded_bits(1, K + 2)
    a, b, c, d = (context(pkg, 1, 2048000, tii=True) for _ in range(4))
    try:
        stages = G | F | R                         # (RESAMPLE at equal rates is not in the chain)
        a.chain(bits[:K], stages)
        blob = a.stream_state()
        assert len(blob) == HEADER == a._lib.dabgpu_stream_state_bytes(a._h)
        assert parse(blob)["insert"] == 0 and parse(blob)["nin"] == 0
        b.set_stream_state(blob)
        yb = b.chain(bits[K:], stages)
        yc = c.chain(bits, stages)
        assert same_bytes(yb, yc[K:])
        assert not same_bytes(yb[0], d.chain(bits[K:K + 1], stages)[0])     # (the parity is what made the difference)
        d.seed(None, stages, K)                    # host-only at equal rates: no lead-in frame needed
        assert d.stream_state() == b.stream_state()
    finally:
        for md in (a, b, c, d):
            md.close()


# --------------------------------------------------------------------------- 4. partition
_whole = {}


def whole_stream(pkg, mode, out_rate, tii, n):
    key = (mode, out_rate, tii, n)
    if key not in _whole:
        md = context(pkg, mode, out_rate, None, tii, max_frames=n)
        try:
            _whole[key] = md.chain(coded_bits(mode, n), CHAIN).copy()
        finally:
            md.close()
    return _whole[key]


PARTITIONS = [(1, 8192000, True, n_ctx, chunk, 12) for n_ctx in (2, 3) for chunk in (1, 2, 5)] + \
             [(2, 2400000, True, 2, 5, 12), (3, 8192000, False, 3, 1, 12),
              # calls of 16 frames (runs of several symbols per workgroup, against the seed's one-frame call), many queued
              (1, 8192000, False, 2, 16, 72), (1, 8192000, True, 3, 16, 72)]


@pytest.mark.parametrize("mode,out_rate,tii,n_ctx,chunk,n", PARTITIONS)
def test_partitioned_stream_equals_one_context(pkg, mode, out_rate, tii, n_ctx, chunk, n):
    """12 frames of one stream over 2 and 3 contexts in chunks of 1, 2 and 5 frames (odd chunks flip the TII parity per
    chunk; 5 leaves a ragged tail), and 72 frames in chunks of 16: one context's bytes."""
    import importlib
    streams = importlib.import_module("odr-dabmod_amd.streams")
    bits = coded_bits(mode, n)
    want = whole_stream(pkg, mode, out_rate, tii, n)
    mods = [context(pkg, mode, out_rate, None, tii) for _ in range(n_ctx)]
    try:
        ps = streams.PartitionedStream(mods)
        got = ps.modulate(bits, CHAIN, chunk)
        assert got.shape == want.shape
        differ = [f for f in range(n) if not same_bytes(got[f], want[f])]
        assert not differ, differ
        if chunk == 5:
            # device-resident, into the caller's tensor, and a second stream through the same contexts
            import torch
            d_bits = torch.from_numpy(bits).to("cuda:0")
            d_out = torch.zeros(want.shape, dtype=torch.complex64, device="cuda:0")
            assert ps.modulate(d_bits, CHAIN, chunk, out=d_out) is not None
            assert same_bytes(d_out.cpu().numpy(), want)
    finally:
        for md in mods:
            md.close()


# --------------------------------------------------------------------------- 5. dabmod_file
def run_tool(tmp_path, fin, name, opts):
    fout = str(tmp_path / name)
    r = subprocess.run([os.path.join(HOST, "dabmod_file"), fin, fout] + opts, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    m = re.search(r"(\d+) clipped components", r.stderr)
    return np.fromfile(fout, dtype=np.uint8), r.stdout.split(), (int(m.group(1)) if m else None)


@pytest.mark.parametrize("fmt", ["complexf", "s16"])
def test_dabmod_file_contexts_write_the_file_of_one_context(tmp_path, fmt):
    """dabmod_file --batch 4 --contexts N: 11 transmission frames as batches of 4, 4, 3 over 2 and over 3 chains, each seeded
    from the frame before its batch -- the file, and the clipped count, of --contexts 1."""
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "odr-dabmod_amd", "csrc"), "-j2"])
    subprocess.check_call(["make", "-s", "-C", HOST, "-j2"])
    fin = str(tmp_path / "in.eti")
    synth_eti(44).tofile(fin)
    coef = str(tmp_path / "poly.coef")
    O.write_poly_file(coef, POLY_AM, POLY_PM)
    opts = ["--batch", "4", "--rate", "8192000", "--fir", "default", "--poly", coef, "--tii", "1,2", "--format", fmt]
    one, counts, clip = run_tool(tmp_path, fin, "one.iq", opts + ["--contexts", "1"])
    assert counts == ["44", "11", "11"] and one.size == 11 * 196608 * 4 * (8 if fmt == "complexf" else 4)
    assert (clip is None) == (fmt == "complexf")
    for n_ctx in (2, 3):
        got, counts, clip_n = run_tool(tmp_path, fin, "n%d.iq" % n_ctx, opts + ["--contexts", str(n_ctx)])
        assert counts == ["44", "11", "11"]
        assert got.size == one.size and np.array_equal(got, one), n_ctx
        assert clip_n == clip
    # --reference-latency holds frames back in FRONT of the chains: the frames that are modulated are the first N - k of the
    # stream, in order, so the split is the same split -- and the file (and the clipped count) is the one --contexts 1 writes
    lat = opts + ["--reference-latency"]
    one_l, counts_l, clip_1 = run_tool(tmp_path, fin, "one_l.iq", lat + ["--contexts", "1"])
    two_l, counts_2, clip_2 = run_tool(tmp_path, fin, "two_l.iq", lat + ["--contexts", "2"])
    assert counts_l == counts_2 == ["44", "11", "8"]
    assert np.array_equal(two_l, one_l) and np.array_equal(one_l, one[:one_l.size]) and clip_1 == clip_2
