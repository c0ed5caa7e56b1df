"""CicEqualizer in the fused chain (dabgpu_set_cic_equalizer): coded bits -> equalised carriers in one kernel
(carriers_from_bits_kernel, dabgpu_carriers_process), the from-carriers chain behind it.

1. the carriers are the oracle's stage composition BIT FOR BIT (qpsk -> freq_interleave -> diff_mod with the phase reference ->
   mux -> tii -> cic_equalize; every one of these is pinned to the reference's classes by tests/test_oracle_golden.py);
2. structure: a chain call from bits with CIC on is, byte for byte, the from-carriers chain on those carriers;
3. accuracy: the composition continued with the oracle's ofdm_generate -> gain_control -> guard_interval -> fir_filter
   (-> resampler -> poly) under the project's existing bars (tests/test_gpu_parity.py);
4. state: seeds, submit / collect, a change of (spacing, R) between calls on three lanes, ETI-fed calls;
5. refusals."""
import functools

import numpy as np
import pytest

import oracle as O
from tests.conftest import int_off_by_one_limit, record_bound
from tests.golden.synth import POLY_AM, POLY_PM, synth_eti

pytestmark = pytest.mark.gpu

G, F, R, P = 1, 2, 4, 8
# (mode: (spacing, R)): the parameter sets tests/test_oracle_golden.py pins against the reference's CicEqualizer
CIC = {1: [(2048, 8), (8192, 25)], 2: [(512, 4)], 3: [(256, 3)], 4: []}
TII = (3, 5)                      # comb, pattern
REL_RMS = 1e-6


def bits_eq(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.size > 0 and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a).view(np.uint8).reshape(-1), np.ascontiguousarray(b).view(np.uint8).reshape(-1)
    return a.size == b.size and a.size > 0 and np.array_equal(a, b)


def rel_rms(y, ref):
    return float(np.linalg.norm(y.astype(np.complex128) - ref) / max(np.linalg.norm(ref), 1e-30))


@functools.lru_cache(maxsize=None)
def coded_bits(mode, n, seed=4711):
    b = np.random.RandomState(seed + mode).randint(0, 256, (n, O.tf_input_bytes(mode))).astype(np.uint8)
    b.setflags(write=False)
    return b


@functools.lru_cache(maxsize=None)
def ref_carriers(mode, n, cic=None, tii_old=None, first_frame=0):
    """The oracle's stages composed, for frames first_frame ... first_frame + n - 1 of the stream coded_bits(mode, first_frame
    + n): (n, (nb_symbols + 1) * K) complex64.  tii_old: None = TII off, else the old_variant flag; TII sits on the even frames
    of the stream (src/TII.cpp:226-242)."""
    g = O.mode_params(mode)
    K = g["carriers"]
    pr, _ = O.phase_reference(mode)
    bits = coded_bits(mode, first_frame + n)
    acp = O.tii_pattern(mode, *TII) if tii_old is not None else None
    out = []
    for f in range(first_frame, first_frame + n):
        dm = O.diff_mod(pr, O.freq_interleave(O.qpsk_map(bits[f], K), mode), K)
        first = np.zeros(K, np.complex64)
        if acp is not None:
            first = O.tii_process(pr, acp, bool(tii_old), insert=(f % 2 == 0))
        z = O.signal_mux(first, dm)
        if cic:
            z = O.cic_equalize(z, K, cic[0], cic[1])
        out.append(z)
    out = np.stack(out)
    out.setflags(write=False)
    return out


def modulator(pkg, mode, cic=None, tii_old=None, setup=None, max_frames=8, **kw):
    md = pkg.Modulator(mode=mode, max_frames=max_frames, **kw)
    try:
        if cic:
            md.set_cic_equalizer(True, *cic)
        if tii_old is not None:
            md.set_tii(True, TII[0], TII[1], bool(tii_old))
        if setup:
            setup(md)
    except Exception:
        md.close()
        raise
    return md


# --------------------------------------------------------------------------- 1. the carriers, bit for bit
CARRIER_CASES = [(m, c, n, None) for m in (1, 2, 3, 4) for c in [None] + CIC[m] for n in (1, 3)]
CARRIER_CASES += [(m, c, 3, old) for m in (1, 2) for c in (None, CIC[m][0]) for old in (False, True)]
CARRIER_CASES += [(1, CIC[1][0], 1, False)]


@pytest.mark.parametrize("mode,cic,n,tii_old", CARRIER_CASES)
def test_carriers_equal_the_oracle_composition_bit_for_bit(pkg, mode, cic, n, tii_old):
    """Two calls of n frames in a row: the second starts where the first left the TII parity (n odd: on a frame without TII)."""
    md = modulator(pkg, mode, cic, tii_old)
    try:
        bits = coded_bits(mode, 2 * n)
        want = ref_carriers(mode, 2 * n, cic, tii_old)
        for call in range(2):
            got = md.carriers(bits[call * n:(call + 1) * n])
            w = want[call * n:(call + 1) * n]
            assert got.shape == w.shape
            assert bits_eq(got, w), (call, int((got.view(np.uint32) != w.view(np.uint32)).sum()))
        if tii_old is not None:
            K = md.geometry["carriers"]
            assert np.abs(want[0, :K]).max() > 0 and np.abs(want[1, :K]).max() == 0      # (the cases do carry TII)
    finally:
        md.close()


def test_carriers_dev_equals_the_host_entry(pkg):
    import torch
    mode, cic, n = 2, CIC[2][0], 3
    md = modulator(pkg, mode, cic, False)
    try:
        bits = coded_bits(mode, n)
        d_bits = torch.from_numpy(np.array(bits)).cuda()
        g = md.geometry
        d_out = torch.empty(n * (g["nb_symbols"] + 1) * g["carriers"], dtype=torch.complex64, device="cuda")
        md.trace(True)
        assert md.carriers_dev(d_bits, n, d_out) == d_out.numel() * 8
        torch.cuda.synchronize()
        assert md.last_variant() == ["carriers_from_bits_kernel"]
        assert bits_eq(d_out.cpu().numpy().reshape(n, -1), ref_carriers(mode, n, cic, False))
    finally:
        md.close()


# --------------------------------------------------------------------------- 2. structure
def _symbols(md, car, n, stages):
    import torch
    d_car = torch.from_numpy(np.array(car)).cuda()
    d_out = torch.empty(n * md.out_samples_per_frame(stages), dtype=torch.complex64, device="cuda")
    md.symbols_dev(d_car, n, stages, d_out)
    torch.cuda.synchronize()
    return d_out.cpu().numpy().reshape(n, -1)


@pytest.mark.parametrize("stages,rate", [(G, None), (G | F, None), (G | F | R | P, 8192000), (G | F | R, 2400000)])
def test_chain_with_cic_is_the_carriers_chain_on_the_equalised_carriers(pkg, stages, rate):
    mode, cic, n = 1, CIC[1][0], 3

    def setup(md):
        md.set_gain(2, 1.0, 1.0 / 50000.0, 4.0)
        md.set_tii(True, TII[0], TII[1], False)
        if rate:
            md.set_resampler(2048000, rate)
            md.set_poly(POLY_AM, POLY_PM)
        md.trace(True)

    a, b, c = modulator(pkg, mode, cic, setup=setup), modulator(pkg, mode, None, setup=setup), modulator(pkg, mode, cic, setup=setup)
    try:
        bits = coded_bits(mode, n)
        y = a.chain(bits, stages)
        names = a.last_variant()
        assert names[0] == "carriers_from_bits_kernel" and "bits=0" in names[1], names
        assert not any("tii" in k for k in names[1:]), names
        # CIC off, fed the equalised carriers
        yb = _symbols(b, ref_carriers(mode, n, cic, False), n, stages)
        assert same_bytes(y, yb)
        assert b.last_variant() == names[1:]
        # CIC on, fed the carriers without the equaliser
        yc = _symbols(c, ref_carriers(mode, n, None, False), n, stages)
        assert c.last_variant() == ["cic_kernel"] + names[1:]
        assert same_bytes(y, yc)
        # the device path from bits
        import torch
        d_out = torch.empty(y.size, dtype=torch.complex64, device="cuda")
        a2 = modulator(pkg, mode, cic, setup=setup)
        try:
            a2.chain_dev(torch.from_numpy(np.array(bits)).cuda(), n, stages, d_out)
            torch.cuda.synchronize()
            assert same_bytes(d_out.cpu().numpy(), y)
        finally:
            a2.close()
    finally:
        for md in (a, b, c):
            md.close()


def test_cic_off_is_the_context_that_never_heard_of_the_setter(pkg):
    mode, n, stages = 1, 2, G | F
    bits = coded_bits(mode, n)
    plain = modulator(pkg, mode, setup=lambda md: md.trace(True))
    toggled = modulator(pkg, mode, CIC[1][0], setup=lambda md: md.trace(True))
    try:
        y0 = plain.chain(bits, stages)
        y_on = toggled.chain(bits, stages)
        toggled.set_cic_equalizer(False)
        y1 = toggled.chain(bits, stages)
        assert same_bytes(y0, y1) and not same_bytes(y0, y_on)
        assert plain.last_variant() == toggled.last_variant() and len(plain.last_variant()) == 1
        assert "bits=1" in plain.last_variant()[0]
    finally:
        plain.close()
        toggled.close()


# --------------------------------------------------------------------------- 3. accuracy against the oracle's stages
def oracle_chain(mode, car, stages, gain_mode=2, normalise=1.0 / 50000.0, overlap=0, cfr=None, rate=None, poly=False):
    """The oracle's stages behind the carriers, frame by frame as dabo_chain_process runs them.  Returns (stream (n, per),
    symbols before GainControl (n, nsym + 1, N), symbols behind it)."""
    g = O.mode_params(mode)
    K, N, nsym = g["carriers"], g["spacing"], g["nb_symbols"]
    rs = O.Resampler(2048000, rate, N) if rate else None
    taps = O.fir_default_taps()
    out, xs, ygs = [], [], []
    for f in range(car.shape[0]):
        if cfr:
            x = O.ofdm_generate_cfr(car[f], nsym + 1, K, N, cfr[0], cfr[1], (f + 1) % (nsym + 1))[0]
        else:
            x = O.ofdm_generate(car[f], nsym + 1, K, N)
        yg = O.gain_control(x, N, gain_mode, 1.0, normalise, 4.0) if stages & G else x
        y = O.guard_interval(yg, nsym, N, g["null_size"], g["sym_size"], overlap)
        if stages & F:
            y = O.fir_filter(y, taps)
        if rs:
            y = rs.process(y)
        if poly:
            y = O.memless_poly(y, POLY_AM, POLY_PM)
        out.append(y)
        xs.append(x.reshape(nsym + 1, N))
        ygs.append(yg.reshape(nsym + 1, N))
    return np.stack(out), np.stack(xs), np.stack(ygs)


def gain_bars(tag, y, ref, xs, ygs, mode, gain_mode, normalise, exact_rounding, head, tail):
    """The a7 scalar and chain-total bars of INTEGRATION.md F (tests/test_gpu_parity.py::_hold_gain_bars), with the reference
    symbols taken from the composition above: per symbol the scale alpha between device and oracle is the ratio of the two
    gain scalars; mode var under the default rounding is also held against the EXACT variance of the oracle's own symbols."""
    g = O.mode_params(mode)
    ns, ss, nsym = g["null_size"], g["sym_size"], g["nb_symbols"]
    peak = np.abs(ref).max()
    da = res = dex = 0.0
    for f in range(ref.shape[0]):
        ratio = np.ones(nsym + 1)
        if gain_mode == 2:
            for s in range(1, nsym + 1):
                x, v = xs[f, s].astype(np.complex128), ygs[f, s].astype(np.complex128)
                g_ref = np.vdot(x, v).real / np.vdot(x, x).real
                g_exact = 32767.0 / (4.0 * max(x.real.std(), x.imag.std())) * float(np.float32(normalise))
                ratio[s] = g_ref / g_exact
            ratio[0] = ratio[1]
        for s in range(nsym + 1):
            lo = 0 if s == 0 else ns + (s - 1) * ss
            hi = (ns if s == 0 else lo + ss) - tail
            lo += head
            r, d = ref[f, lo:hi].astype(np.complex128), y[f, lo:hi].astype(np.complex128)
            e = np.vdot(r, r).real
            if e == 0.0:
                res = max(res, np.abs(d).max() / peak)
                continue
            alpha = np.vdot(r, d).real / e
            da = max(da, abs(alpha - 1.0))
            res = max(res, np.abs(d - alpha * r).max() / peak)
            dex = max(dex, abs(alpha * ratio[s] - 1.0))
    total = np.abs(y - ref).max() / peak
    print("%s: a7 vs reference %.3g, vs exact %.3g, residual %.3g, total %.3g" % (tag, da, dex, res, total))
    ok = True
    if gain_mode == 2 and exact_rounding:
        ok &= record_bound("a7 gain scalar against the exact variance, rel, " + tag, dex, 2e-7)
        ok &= record_bound("a7 gain scalar against the reference's recurrence, rel, " + tag, da, 8e-7)
        ok &= record_bound("chain total max-abs / |out|_inf against the reference (gain mode 2), " + tag, total, 8e-7, warn_at=7e-7)
    elif gain_mode == 2:
        ok &= record_bound("a7 gain scalar against the reference's recurrence (gain rounding REFERENCE), rel, " + tag, da, 3e-7)
        ok &= record_bound("chain total max-abs / |out|_inf against the reference (gain rounding REFERENCE), " + tag, total, 7e-7)
    else:
        ok &= record_bound("a7 gain scalar (mode %d) against the reference's, rel, " % gain_mode + tag, da, 3.5e-7)
        ok &= record_bound("chain total max-abs / |out|_inf against the reference (gain mode %d), " % gain_mode + tag, total, 7e-7)
    ok &= record_bound("max-abs / |out|_inf after the gain scalar (symbol interiors), " + tag, res, 6.2e-7)
    return ok


ACCURACY = [
    # mode, cic, gain mode, reference rounding, overlap, cfr, tii
    (1, (2048, 8), 2, False, 0, False, False),
    (1, (8192, 25), 2, False, 0, False, False),
    (1, (2048, 8), 0, False, 0, False, False),
    (1, (2048, 8), 1, False, 0, False, False),
    (1, (2048, 8), 2, True, 0, False, False),
    (1, (2048, 8), 2, False, 10, False, False),
    (1, (2048, 8), 2, False, 0, True, False),
    (1, (2048, 8), 2, False, 0, False, True),
    (3, (256, 3), 2, False, 0, False, False),
    (3, (256, 3), 1, False, 10, False, False),
]


@pytest.mark.parametrize("mode,cic,gain_mode,ref_rounding,overlap,cfr,tii", ACCURACY)
def test_chain_with_cic_against_the_oracle(pkg, mode, cic, gain_mode, ref_rounding, overlap, cfr, tii):
    """cfg 3 (GainControl + FIRFilter) with the equaliser: rel-RMS < 1e-6 per frame, and -- without CFR, whose clipping is not
    a scale -- the a7 and chain-total bars.  CIC changes the per-carrier magnitudes by up to filter.max() (2.6 for (2048, 8)): a
    bar exceeded here is a finding about the carriers path's variance statistic, not a reason to widen it."""
    n, stages = 2, G | F
    K = O.mode_params(mode)["carriers"]
    normalise = 1.0 / 50000.0
    clip = (float(np.float32(60.0 * np.sqrt(K / 1536.0))), 0.1) if cfr else None

    def setup(md):
        md.set_gain(gain_mode, 1.0, normalise, 4.0)
        md.set_gain_rounding(ref_rounding)
        md.set_window_overlap(overlap)
        if clip:
            md.set_cfr(True, *clip)

    md = modulator(pkg, mode, cic, False if tii else None, setup=setup)
    try:
        y = md.chain(coded_bits(mode, n), stages)
        ref, xs, ygs = oracle_chain(mode, ref_carriers(mode, n, cic, False if tii else None), stages, gain_mode, normalise, overlap, clip)
        assert y.shape == ref.shape
        tag = "CIC %s mode %d gain %d%s overlap %d%s%s" % (cic, mode, gain_mode, " REFERENCE" if ref_rounding else "", overlap,
                                                           " cfr" if cfr else "", " tii" if tii else "")
        worst = max(rel_rms(y[f], ref[f]) for f in range(n))
        assert record_bound("rel-RMS per frame, " + tag, worst, REL_RMS)
        if not cfr:
            assert gain_bars(tag, y, ref, xs, ygs, mode, gain_mode, normalise, not ref_rounding, head=overlap, tail=44 + overlap)
    finally:
        md.close()


def test_chain_with_cic_resampled_and_s16_against_the_oracle(pkg):
    mode, cic, n = 1, CIC[1][0], 2
    car = ref_carriers(mode, n, cic, None)
    # x4 with the predistorter, complexf
    md = modulator(pkg, mode, cic, setup=lambda m: (m.set_gain(2, 1.0, 1.0 / 50000.0, 4.0), m.set_resampler(2048000, 8192000),
                                                    m.set_poly(POLY_AM, POLY_PM)))
    try:
        y = md.chain(coded_bits(mode, n), G | F | R | P)
        ref = oracle_chain(mode, car, G | F, 2, 1.0 / 50000.0, rate=8192000, poly=True)[0]
        assert record_bound("rel-RMS per frame, CIC (2048, 8) x4 resampler + predistorter",
                            max(rel_rms(y[f], ref[f]) for f in range(n)), REL_RMS)
    finally:
        md.close()
    # s16 at the native rate
    norm = 32767.0 / 50000.0
    md = modulator(pkg, mode, cic, setup=lambda m: (m.set_gain(2, 1.0, norm, 4.0), m.set_output_format("s16")))
    try:
        y = md.chain(coded_bits(mode, n), G | F)
        want, _ = O.format_convert(oracle_chain(mode, car, G | F, 2, norm)[0], "s16")
        want = want.reshape(y.shape)
        d = np.abs(y.astype(np.int32) - want.astype(np.int32))
        assert d.max() <= 1
        assert record_bound("s16 components one step apart, CIC (2048, 8) cfg 3", float((d == 1).mean()),
                            int_off_by_one_limit(want, 2048, "s16"))
    finally:
        md.close()


# --------------------------------------------------------------------------- 4. state
def test_resampled_stream_with_tii_and_cic_split_over_two_contexts(pkg):
    mode, cic, n, stages = 1, CIC[1][0], 4, G | F | R

    def setup(md):
        md.set_gain(2, 1.0, 1.0 / 50000.0, 4.0)
        md.set_resampler(2048000, 4096000)

    bits = coded_bits(mode, n)
    whole, first, second = (modulator(pkg, mode, cic, True, setup=setup) for _ in range(3))
    try:
        y = whole.chain(bits, stages)
        for k in (1, 2):                                    # (a seed on an odd and on an even frame: both parities)
            first.seed(None, stages, 0)
            second.seed(bits[k - 1], stages, k)
            assert same_bytes(first.chain(bits[:k], stages), y[:k])
            assert same_bytes(second.chain(bits[k:], stages), y[k:])
            assert second.stream_state() == whole.stream_state()
    finally:
        for md in (whole, first, second):
            md.close()


def test_submit_collect_with_cic_equals_the_synchronous_call(pkg):
    mode, cic, stages = 2, CIC[2][0], G | F
    bits = coded_bits(mode, 3)
    sync, asyn = modulator(pkg, mode, cic, False), modulator(pkg, mode, cic, False)
    try:
        y = sync.chain(bits, stages)
        asyn.submit(bits[:1], stages)
        asyn.submit(bits[1:], stages)
        got = np.concatenate([asyn.collect().reshape(-1), asyn.collect().reshape(-1)])
        assert same_bytes(got, y)
    finally:
        sync.close()
        asyn.close()


def test_changing_the_cic_parameters_between_queued_calls(pkg):
    """Three lanes, nothing waited for: every call sees its own (spacing, R) -- the table is rewritten only after the lanes
    have drained -- and gives the bytes of a fresh one-lane context with those parameters."""
    import torch
    mode, stages, n = 1, G | F, 2
    bits = coded_bits(mode, n)
    d_bits = torch.from_numpy(np.array(bits)).cuda()
    torch.cuda.synchronize()
    params = [(2048, 8), (8192, 25), (2048, 8), (2048, 6), None]
    md = modulator(pkg, mode)
    try:
        md.set_lanes(3)
        per = md.out_samples_per_frame(stages)
        outs = [torch.zeros(n * per, dtype=torch.complex64, device="cuda") for _ in params]
        torch.cuda.synchronize()
        for p, d_out in zip(params, outs):
            md.set_cic_equalizer(p is not None, *(p or (0, 0)))
            md.chain_dev_queued(d_bits, n, stages, d_out)
        md.synchronize()
        for p, d_out in zip(params, outs):
            fresh = modulator(pkg, mode, p, setup=lambda m: m.set_lanes(1))
            try:
                assert same_bytes(d_out.cpu().numpy(), fresh.chain(bits, stages)), p
            finally:
                fresh.close()
    finally:
        md.close()


def test_eti_fed_chain_with_cic_equals_the_chain_on_the_front_ends_bits(pkg):
    mode, cic, stages = 1, CIC[1][0], G | F
    eti = synth_eti(8)
    a, b = modulator(pkg, mode, cic, False), modulator(pkg, mode, cic, False)
    try:
        a.frontend_configure(eti[0])
        b.frontend_configure(eti[0])
        y = a.chain_eti(eti, stages)
        assert same_bytes(y, b.chain(b.eti_to_bits(eti), stages))
    finally:
        a.close()
        b.close()


# --------------------------------------------------------------------------- 5. refusals
def test_refusals(pkg):
    md = pkg.Modulator(mode=1, max_frames=2)
    try:
        try:
            md.cic_equalizer(np.zeros(1536, np.complex64), 0, 8)
            stage_message = None
        except pkg.DabGpuError as e:
            stage_message = str(e)
        assert stage_message
        for args in ((1, 0, 8), (1, 2048, 0)):
            with pytest.raises(pkg.DabGpuError) as ei:
                md.set_cic_equalizer(*args)
            assert str(ei.value) == stage_message
        md.set_cic_equalizer(0, 0, 0)                         # off needs no parameters
        with pytest.raises(pkg.DabGpuError):
            md.carriers(coded_bits(1, 1).reshape(-1)[:-4])
        with pytest.raises(pkg.DabGpuError):
            md.carriers(np.zeros(0, np.uint8))
    finally:
        md.close()
