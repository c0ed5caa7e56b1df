"""The oracle against the golden fixtures generated from the reference's own
stage classes (tests/golden/make_golden.py), and against independent float64
math for the two FFTW-backed stages.  CPU only."""
import hashlib
import json
import os

import numpy as np
import pytest

import oracle as O
from tests.conftest import ROOT
from tests.receiver import dab_demodulate_mode1
from tests.golden.synth import (LUT_SCALE, POLY_AM, POLY_PM, format_edges, format_input, lut_table, synth_bits,
                                synth_signal)

GOLD_DIR = os.path.join(os.path.dirname(__file__), "golden")
GOLD = json.load(open(os.path.join(GOLD_DIR, "golden.json")))["modes"]
LIVE = json.load(open(os.path.join(GOLD_DIR, "live_reference.json")))["oracle_mode4_seed2024"]


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def bits_for(mode):
    b = np.fromfile(os.path.join(GOLD_DIR, "bits_mode%d.bin" % mode), dtype=np.uint8)
    assert b.size == O.tf_input_bytes(mode)
    return b


@pytest.mark.parametrize("mode", [1, 2, 3, 4])
def test_synth_generators_reproduce_committed_inputs(mode):
    assert np.array_equal(synth_bits(O.tf_input_bytes(mode), seed=mode), bits_for(mode))
    m = O.mode_params(mode)
    x = synth_signal((m["nb_symbols"] + 1) * m["spacing"], seed=100 + mode)
    assert sha(x) == GOLD[str(mode)]["synth_signal"]["sha256"]


@pytest.mark.parametrize("mode", [1, 2, 3, 4])
def test_integer_stages_bit_exact_vs_reference(mode):
    g = GOLD[str(mode)]
    m = O.mode_params(mode)
    K = m["carriers"]
    q = O.qpsk_map(bits_for(mode), K)
    assert sha(q) == g["qpsk"]["sha256"]
    fi = O.freq_interleave(q, mode)
    assert sha(fi) == g["freq_interleave"]["sha256"]
    pr, _ = O.phase_reference(mode)
    assert sha(pr) == g["phase_reference"]["sha256"]
    dm = O.diff_mod(pr, fi, K)
    assert sha(dm) == g["diff_mod"]["sha256"]
    mx = O.signal_mux(np.zeros(K, np.complex64), dm)
    assert sha(mx) == g["signal_mux"]["sha256"]


@pytest.mark.parametrize("mode", [1, 2, 3, 4])
def test_float_stages_bit_exact_vs_reference(mode):
    g = GOLD[str(mode)]
    m = O.mode_params(mode)
    N = m["spacing"]
    x = synth_signal((m["nb_symbols"] + 1) * N, seed=100 + mode)
    for gm, name in ((0, "fix"), (1, "max"), (2, "var")):
        for norm, nn in ((1.0, "n1"), (1.0 / 50000.0, "n50000")):
            y = O.gain_control(x, N, gm, 1.0, norm, 4.0)
            assert sha(y) == g["gain_%s_%s" % (name, nn)]["sha256"], (name, nn)
    assert sha(O.gain_control(x, N, 2, 0.8, 1.0 / 50000.0, 3.5)) == g["gain_var_dig0.8_var3.5"]["sha256"]
    xg = O.gain_control(x, N, 2, 1.0, 1.0 / 50000.0, 4.0)
    for ov in (0, 10):
        y = O.guard_interval(xg, m["nb_symbols"], N, m["null_size"], m["sym_size"], ov)
        assert sha(y) == g["guard_ov%d" % ov]["sha256"], ov
    gi = O.guard_interval(xg, m["nb_symbols"], N, m["null_size"], m["sym_size"], 0)
    f = O.fir_filter(gi, O.fir_default_taps())
    assert sha(f) == g["fir_default"]["sha256"]
    assert g["fir_default"]["sha256"] == g["fir_tapsfile"]["sha256"]
    assert sha(O.memless_poly(f, POLY_AM, POLY_PM)) == g["poly"]["sha256"]
    assert sha(O.memless_poly(f, [1, 0, 0, 0, 0], [0, 0, 0, 0, 0])) == g["poly_identity_file"]["sha256"]
    assert sha(O.memless_lut(f, LUT_SCALE, lut_table())) == g["lut"]["sha256"]


@pytest.mark.parametrize("mode", [1, 2, 3, 4])
@pytest.mark.parametrize("fmt", ["s16", "u8", "s8"])
def test_format_converter_bit_exact_vs_reference(mode, fmt):
    """f-2: integer output and the clipped-component count are the reference's."""
    g = GOLD[str(mode)]
    y, clipped = O.format_convert(format_input(O.tf_samples(mode), 200 + mode, fmt), fmt)
    assert sha(y) == g["format_%s" % fmt]["sha256"]
    assert clipped == g["format_%s" % fmt]["clipped"]
    ye, ce = O.format_convert(format_edges(fmt), fmt)
    assert [int(v) for v in ye] == g["format_edges_%s" % fmt]["out"]
    assert ce == g["format_edges_%s" % fmt]["clipped"]


@pytest.mark.parametrize("mode", [1, 2, 3, 4])
def test_cic_equalizer_bit_exact_vs_reference(mode):
    K = O.mode_params(mode)["carriers"]
    x = synth_signal(5 * K, seed=600 + mode)
    for sp, R in ((2048, 8), (8192, 25), (512, 4), (256, 3)):
        assert sha(O.cic_equalize(x, K, sp, R)) == GOLD[str(mode)]["cic_%d_%d" % (sp, R)]["sha256"]
    with pytest.raises(ValueError):
        O.cic_equalize(x[:-1], K, 2048, 8)


def _mux_symbols(mode, seed=None):
    m = O.mode_params(mode)
    K = m["carriers"]
    bits = bits_for(mode) if seed is None else synth_bits(O.tf_input_bytes(mode), seed=seed)
    pr, _ = O.phase_reference(mode)
    return O.signal_mux(np.zeros(K, np.complex64), O.diff_mod(pr, O.freq_interleave(O.qpsk_map(bits, K), mode), K))


@pytest.mark.parametrize("mode", [1, 2, 3, 4])
def test_papr_stats_vs_reference_class(mode):
    """f-3: PAPRStats::process_block / calculate_papr (src/PAPRStats.cpp) -- the oracle's per-symbol
    (peak, mean) pairs reduce to the reference's figure."""
    g = GOLD[str(mode)]["papr_synth_signal"]
    m = O.mode_params(mode)
    N, nsym = m["spacing"], m["nb_symbols"] + 1
    x = synth_signal(nsym * N, seed=100 + mode).reshape(nsym, N)
    p2 = (x.real.astype(np.float32) ** 2 + x.imag.astype(np.float32) ** 2).astype(np.float64)
    pairs = np.stack([p2.max(axis=1), p2.sum(axis=1) / N], axis=1)
    assert abs(O.papr_db(pairs) - g["db"]) < 1e-9
    assert g["db_too_few_blocks"] == 0.0


@pytest.mark.parametrize("mode", [1, 3])
def test_cfr_matches_float64_model(mode):
    """f-3: clip -> FFT -> error clip -> IFFT (src/OfdmGenerator.cpp:310-373) against an independent
    numpy model (tests/cfr_model.py: pocketfft, complex128 throughout)."""
    from tests.cfr_model import cfr_model
    m = O.mode_params(mode)
    K, N, nsym = m["carriers"], m["spacing"], m["nb_symbols"] + 1
    z = _mux_symbols(mode)
    clip, eclip, mer_index = np.float32(50.0 * np.sqrt(K / 1536.0)), np.float32(0.1), 7
    y, st, papr = O.ofdm_generate_cfr(z, nsym, K, N, clip, eclip, mer_index)
    mdl = cfr_model(z, nsym, K, N, clip, eclip)
    assert np.linalg.norm(y - mdl.y.ravel()) / np.linalg.norm(mdl.y) < 1e-6
    # decisions next to a threshold may fall on either side
    assert abs(st["num_clip"] - mdl.num_clip) <= 3 and abs(st["num_error_clip"] - mdl.num_error_clip) <= 3
    assert st["num_clip"] > 0.05 * nsym * N and st["num_error_clip"] > 0.3 * nsym * N   # CFR is really active
    mer = 10 * np.log10(mdl.mer_iq[mer_index] / mdl.mer_delta[mer_index])
    assert abs(st["mer_db"] - mer) < 1e-3
    assert np.allclose(papr[1:, 0], mdl.papr_before[1:, 0], rtol=1e-5)
    assert np.allclose(papr[1:, 3], mdl.papr_after[1:, 1], rtol=1e-5)
    assert not papr[0].any()                                    # blank null symbol
    # thresholds out of reach: CFR is the identity and nothing is counted
    y2, st2, _ = O.ofdm_generate_cfr(z, nsym, K, N, 1e9, 1e9, 0)
    assert np.linalg.norm(y2 - O.ofdm_generate(z, nsym, K, N)) / np.linalg.norm(y2) < 2e-7
    assert st2["num_clip"] == 0 and st2["num_error_clip"] == 0 and np.isnan(st2["mer_db"])


@pytest.mark.parametrize("mode", [1, 2])
def test_tii_bit_exact_vs_reference(mode):
    """f-4: every comb x pattern, old and new variant, inserting call and idle call."""
    g = GOLD[str(mode)]
    pr, _ = O.phase_reference(mode)
    for ov, name in ((0, "new"), (1, "old")):
        parts = []
        for c in range(24):
            for p in range(70):
                acp = O.tii_pattern(mode, c, p)
                parts += [O.tii_process(pr, acp, ov, True), O.tii_process(pr, acp, ov, False)]
        assert sha(np.concatenate(parts)) == g["tii_all_%s" % name]["sha256"]
    one = O.tii_process(pr, O.tii_pattern(mode, 3, 5), False, True)
    assert [int(i) for i in np.flatnonzero(one)] == g["tii_c3_p5"]["set"]
    assert g["tii_c3_p5"]["idle_calls_all_zero"] and g["tii_c3_p5"]["third_equals_first"]
    assert g["tii_disabled"]["all_zero"]


@pytest.mark.parametrize("args", [(3, 0, 0), (4, 0, 0), (1, 24, 0), (1, -1, 0), (1, 0, 70), (2, 0, -1)])
def test_tii_rejects_what_the_reference_throws_on(args):
    with pytest.raises(ValueError):
        O.tii_pattern(*args)


def test_chain_with_tii_alternates_frames():
    """TII replaces the null symbol on frames 0, 2, 4 ... of a stream (TII::m_insert starts true)."""
    bits = np.stack([synth_bits(O.tf_input_bytes(1), seed=60 + i) for i in range(3)])
    plain = O.Chain(mode=1, stages=3, gain_mode=2, normalise=1 / 50000.).process(bits)
    tii = O.Chain(mode=1, stages=3, gain_mode=2, normalise=1 / 50000., tii=(3, 5, False)).process(bits)
    null = O.mode_params(1)["null_size"]
    assert np.array_equal(plain[1], tii[1])
    for f in (0, 2):
        assert np.array_equal(plain[f][null:], tii[f][null:])
        p_null = np.mean(np.abs(tii[f][:null - 44]) ** 2)
        p_data = np.mean(np.abs(tii[f][null:]) ** 2)
        assert not plain[f][:null - 44].any()
        # 32 of 1536 carriers: 1/48 of the power of a data symbol (ETSI TR 101 496-3 5.4.2.2)
        assert 0.7 / 48 < p_null / p_data < 1.4 / 48


def test_format_converter_rejects_unknown_format():
    with pytest.raises(ValueError):
        O.format_convert(np.zeros(4, np.float32), "s32")


def test_fir_default_taps_are_symmetric_lowpass():
    t = O.fir_default_taps()
    assert t.size == 45 and np.array_equal(t, t[::-1])
    assert abs(float(t.astype(np.float64).sum()) - 1.0) < 2e-3


@pytest.mark.parametrize("mode", [1, 2, 3, 4])
def test_freq_interleave_table_is_a_permutation(mode):
    idx = O.freq_interleave_table(mode)
    K = O.mode_params(mode)["carriers"]
    assert sorted(idx.tolist()) == list(range(K))


def test_input_size_checks_match_reference_throws():
    with pytest.raises(ValueError):
        O.qpsk_map(np.zeros(383, np.uint8), 1536)       # src/QpskSymbolMapper.cpp:109-115
    with pytest.raises(ValueError):
        O.freq_interleave(np.zeros(1535, np.complex64), 1)  # src/FrequencyInterleaver.cpp:110-113
    with pytest.raises(ValueError):
        O.diff_mod(np.zeros(1536, np.complex64), np.zeros(100, np.complex64), 1536)
    with pytest.raises(ValueError):
        O.ofdm_generate(np.zeros(10, np.complex64), 77, 1536, 2048)  # src/OfdmGenerator.cpp:170-177
    with pytest.raises(ValueError):
        O.gain_control(np.zeros(2047, np.complex64), 2048, 2)        # src/GainControl.cpp:127-130


@pytest.mark.parametrize("mode", [1, 3])
def test_ofdm_matches_float64_dft_definition(mode):
    """a6: FFTW is absent; the oracle is pinned by definition to the exact
    unnormalised backward DFT (numpy pocketfft float64 as the independent check)."""
    m = O.mode_params(mode)
    K, N, nsym = m["carriers"], m["spacing"], m["nb_symbols"] + 1
    pr, _ = O.phase_reference(mode)
    dm = O.diff_mod(pr, O.freq_interleave(O.qpsk_map(bits_for(mode), K), mode), K)
    z = O.signal_mux(np.zeros(K, np.complex64), dm)
    t = O.ofdm_generate(z, nsym, K, N).reshape(nsym, N)
    X = np.zeros((nsym, N), np.complex128)
    zz = z.reshape(nsym, K)
    X[:, 1:K // 2 + 1] = zz[:, :K // 2]          # src/OfdmGenerator.cpp:211-221
    X[:, N - K // 2:] = zz[:, K // 2:]
    ref = np.fft.ifft(X, axis=1) * N
    assert np.all(t[0] == 0)
    rel = np.linalg.norm(t - ref) / np.linalg.norm(ref)
    assert rel < 1e-7
    # unnormalised: data-symbol RMS is sqrt(K)
    assert abs(np.sqrt(np.mean(np.abs(t[1:]) ** 2)) - np.sqrt(K)) < 1e-3 * np.sqrt(K)


def _resampler_model(x, nin, nout, factor):
    w = (0.5 * (1 - np.cos(2 * np.pi * np.arange(nin) / (nin - 1)))).astype(np.float32)
    hin, hout = nin // 2, nout // 2
    prev = np.zeros(hin, np.complex128)
    tail = np.zeros(hout, np.complex128)
    out = []
    for h in range(x.size // hin):
        cur = x[h * hin:(h + 1) * hin].astype(np.complex128)
        F = np.fft.fft(np.concatenate([prev, cur]) * w)
        B = np.zeros(nout, np.complex128)
        if nout > nin:
            B[:hin] = F[:hin]
            B[nout - hin:] = F[hin:]
            B[hin] = F[hin]
        else:
            B[:hout] = F[:hout]
            B[hout:] = F[nin - hout:]
            B[hout] = 0.5 * (F[nin - hout] + F[hout])
        y = np.fft.ifft(B * factor) * nout
        out.append(tail + y[:hout])
        tail = y[hout:]
        prev = cur
    return np.concatenate(out)


@pytest.mark.parametrize("out_rate", [8192000, 4096000, 1024000, 2400000, 3072000, 6144000, 2304000, 2500000])
def test_resampler_matches_float64_model_across_two_frames(out_rate):
    """a10: state carries across frames (src/Resampler.cpp:142-192): feed two TFs."""
    r = O.Resampler(2048000, out_rate, 2048)
    assert r.fft_in == 4096
    x = synth_signal(2 * 49152, seed=5) * np.float32(1 / 64)
    y = np.concatenate([r.process(x[:49152]), r.process(x[49152:])])
    ref = _resampler_model(x, r.fft_in, r.fft_out, np.float64(r.factor))
    assert y.size == x.size * r.L // r.M
    assert np.linalg.norm(y - ref) / np.linalg.norm(ref) < 2e-7


@pytest.mark.parametrize("mode", [1, 2, 3, 4])
def test_reference_var_gain_recurrence_against_the_exact_variance(mode):
    """Why the fused chain's a7 bar is stated against the EXACT variance: GainControl's mode var is an fp32 running-mean /
    running-variance recurrence with a division per sample (src/GainControl.cpp:259-319; the oracle's gain_control is that
    code, bit-identical to the reference class -- test_float_stages_bit_exact_vs_reference), and its result is itself
    several 1e-7 away from the exact population variance of its own input -- more than the 2e-7 SURVEY 8(a) allots to a7.
    An implementation that does not replay the recurrence sample by sample (the stand-alone gain kernel does; a fused
    kernel cannot) can therefore agree with the reference's scalar only to that distance."""
    g = O.mode_params(mode)
    K, N, nsym = g["carriers"], g["spacing"], g["nb_symbols"] + 1
    pr, _ = O.phase_reference(mode)
    worst = 0.0
    for seed in range(3):
        bits = synth_bits(O.tf_input_bytes(mode), seed=1000 + seed)
        z = O.signal_mux(np.zeros(K, np.complex64), O.diff_mod(pr, O.freq_interleave(O.qpsk_map(bits, K), mode), K))
        x = O.ofdm_generate(z, nsym, K, N).reshape(nsym, N)
        y = O.gain_control(x.reshape(-1), N, 2, 1.0, 1.0, 4.0).reshape(nsym, N)
        for s_ in range(1, nsym):
            xs, ys = x[s_].astype(np.complex128), y[s_].astype(np.complex128)
            g_ref = np.vdot(xs, ys).real / np.vdot(xs, xs).real
            g_exact = 32767.0 / (4.0 * max(xs.real.std(), xs.imag.std()))
            worst = max(worst, abs(g_ref / g_exact - 1.0))
    from tests.conftest import record_bound
    record_bound("reference's own var-gain recurrence against the exact variance, rel, mode %d" % mode, worst, 6e-7)
    assert 1.5e-7 < worst < 6e-7, worst


@pytest.mark.parametrize("mode", [1, 2, 3, 4])
def test_reference_var_gain_recurrence_moves_with_the_transform_in_front_of_it(mode):
    """What "the reference's scalar" is worth as a target once the transform in front of GainControl is not FFTW's: the SAME
    bit-pinned recurrence on the symbols of two correct transforms -- the oracle's (float64 inside, rounded once) and an
    independent fp32 one (numpy's single-precision pocketfft, rel-RMS ~1e-7 from the first, like any fp32 FFT incl. the
    device's and FFTW's own) -- returns scalars that differ by 1 ... 2.5e-7 (here; 1.9 ... 2.3e-7 measured between the device's
    transform and the oracle's, tests/test_gain_rounding_gpu.py), more than the exact variances of the same two sets of symbols do.  The recurrence's rounding path depends on the last bits of its input, so 2e-7 of the
    reference's scalar is reachable only bit-for-bit on identical symbols -- which is what
    dabgpu_set_gain_rounding(ctx, REFERENCE) and the stand-alone gain stage deliver (tests/test_gain_rounding_gpu.py) -- and
    along a chain the bar for the replayed scalar is this sensitivity, 3e-7."""
    g = O.mode_params(mode)
    K, N, nsym = g["carriers"], g["spacing"], g["nb_symbols"] + 1
    pr, _ = O.phase_reference(mode)
    d_rec, d_exact = 0.0, 0.0
    for seed in range(3):
        bits = synth_bits(O.tf_input_bytes(mode), seed=1000 + seed)
        z = O.signal_mux(np.zeros(K, np.complex64), O.diff_mod(pr, O.freq_interleave(O.qpsk_map(bits, K), mode), K))
        x = O.ofdm_generate(z, nsym, K, N).reshape(nsym, N)
        # the bin layout of src/OfdmGenerator.cpp:77-94,207-228: carriers 0 .. K/2-1 on bins 1 .. K/2, the rest on the top K/2
        X = np.zeros((nsym, N), np.complex64)
        zc = z.reshape(nsym, K)
        X[:, 1:K // 2 + 1] = zc[:, :K // 2]
        X[:, N - K // 2:] = zc[:, K // 2:]
        x32 = (np.fft.ifft(X, axis=1) * np.float32(N)).astype(np.complex64)
        assert x32.dtype == np.complex64 and np.fft.ifft(X, axis=1).dtype == np.complex64      # (really single precision)
        e = np.linalg.norm(x32[1:] - x[1:]) / np.linalg.norm(x[1:])
        assert 1e-8 < e < 1e-6, e                                # the same transform, a different rounding
        ya = O.gain_control(x.reshape(-1), N, 2, 1.0, 1.0, 4.0).reshape(nsym, N)
        yb = O.gain_control(x32.reshape(-1), N, 2, 1.0, 1.0, 4.0).reshape(nsym, N)
        for s_ in range(1, nsym):
            xa, xb = x[s_].astype(np.complex128), x32[s_].astype(np.complex128)
            ga = np.vdot(xa, ya[s_].astype(np.complex128)).real / np.vdot(xa, xa).real
            gb = np.vdot(xb, yb[s_].astype(np.complex128)).real / np.vdot(xb, xb).real
            d_rec = max(d_rec, abs(ga / gb - 1.0))
            d_exact = max(d_exact, abs(max(xa.real.std(), xa.imag.std()) / max(xb.real.std(), xb.imag.std()) - 1.0))
    from tests.conftest import record_bound
    record_bound("reference's var-gain recurrence on two correct fp32 transforms of the same carriers, rel, mode %d" % mode,
                 d_rec, 3e-7)
    record_bound("exact variance on the same two, rel, mode %d" % mode, d_exact, 1e-7)
    assert 5e-8 < d_rec < 3e-7, d_rec
    assert d_exact < 1e-7 and d_exact < d_rec, (d_exact, d_rec)


def test_resampler_geometry_x4():
    r = O.Resampler(2048000, 8192000, 2048)       # src/DabModulator.cpp:265-268
    assert (r.L, r.M, r.fft_in, r.fft_out) == (4, 1, 4096, 16384)
    assert r.factor == 2.0 ** -12


def test_chain_equals_stage_by_stage():
    mode = 2
    m = O.mode_params(mode)
    K, N = m["carriers"], m["spacing"]
    bits = np.concatenate([bits_for(mode), synth_bits(O.tf_input_bytes(mode), seed=77)])
    ch = O.Chain(mode=mode, stages=O.STAGE_GAIN | O.STAGE_FIR, normalise=1 / 50000.0)
    out = ch.process(bits)
    assert out.shape == (2, O.tf_samples(mode))
    pr, _ = O.phase_reference(mode)
    for f in range(2):
        b = bits[f * ch.in_bytes_per_tf:(f + 1) * ch.in_bytes_per_tf]
        z = O.signal_mux(np.zeros(K, np.complex64),
                         O.diff_mod(pr, O.freq_interleave(O.qpsk_map(b, K), mode), K))
        t = O.ofdm_generate(z, m["nb_symbols"] + 1, K, N)
        t = O.gain_control(t, N, O.GAIN_VAR, 1.0, 1 / 50000.0, 4.0)
        t = O.guard_interval(t, m["nb_symbols"], N, m["null_size"], m["sym_size"], 0)
        t = O.fir_filter(t, O.fir_default_taps())
        assert np.array_equal(t.view(np.uint32), out[f].view(np.uint32))


def test_oracle_vs_live_reference_on_fresh_random_input():
    """Against the reference's classes live where oracle/_ref is built; everywhere against their outputs on the same
    input, recorded in tests/golden/live_reference.json (make_golden.py)."""
    live = O.have_ref()
    rng = np.random.default_rng(2024)
    mode = 4
    m = O.mode_params(mode)
    K, N = m["carriers"], m["spacing"]
    bits = rng.integers(0, 256, O.tf_input_bytes(mode), dtype=np.uint8)
    q = O.qpsk_map(bits, K)
    assert sha(q) == LIVE["qpsk"]
    assert not live or np.array_equal(q.view(np.uint32), O.ref_qpsk(bits, K).view(np.uint32))
    fi = O.freq_interleave(q, mode)
    assert sha(fi) == LIVE["freq_interleave"]
    assert not live or np.array_equal(fi.view(np.uint32), O.ref_freq_interleave(q, mode).view(np.uint32))
    pr, _ = O.phase_reference(mode)
    dm = O.diff_mod(pr, fi, K)
    assert sha(dm) == LIVE["diff_mod"]
    assert not live or np.array_equal(dm.view(np.uint32), O.ref_diff_mod(pr, fi, K).view(np.uint32))
    t = O.ofdm_generate(O.signal_mux(np.zeros(K, np.complex64), dm), m["nb_symbols"] + 1, K, N)
    for gm in (0, 1, 2):
        a = O.gain_control(t, N, gm, 1.0, 1.0, 4.0)
        assert sha(a) == LIVE["gain_control_%d" % gm]
        assert not live or np.array_equal(a.view(np.uint32), O.ref_gain_control(t, N, gm, 1.0, 1.0, 4.0).view(np.uint32))


def test_oracle_chain_decodes_through_an_independent_receiver():
    """The oracle's FFT-based stages have no reference run behind them (FFTW is not in the image): an independent
    check of their orientation, bin layout and timing -- the oracle's Mode-I frames decode bit for bit through a
    receiver written from the standard.  cfg 2, cfg 3 (FIR: window 44 samples early) and cfg 4 as a stream (every
    4th sample, one hop of delay)."""
    rs = np.random.RandomState(11)
    bits = np.frombuffer(rs.bytes(2 * 28800), np.uint8).reshape(2, 28800)
    y = O.Chain(mode=1, stages=0).process(bits[:1])
    assert np.array_equal(dab_demodulate_mode1(y[0]), bits[0])
    y = O.Chain(mode=1, stages=3, gain_mode=2, normalise=1.0 / 50000.0).process(bits[:1])
    assert np.array_equal(dab_demodulate_mode1(y[0], 44), bits[0])
    y = O.Chain(mode=1, stages=15, gain_mode=2, normalise=1.0 / 50000.0, out_rate=8192000, am=POLY_AM, pm=POLY_PM,
                fast=True).process(bits[:2])
    stream = y.reshape(-1)[4 * 2048::4]
    assert np.array_equal(dab_demodulate_mode1(stream[:196608], 44), bits[0])


FAKE_FFTW = r"""
/* test double of libfftw3f.so.3: the three entry points the baseline build looks up, over a plain float64 DFT */
#include <math.h>
#include <stdlib.h>
typedef float cpx[2];
typedef struct { int n, sign; } plan;
void *fftwf_plan_dft_1d(int n, cpx *in, cpx *out, int sign, unsigned flags)
{
    (void)in; (void)out; (void)flags;
    plan *p = malloc(sizeof *p);
    p->n = n; p->sign = sign;
    return p;
}
void fftwf_execute_dft(void *pp, cpx *in, cpx *out)
{
    const plan *p = pp;
    const int n = p->n;
    /* radix-2 decimation in time, float64, recursion-free: bit-reversed copy, then butterflies */
    double *re = malloc(sizeof(double) * n), *im = malloc(sizeof(double) * n);
    int lg = 0;
    while ((1 << lg) < n) ++lg;
    for (int i = 0; i < n; ++i) {
        int r = 0;
        for (int b = 0; b < lg; ++b) r |= ((i >> b) & 1) << (lg - 1 - b);
        re[r] = in[i][0]; im[r] = in[i][1];
    }
    for (int len = 2; len <= n; len <<= 1) {
        const double ang = (p->sign > 0 ? 2.0 : -2.0) * M_PI / len;
        for (int i = 0; i < n; i += len)
            for (int k = 0; k < len / 2; ++k) {
                const double wr = cos(ang * k), wi = sin(ang * k);
                const int a = i + k, b = i + k + len / 2;
                const double tr = re[b] * wr - im[b] * wi, ti = re[b] * wi + im[b] * wr;
                re[b] = re[a] - tr; im[b] = im[a] - ti;
                re[a] += tr; im[a] += ti;
            }
    }
    for (int i = 0; i < n; ++i) { out[i][0] = (float)re[i]; out[i][1] = (float)im[i]; }
    free(re); free(im);
}
"""


def test_cpu_baseline_build_picks_up_fftw3f_when_the_host_has_it(tmp_path):
    """bench.py's CPU baseline runs on FFTW3f -- the reference's own transform library (src/OfdmGenerator.cpp:106-117)
    -- when libfftw3f.so.3 is present, and says which engine it used.  The image has no FFTW, so the run-time lookup is
    exercised against a test double on LD_LIBRARY_PATH: same frames within the float tolerance, engine reported."""
    import json
    import subprocess
    import sys
    src = tmp_path / "fake_fftw.c"
    src.write_text(FAKE_FFTW)
    subprocess.check_call(["gcc", "-O2", "-shared", "-fPIC", "-o", str(tmp_path / "libfftw3f.so.3"), str(src), "-lm"])
    code = ("import sys, json, numpy as np; sys.path.insert(0, %r); import oracle as O\n"
            "from tests.golden.synth import synth_bits\n"
            "bits = synth_bits(28800, seed=77).reshape(1, -1)\n"
            "y = O.Chain(mode=1, stages=15, gain_mode=2, normalise=1 / 50000., out_rate=8192000, fast=True).process(bits)\n"
            "np.save(sys.argv[1], y); print(json.dumps({'engine': O.fft_engine()}))\n" % ROOT)
    res = {}
    for name, env in (("fftw", {"LD_LIBRARY_PATH": str(tmp_path)}), ("port", {"DABO_FFTW": "0", "LD_LIBRARY_PATH": str(tmp_path)}),
                      ("absent", {})):
        out = str(tmp_path / (name + ".npy"))
        r = subprocess.run([sys.executable, "-c", code, out], env=dict(os.environ, **env), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        res[name] = (json.loads(r.stdout.strip().splitlines()[-1])["engine"], np.load(out))
    assert res["fftw"][0] == "fftw3f" and res["port"][0] == "port" and res["absent"][0] == "port"
    a, b = res["fftw"][1], res["port"][1]
    assert np.linalg.norm(a - b) / np.linalg.norm(b) < 1e-6
    assert np.array_equal(res["port"][1], res["absent"][1])
