"""The channel emulator without a device: the float64 model (tests/channel_model.py, written from include/dabgpu.h) reproduces
Philox's known answers, its noise is Gaussian to five standard errors, a chunked stream equals the unchunked one exactly; the
settings' refusals are host code alone; the operating point of the soft loop and the margins of the captures that the GPU
tests rely on are found here, on the models."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import channel_cases as CC
from tests import channel_model as CM
from tests import decode_model as M
from tests import soft_cases as SC
from tests import soft_model as S
from tests.conftest import ROOT, load_pkg
from tests.demod_model import demod_model
from tests.receiver import dab_demodulate
from tests.sync_model import extract_model, extract_slots, geometry, sync_model

ENTRIES = ["dabgpu_channel_check", "dabgpu_set_channel", "dabgpu_channel_reset", "dabgpu_get_channel_position",
           "dabgpu_channel_dev", "dabgpu_channel", "dabgpu_debug_channel_run_samples"]


def test_header_library_and_exports_are_in_step():
    pkg = load_pkg()
    text = open(os.path.join(ROOT, "include", "dabgpu.h")).read()
    lib = pkg.load_library()
    for name in ENTRIES:
        assert re.search(r"DABGPU_API int %s\(" % name, text), name
        assert name in pkg.EXPORTS and hasattr(lib, name), name
    assert "#define DABGPU_CH_MAX_PATHS 64" in text and "#define DABGPU_CH_MAX_DELAY 2047" in text
    assert (pkg.CH_MAX_PATHS, pkg.CH_MAX_DELAY) == (CM.MAX_PATHS, CM.MAX_DELAY) == (64, 2047)
    assert C.sizeof(pkg._ChannelPath) == 24 and C.sizeof(pkg._ChannelConfig) == 24 + 64 * 24
    for words in ("sqrt(48 ln 2) = 5.77", "Fractional-sample delays".lower(), "sampling-clock offset", "Philox4x32-10"):
        assert words in text, words
    for m in ("set_channel", "channel_reset", "channel_position", "channel", "channel_dev"):
        assert callable(getattr(pkg.Modulator, m)), m
    for f in ("channel_check", "channel_sigma", "rayleigh_paths"):
        assert callable(getattr(pkg, f)), f


# --------------------------------------------------------------------------- 1. Philox known answers
@pytest.mark.parametrize("counter,key,want", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_answers(counter, key, want):
    w = CM.philox4x32_10(counter, key)
    assert " ".join("%08x" % int(v[0]) for v in w) == want


# --------------------------------------------------------------------------- 2. the noise of the model
def test_model_noise_is_gaussian_to_five_standard_errors():
    n = 1 << 21
    z = CM.unit_noise(3, 0, n)
    re, im = z.real, z.imag
    figures = dict(mean_re=re.mean(), mean_im=im.mean(), var_re=re.var(), var_im=im.var(), cross=(re * im).mean(),
                   lag1_re=(re[1:] * re[:-1]).mean() / re.var(), lag1_im=(im[1:] * im[:-1]).mean() / im.var(),
                   kurt_re=(re ** 4).mean() / re.var() ** 2, kurt_im=(im ** 4).mean() / im.var() ** 2,
                   largest=max(np.abs(re).max(), np.abs(im).max()))
    print(figures)
    se = 5.0 / np.sqrt(n)
    assert abs(figures["mean_re"]) <= se and abs(figures["mean_im"]) <= se
    assert abs(figures["var_re"] - 1.0) <= 5.0 * np.sqrt(2.0 / n) and abs(figures["var_im"] - 1.0) <= 5.0 * np.sqrt(2.0 / n)
    assert abs(figures["cross"]) <= se
    assert abs(figures["lag1_re"]) <= se and abs(figures["lag1_im"]) <= se
    assert abs(figures["kurt_re"] - 3.0) <= 5.0 * np.sqrt(24.0 / n) and abs(figures["kurt_im"] - 3.0) <= 5.0 * np.sqrt(24.0 / n)
    assert figures["largest"] <= 5.77
    # a sample's noise belongs to its absolute index: any window of the stream is the same numbers
    assert np.array_equal(CM.unit_noise(3, 1001, 64), z[1001:1065])
    assert not np.array_equal(CM.unit_noise(3 + (1 << 32), 0, 64), z[:64])         # (the seed's upper half is in the key)


# --------------------------------------------------------------------------- 3. chunking and reset, on the model
def _run(ch, x, lengths, position):
    ch.reset(position)
    out, at = [], 0
    for m in lengths:
        out.append(ch(x[2 * at:2 * (at + m)] if x.dtype == np.int16 else x[at:at + m]))
        at += m
    assert at == CM.as_samples(x).size
    return np.concatenate(out)


def test_model_chunked_equals_unchunked_and_a_reset_equals_the_tail_of_a_zero_padded_run():
    x = CC.signal(CC.N_STREAM, 2)
    ch = CM.Channel(CC.EVERYTHING, 0.1, CC.SEED64)
    whole = _run(ch, x, [CC.N_STREAM], CC.STREAM_POSITION)
    assert np.abs(whole).min() > 0
    for name, lengths in CC.splits().items():
        assert np.array_equal(_run(ch, x, lengths, CC.STREAM_POSITION), whole), name
    q = CC.signal(CC.N_STREAM, 3, s16=True)
    want = _run(ch, q, [CC.N_STREAM], CC.STREAM_POSITION)
    assert np.array_equal(_run(ch, CM.as_samples(q).astype(np.complex64), CC.splits()["sevens"], CC.STREAM_POSITION), want)
    # a reset at P = the tail of a run from 0 whose input is zeros up to P
    P = 5000
    padded = _run(ch, np.concatenate([np.zeros(P, np.complex64), x]), [P + CC.N_STREAM], 0)
    assert np.array_equal(_run(ch, x, [CC.N_STREAM], P), padded[P:])
    # the history is the last 2047 inputs: a delayed path alone reproduces them
    d = CM.Channel([(2047, 1.0, 0.0)])
    d(x[:3000])
    assert np.array_equal(d(x[3000:3010]), x[953:963].astype(np.complex128))


# --------------------------------------------------------------------------- 4. the settings' refusals, host code alone
REFUSALS = [
    ("delay", dict(paths=[(0, 1.0, 0.0), (2048, 1.0, 0.0)]), "delay is 0 ... 2047"),
    ("gain_inf", dict(paths=[(0, complex(np.inf, 0.0), 0.0)]), "finite"),
    ("gain_nan", dict(paths=[(0, complex(0.0, np.nan), 0.0)]), "finite"),
    ("sigma_nan", dict(paths=[], sigma=np.nan), "finite"),
    ("sigma_inf", dict(paths=[], sigma=np.inf), "finite"),
    ("sigma_negative", dict(paths=[], sigma=-1e-3), "sigma must not be negative"),
    ("rate_zero", dict(paths=[], rate_hz=0.0), "rate_hz must be positive"),
    ("rate_negative", dict(paths=[], rate_hz=-2048000.0), "rate_hz must be positive"),
    ("doppler_half", dict(paths=[(0, 1.0, 1024000.0)]), "below rate_hz / 2"),
    ("doppler_minus_half", dict(paths=[(0, 1.0, -1024000.0)]), "below rate_hz / 2"),
    ("doppler_nan", dict(paths=[(0, 1.0, np.nan)]), "below rate_hz / 2"),
    ("doppler_other_rate", dict(paths=[(0, 1.0, 600000.0)], rate_hz=1200000.0), "below rate_hz / 2"),
    ("paths65", dict(paths=[(0, 1.0, 0.0)] * 65), "at most 64 paths"),
]


@pytest.mark.parametrize("name,kw,message", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_channel_check_refuses_with_its_message(name, kw, message):
    pkg = load_pkg()
    with pytest.raises(pkg.DabGpuError) as e:
        pkg.channel_check(**kw)
    assert message in str(e.value) and str(e.value).startswith("channel:")


def test_channel_check_accepts_the_documented_ranges_and_the_c_entry_counts_the_paths_itself():
    pkg = load_pkg()
    lib = pkg.load_library()
    pkg.channel_check([])
    pkg.channel_check([(2047, 1e30 + 0j, 1023999.0), (0, 0.0, -1023999.0)] * 32, sigma=0.0, seed=2 ** 64 - 1)
    pkg.channel_check([(0, 1.0, 4000000.0)], sigma=3.0, rate_hz=8192000.0)
    for name in CC.KERNEL_CASES:
        c = CC.kernel_case(name)
        pkg.channel_check(c["paths"], c["sigma"], c["seed"], c["rate_hz"])
    cfg = pkg._ChannelConfig()
    cfg.n_paths, cfg.rate_hz = 65, 2048000.0
    assert lib.dabgpu_channel_check(C.byref(cfg)) != 0 and b"at most 64 paths" in lib.dabgpu_last_error(None)
    cfg.n_paths = 64
    assert lib.dabgpu_channel_check(C.byref(cfg)) == 0
    assert lib.dabgpu_channel_check(None) != 0 and b"null argument" in lib.dabgpu_last_error(None)
    assert abs(pkg.channel_sigma(2.0, 10.0) - np.sqrt(2.0 / 10.0 / 2.0)) < 1e-15


def test_rayleigh_paths_are_well_formed_sum_to_the_profile_and_repeat():
    pkg = load_pkg()
    delays, powers = [0, 30, 200, 2047], [0.0, -3.0, -6.0, -9.0]
    paths = pkg.rayleigh_paths(delays, powers, 80.0, 16, seed=5)
    assert len(paths) == 64 and paths == pkg.rayleigh_paths(delays, powers, 80.0, 16, seed=5)
    assert paths != pkg.rayleigh_paths(delays, powers, 80.0, 16, seed=6)
    pkg.channel_check(paths)
    for i, (d, p_db) in enumerate(zip(delays, powers)):
        mine = paths[16 * i:16 * (i + 1)]
        assert all(q[0] == d and abs(q[2]) <= 80.0 for q in mine)
        assert len({round(abs(q[1]), 12) for q in mine}) == 1                      # equal power
        assert abs(sum(abs(q[1]) ** 2 for q in mine) - 10.0 ** (p_db / 10.0)) < 1e-12
        assert len({q[2] for q in mine}) == 16
    with pytest.raises(pkg.DabGpuError):
        pkg.rayleigh_paths(delays, powers, 80.0, 17, seed=5)
    with pytest.raises(pkg.DabGpuError):
        pkg.rayleigh_paths(delays, powers[:3], 80.0, 4, seed=5)


# --------------------------------------------------------------------------- 5. the operating point of GPU test 7
def test_operating_point_with_the_channels_noise():
    """tests/test_soft_cpu.py's search with the channel model's noise in place of add_noise: C/N downwards in 0.5 dB steps; L =
    the highest level at which the hard path has a payload bit error in every returned frame; the first seed for which the
    soft path has none at L and 1 dB below is the one channel_cases records."""
    import oracle as O
    pkg = load_pkg()
    eti, bits, ref = SC.op_stream()
    layout = pkg.Modulator.frontend_describe(eti[0])
    y = np.asarray(O.Chain(mode=SC.OP_MODE, stages=3, gain_mode=2, normalise=SC.NORMALISE).process(bits)).reshape(SC.OP_FRAMES, -1)
    power = CC.data_power(y, SC.OP_MODE)

    def paths(cn, seed):
        ch = CM.Channel([(0, 1.0, 0.0)], pkg.channel_sigma(power, cn), seed)
        yn = ch(y.reshape(-1)).reshape(y.shape)
        hard = np.stack([demod_model(f, SC.OP_MODE, SC.OP_EARLY)["bits"] for f in yn])
        soft = np.stack([S.demod_soft_model(f, SC.OP_MODE, SC.OP_EARLY) for f in yn])
        return (SC.frame_errors(M.decode_stream(layout, hard, ref)[1]), SC.frame_errors(S.decode_soft_stream(layout, soft, ref)[1]))

    found = None
    for seed in CC.OP_SEEDS_TRIED:
        level = None
        for cn in np.arange(SC.OP_START_DB, SC.OP_STOP_DB - 1e-9, -SC.OP_STEP_DB):
            hard, soft = paths(cn, seed)
            if all(e > 0 for e in hard):
                level = float(cn)
                break
        assert level is not None, seed
        at = [paths(level - back, seed) for back in (0.0, 1.0)]
        print("seed %d: L = %.1f dB, hard %s / %s, soft %s / %s" % (seed, level, at[0][0], at[1][0], at[0][1], at[1][1]))
        if not any(at[0][1]) and not any(at[1][1]):
            found = (seed, level)
            break
    assert found == (CC.OP_SEED, CC.OP_LEVEL_DB)
    recorded = open(os.path.join(ROOT, "profiles", "channel.txt")).read()
    assert re.search(r"operating point: seed %d, L = %.1f dB" % found, recorded)


# --------------------------------------------------------------------------- 6. the captures of GPU test 8 are safe
@pytest.mark.parametrize("name", sorted(CC.CAPTURES))
def test_the_captures_meet_the_synchronisers_conditions_on_the_channel_models_output(name):
    """tests/test_sync_cpu.py's conditions, with its bars, on the channel model's output: the frames are found at the first
    path and decode to the input bits."""
    pkg = load_pkg()
    x, mode, bits, _ = CC.capture_input(name)
    early = CC.CAPTURES[name][9]
    g = geometry(mode)
    lead = CC.CAPTURES[name][3]
    paths, sigma, seed = CC.capture_channel(name, pkg.channel_sigma)
    y = CM.Channel(paths, sigma, seed)(x)
    r = sync_model(y, mode, 31, 2)
    assert r["n_frames"] == 2, r
    print("%s: coarse0 %d, null_depth %.3g, S second/lowest %.3g / %.3g" % (name, r["coarse0"], r["null_depth"], r["s_second"], r["s_lowest"]))
    assert r["s_second"] >= 1.5 * r["s_lowest"]
    for k, (fr, mg) in enumerate(zip(r["frames"], r["margins"])):
        true = lead + k * g["tf"]
        print("  frame %d: start %d (true %d) shift %d eps %+.6f quality %.4f, runner-up D %.3g c %.3g"
              % (k, fr["start"], true, fr["shift"], fr["eps"], fr["quality"], mg["d_runner_up"], mg["c_runner_up"]))
        if name in CC.CFG3_CAPTURES:
            assert abs(fr["start"] - true) <= 44
        else:
            assert fr["start"] == true
        assert fr["valid"] == 1
        assert abs(fr["shift"] + fr["eps"] - CC.CFO) <= 1e-3
        assert mg["d_runner_up"] <= 0.5 and mg["c_runner_up"] <= 0.5
        assert abs(fr["eps"]) <= 0.45
    frames = extract_model(y, mode, r["frames"], extract_slots(y.size, mode, 2))
    for k in range(2):
        assert np.array_equal(dab_demodulate(frames[k], mode, early), bits[k]), (name, k)
