"""The carrier state on the device (include/dabgpu.h, "the carrier state"): integer sums and weights equal to
the float64 / integer model (tests/csi_model.py), weighted softs within one step of it, byte equality over run geometry, repetition, batch and input
format, every transform size with an interferer on lane 0's DC-bin exception, unit weights against demod_soft, the hard call's
bits and figures, refusals, lane ordering, and the loop at the operating point behind a tone that tests/test_csi_cpu.py found."""
import numpy as np
import pytest

from tests import channel_cases as CC
from tests import csi_cases as XC
from tests import csi_model as X
from tests import decode_model as M
from tests import soft_cases as SC
from tests.conftest import record_bound
from tests.receiver import MODES

pytestmark = pytest.mark.gpu
G, F = 1, 2
EARLY = 5
BAR_SIGNAL, BAR_QUADRATURE = 4 * 1.036e-7, 4 * 1.128e-7          # tests/test_demod_gpu.py: the float sums repeat to these

# ---- what the fp32 soft pass may differ by from the float64 model (the state pass is float64 and is held to the model exactly).
# TRANSFORM: the fp32 transform and the product z_s conj(z_(s-1)) against float64, relative to the RMS of u over the symbol
# (64 sqrt(2)): conftest.int_off_by_one_limit takes 5e-7 for one transform of a chain; d is a product of two transformed values.
TRANSFORM = 2 * 5e-7
U_RMS = 64.0 * np.sqrt(2.0)
EPS = 2.0 ** -24                                                # half an ulp of fp32, relative


def _frames(mode, n=1, cn_db=10.0, spurs=True):
    """n noisy frames of `mode` as complex64; with spurs an unmodulated carrier 15 dB above a data carrier on position K/2 - 1
    (bin K/2 = 3 T: lane 0's first carrier, the slot the DC bin would have had) and on position 7"""
    K = MODES[mode][1]
    return np.stack([XC.random_frame(mode, 100 * mode + f, cn_db, (K // 2 - 1, 7) if spurs else (), 15.0) for f in range(n)]).astype(np.complex64)


@pytest.fixture(scope="module")
def mods(pkg):
    ms = {m: pkg.Modulator(mode=m, max_frames=3) for m in (1, 2, 3, 4)}
    yield ms
    for m in ms.values():
        m.close()


def _ulp_apart(a, b):
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def _check_weights(A, V, w, what):
    """The device's weights against the model's rule on the device's own integer sums: the same fp32 bits.  Every operation
    of the rule is a single IEEE float64 operation; the one a GPU may not round correctly is the division."""
    want = X.weights(A, V)
    apart = _ulp_apart(w, want)
    print("%s: weights %.4g ... %.4g, %d of %d differ from the model's bits, at most %d ulp" % (what, w.min(), w.max(), (apart > 0).sum(), w.size, apart.max()))
    assert apart.max() <= 1, "weights more than one ulp from the model"
    assert apart.max() == 0, "the float64 division (A SV) / (SA max(V, floor)) is not correctly rounded on the device"


# --------------------------------------------------------------------------- 1. against the model, every transform size
@pytest.mark.parametrize("mode,n", [(3, 2), (2, 1), (4, 1), (1, 1)])
def test_sums_weights_and_softs_follow_the_model_with_a_spur_on_lane_zeros_first_carrier(mods, mode, n):
    md = mods[mode]
    K = MODES[mode][1]
    iq = _frames(mode, n)
    md.set_csi_unit_weights(False)
    md.set_demod_run_symbols(0)
    soft, bits = md.demod_csi(iq, early=EARLY, want_bits=True)
    stats = [md.monitor_stats(f) for f in range(n)]
    shares = []
    for f in range(n):
        st = md.carrier_state(f)
        m = X.demod_csi_model(iq[f], mode, EARLY)
        # the state pass runs in float64 from the samples on: the sums are the model's, count for count
        ea, ev = np.abs(st["A"] - m["A"]), np.abs(st["V"] - m["V"])
        print("mode %d frame %d: A differs on %d carriers, V on %d" % (mode, f, (ea > 0).sum(), (ev > 0).sum()))
        assert np.array_equal(st["A"], m["A"]) and np.array_equal(st["V"], m["V"])
        assert np.array_equal(st["w"].view(np.int32), m["w"].view(np.int32))
        # the spur on lane 0's first carrier (position K/2 - 1, bin 3 T) and on position 7: V far above the rest, weight near 0
        rest = np.delete(st["w"], [K // 2 - 1, 7])
        assert 0.3 < rest.min() and rest.max() < 3.0
        for k in (K // 2 - 1, 7):
            assert st["V"][k] > 100 * np.median(st["V"]) and st["w"][k] < 0.25 * rest.min(), k
        _check_weights(st["A"], st["V"], st["w"], "mode %d frame %d" % (mode, f))
        # the per-carrier MER of the header, from the device's sums
        assert np.allclose(st["mer_db"], X.mer_db(st["A"], st["V"], mode))
        # softs: one step at the most, and only where the exact value lies within the fp32 error of a rounding boundary.  The
        # weights are the model's bits; the error of x = -Re u w in steps is the fp32 transform's on u (TRANSFORM U_RMS w) and
        # the fp32 roundings of d, q, u and the product (4 EPS |x|).  A value lands on the other side of a boundary with the
        # probability of that error in steps; 2.5 times the expectation is the bar, as conftest.int_off_by_one_limit sets it.
        want = m["soft"].astype(np.int64)
        exact = X.softs_of(m["u"], m["w"], mode, exact=True)
        inside = np.abs(exact) < 127
        rel = 4 * EPS
        limit = 2.5 * (TRANSFORM * U_RMS * float(np.mean(m["w"])) + rel * float(np.mean(np.abs(exact[inside]))))
        diff = np.abs(soft[f].astype(np.int64) - want)
        share = float((diff == 1).mean())
        print("mode %d frame %d: %d of %d softs one step from the model (share %.3g, bar %.3g), worst %d" % (mode, f, (diff == 1).sum(), diff.size, share, limit, diff.max()))
        assert diff.max() <= 1
        assert record_bound("demod_csi share one step from the float64 model, mode %d frame %d" % (mode, f), share, limit)
        shares.append(share)
        assert len(np.unique(want)) > 100
    # the hard call's bits and per-frame figures
    hard = md.demod(iq, early=EARLY)
    assert np.array_equal(bits, hard)
    for f in range(n):
        a, b = stats[f], md.monitor_stats(f)
        assert (a["bit_errors"], a["n_bits"], a["min_margin"]) == (b["bit_errors"], b["n_bits"], b["min_margin"])
        assert abs(a["sum_signal"] / b["sum_signal"] - 1.0) <= BAR_SIGNAL and abs(a["sum_quadrature"] / b["sum_quadrature"] - 1.0) <= BAR_QUADRATURE


def test_integer_sums_and_weights_equal_the_float64_model_exactly(mods):
    """A and V equal to the float64 model count for count, the weights bit for bit, from the state-only call (host path), on a
    frame of its own: Mode III, one frame, run length 7.  The state pass is float64 from the samples on (demod.hip,
    demod_csi_state_kernel): against numpy's float64 transform a term of 4e6 counts lies 1e-8 counts off, so a rounding
    boundary is crossed once in 1e8 terms; the frame has 58 368."""
    md = mods[3]
    iq = _frames(3, 1)
    md.set_csi_unit_weights(False)
    md.set_demod_run_symbols(7)
    md.demod_carrier_state(iq, early=EARLY)
    md.set_demod_run_symbols(0)
    st = md.carrier_state(0)
    m = X.demod_csi_model(iq[0], 3, EARLY)
    print("A: %d of %d carriers differ, at most %d counts; V: %d differ, at most %d counts; weights: %d differ, at most %d ulp"
          % ((st["A"] != m["A"]).sum(), m["A"].size, np.abs(st["A"] - m["A"]).max(), (st["V"] != m["V"]).sum(),
             np.abs(st["V"] - m["V"]).max(), (_ulp_apart(st["w"], m["w"]) > 0).sum(), _ulp_apart(st["w"], m["w"]).max()))
    assert np.array_equal(st["A"], m["A"]) and np.array_equal(st["V"], m["V"])
    assert np.array_equal(st["w"].view(np.int32), m["w"].view(np.int32))


# --------------------------------------------------------------------------- 2. the same bytes
@pytest.mark.parametrize("mode", [3, 1])
def test_state_weights_and_softs_are_the_same_bytes_for_every_geometry_repetition_batch_and_format(mods, mode):
    md = mods[mode]
    nblocks = MODES[mode][2] - 1
    md.set_csi_unit_weights(False)
    # values that are exact as s16: the frame scaled to 2000 RMS and rounded
    ints = np.rint(_frames(mode, 3).astype(np.complex128) * 2000.0)
    s16 = np.stack([ints.real, ints.imag], axis=-1).astype(np.int16).reshape(3, -1)
    cf = ints.astype(np.complex64)

    def run(x, frames):
        soft = md.demod_csi(x, early=EARLY)
        return [(soft[i].tobytes(),) + tuple(md.carrier_state(i)[k].tobytes() for k in ("A", "V", "w")) for i in frames]

    try:
        first = run(cf[1:2], [0])[0]
        assert len(set(first[0])) > 100
        assert run(cf[1:2], [0])[0] == first                           # a repetition
        for spr in (1, 4, 7, nblocks):
            md.set_demod_run_symbols(spr)
            assert run(cf[1:2], [0])[0] == first, spr
            md.demod_carrier_state(cf[1:2], early=EARLY)               # the state alone: the same state
            assert tuple(md.carrier_state(0)[k].tobytes() for k in ("A", "V", "w")) == first[1:], spr
        md.set_demod_run_symbols(0)
        batch = run(cf, [0, 1, 2])
        assert batch[1] == first and batch[0] != first and batch[2] != first      # inside a batch of three
        md.set_demod_run_symbols(7)
        assert run(cf, [1])[0] == first
        md.set_demod_run_symbols(0)
        assert run(s16[1:2], [0])[0] == first                          # s16 input with the same values
        assert run(s16, [0, 1, 2]) == batch
    finally:
        md.set_demod_run_symbols(0)


def test_unit_weights_give_demod_softs_bytes_and_the_state_alone_leaves_the_figures(mods):
    md = mods[2]
    iq = _frames(2, 2)
    try:
        md.set_csi_unit_weights(False)
        weighted = md.demod_csi(iq, early=EARLY)
        state = [md.carrier_state(f) for f in range(2)]
        plain = md.demod_soft(iq, early=EARLY)
        assert not np.array_equal(weighted, plain)
        md.set_csi_unit_weights(True)
        assert np.array_equal(md.demod_csi(iq, early=EARLY), plain)
        for f in range(2):
            st = md.carrier_state(f)
            assert (st["w"] == 1).all() and np.array_equal(st["A"], state[f]["A"]) and np.array_equal(st["V"], state[f]["V"])
        md.set_csi_unit_weights(False)
        # the state alone, on the device path: the same state, and the per-frame figures stay the call's before
        import torch
        md.demod(iq[:1], early=EARLY, ref_bits=np.zeros(md.geometry["tf_input_bytes"], np.uint8))
        before = md.monitor_stats(0)
        d_iq = torch.from_numpy(iq).cuda()
        md.demod_carrier_state_dev(d_iq, 2, EARLY)
        for f in range(2):
            st = md.carrier_state(f)
            assert all(np.array_equal(st[k], state[f][k]) for k in ("A", "V", "w"))
        assert md.monitor_stats(0) == before and before["n_bits"] > 0
        # a clean frame (no noise: every quadrature term rounds to 0 or nearly) and an all-zero frame: finite weights, repeated
        clean = _frames(2, 1, cn_db=400.0, spurs=False)
        a = md.demod_csi(clean, early=EARLY)
        wa = md.carrier_state(0)["w"]
        assert np.isfinite(wa).all() and (wa >= 0).all() and (wa <= X.MAX_WEIGHT).all()
        assert np.array_equal(md.demod_csi(clean, early=EARLY), a) and np.array_equal(md.carrier_state(0)["w"], wa)
        zero = md.demod_csi(np.zeros_like(clean), early=EARLY)
        st = md.carrier_state(0)
        assert not zero.any() and not st["A"].any() and not st["V"].any() and (st["w"] == 1).all()
    finally:
        md.set_csi_unit_weights(False)


# --------------------------------------------------------------------------- 3. refusals
def test_refusals_come_before_anything_is_queued_and_leave_outputs_and_state_alone(pkg):
    import torch
    md = pkg.Modulator(mode=3, max_frames=2)
    try:
        g = md.geometry
        lib, h = md._lib, md._h
        with pytest.raises(pkg.DabGpuError, match="no carrier state"):
            md.carrier_state(0)
        iq = _frames(3, 1)
        d_y = torch.from_numpy(iq[0]).cuda()
        d_soft = torch.full((8 * g["tf_input_bytes"],), 5, dtype=torch.int8, device="cuda")
        d_bits = torch.full((g["tf_input_bytes"],), 7, dtype=torch.uint8, device="cuda")
        md.demod_csi_dev(d_y, 1, d_soft, EARLY, d_bits)
        good = (d_soft.cpu().numpy().copy(), d_bits.cpu().numpy().copy(), md.carrier_state(0), md.monitor_stats(0))
        d_soft.fill_(5)
        d_bits.fill_(7)
        INVALID = -1
        p, s, b = d_y.data_ptr(), d_soft.data_ptr(), d_bits.data_ptr()
        for bad in (-1, 64):                                           # early outside the cyclic prefix (63 samples)
            assert lib.dabgpu_demod_csi_dev(h, p, 0, 1, bad, s, b, None, None) == INVALID
            assert lib.dabgpu_demod_carrier_state_dev(h, p, 0, 1, bad, None) == INVALID
            with pytest.raises(pkg.DabGpuError, match="cyclic prefix"):
                md.demod_csi_dev(d_y, 1, d_soft, bad)
        for fmt in (2, 3):                                             # u8 / s8
            assert lib.dabgpu_demod_csi_dev(h, p, fmt, 1, EARLY, s, b, None, None) == INVALID
            assert lib.dabgpu_demod_carrier_state_dev(h, p, fmt, 1, EARLY, None) == INVALID
        with pytest.raises(pkg.DabGpuError):
            md.demod_csi(np.zeros(2 * g["tf_samples"], np.int8))
        assert lib.dabgpu_demod_csi_dev(h, None, 0, 1, EARLY, s, b, None, None) == INVALID       # null pointers
        assert lib.dabgpu_demod_csi_dev(h, p, 0, 1, EARLY, None, b, None, None) == INVALID
        assert lib.dabgpu_demod_carrier_state_dev(h, None, 0, 1, EARLY, None) == INVALID
        for args in ((p + 2, s, b, None), (p, s + 1, b, None), (p, s, b + 2, None), (p, s, b, b + 1)):      # misaligned
            assert lib.dabgpu_demod_csi_dev(h, args[0], 0, 1, EARLY, args[1], args[2], args[3], None) == INVALID
        assert lib.dabgpu_demod_carrier_state_dev(h, p + 2, 0, 1, EARLY, None) == INVALID
        with pytest.raises(pkg.DabGpuError, match="max_frames"):
            md.demod_csi(np.zeros(3 * g["tf_samples"], np.complex64))
        with pytest.raises(pkg.DabGpuError, match="soft buffer"):
            md.demod_csi_dev(d_y, 1, d_soft[:-8])
        with pytest.raises(pkg.DabGpuError, match="no carrier state"):
            md.carrier_state(1)                                        # a frame beyond the call
        K = g["carriers"]
        buf = np.zeros(K, np.int64)
        assert lib.dabgpu_get_carrier_state(h, 1, buf.ctypes.data, None, None) == INVALID and not buf.any()
        md.synchronize()
        # nothing was written, and the state and the figures are the good call's
        assert (d_soft.cpu().numpy() == 5).all() and (d_bits.cpu().numpy() == 7).all()
        st = md.carrier_state(0)
        assert all(np.array_equal(st[k], good[2][k]) for k in ("A", "V", "w")) and md.monitor_stats(0) == good[3]
        md.demod_csi_dev(d_y, 1, d_soft, EARLY, d_bits)
        assert np.array_equal(d_soft.cpu().numpy(), good[0]) and np.array_equal(d_bits.cpu().numpy(), good[1])
    finally:
        md.close()


# --------------------------------------------------------------------------- 4. behind the lanes
def test_a_queued_weighted_call_waits_for_the_chain_call_on_a_lane(pkg):
    """Three chain calls queued on the context's own stream go over the three lanes, each writing a capture of its own; behind
    each, without a wait, demod_csi_dev with stream = NULL on that capture; at the end demod_carrier_state_dev on the last.
    Softs and state are the bytes of the serial order (every step waited for)."""
    import torch
    from tests import demod_cases as DC
    mode, n = 2, 2
    md = pkg.Modulator(mode=mode, max_frames=n)
    try:
        md.set_lanes(3)
        per = md.geometry["tf_input_bytes"]
        d_in = [torch.from_numpy(DC.case_bits(mode, n, per) ^ np.uint8(17 * i)).cuda() for i in range(3)]
        d_iq = [torch.zeros((n, md.geometry["tf_samples"]), dtype=torch.complex64, device="cuda") for _ in range(3)]
        d_soft = [torch.zeros((n, 8 * per), dtype=torch.int8, device="cuda") for _ in range(3)]
        want = []
        for i in range(3):                                             # serial
            md.chain_dev(d_in[i], n, 0, d_iq[i])
            md.demod_csi_dev(d_iq[i], n, d_soft[i], 0)
            want.append((d_soft[i].cpu().numpy().copy(), [md.carrier_state(f) for f in range(n)]))
            assert want[i][0].any() and (i == 0 or not np.array_equal(want[i][0], want[0][0]))
            d_soft[i].zero_()
            d_iq[i].zero_()
        torch.cuda.synchronize()
        for i in range(3):
            md.chain_dev_queued(d_in[i], n, 0, d_iq[i])
            md.demod_csi_dev(d_iq[i], n, d_soft[i], 0, queued=True)
        md.synchronize()
        assert md.lanes_info()[0] == 3
        for i in range(3):
            assert np.array_equal(d_soft[i].cpu().numpy(), want[i][0]), i
        for f in range(n):
            st = md.carrier_state(f)
            assert all(np.array_equal(st[k], want[2][1][f][k]) for k in ("A", "V", "w"))
        d_iq[1].zero_()
        torch.cuda.synchronize()
        md.chain_dev_queued(d_in[0], n, 0, d_iq[0])
        md.chain_dev_queued(d_in[1], n, 0, d_iq[1])
        md.demod_carrier_state_dev(d_iq[1], n, 0, queued=True)
        st = md.carrier_state(1)                                       # (waits for the call)
        assert all(np.array_equal(st[k], want[1][1][1][k]) for k in ("A", "V", "w"))
        md.synchronize()
    finally:
        md.close()


# --------------------------------------------------------------------------- 5. the loop at the operating point
def test_at_the_operating_point_the_weighted_loop_decodes_what_the_unweighted_loop_loses(pkg):
    """ETI -> chain_eti (cfg 3) -> channel_dev (white noise at OP_CN_DB) + the tone at C/I = OP_CI_DB, added as a tensor ->
    demod_soft_dev / demod_csi_dev -> decode_soft_dev: the unweighted loop has a payload bit error in every returned frame,
    the weighted loop none; metric == contra_sum for every unit of every output of both."""
    import torch
    eti, bits, ref = SC.op_stream()
    layout = pkg.Modulator.frontend_describe(eti[0])
    n_units = len(M.units(layout)[0])
    n = SC.OP_FRAMES
    md = pkg.Modulator(mode=SC.OP_MODE, max_frames=n)
    try:
        md.set_gain(2, 1.0, 1.0 / 50000.0, 4.0)
        md.set_fir_taps(None)
        md.frontend_configure(eti[0])
        per = md.geometry["tf_input_bytes"]
        d_eti = torch.from_numpy(eti).cuda()
        d_cod = torch.zeros((n, per), dtype=torch.uint8, device="cuda")
        d_iq = torch.zeros((n, md.geometry["tf_samples"]), dtype=torch.complex64, device="cuda")
        md.chain_eti_dev_queued(d_eti, eti.shape[0], G | F, d_cod, d_iq)
        md.synchronize()
        power = CC.data_power(d_iq.cpu().numpy(), SC.OP_MODE)
        tone = XC.op_tones((n, md.geometry["tf_samples"]), power, XC.OP_TONES, XC.OP_CI_DB).astype(np.complex64)
        d_rx = torch.zeros_like(d_iq)
        md.set_channel([(0, 1.0, 0.0)], pkg.channel_sigma(power, XC.OP_CN_DB), CC.OP_SEED)
        md.channel_reset(0)
        md.channel_dev(d_iq, d_rx)
        d_rx += torch.from_numpy(tone).cuda()
        d_soft = torch.zeros((n, 8 * per), dtype=torch.int8, device="cuda")
        d_ref = torch.from_numpy(ref).cuda()
        d_out = torch.zeros(n * 6144, dtype=torch.uint8, device="cuda")
        got = {}
        for name, call in (("unweighted", md.demod_soft_dev), ("weighted", md.demod_csi_dev)):
            md.decode_reset()
            call(d_rx, n, d_soft, SC.OP_EARLY)
            md.decode_soft_dev(d_soft, n, d_out, d_ref)
            torch.cuda.synchronize()
            got[name] = [md.decode_soft_stats(i) for i in range(n)]
            for i in range(n):
                for ui in range(n_units):
                    st = md.decode_soft_stats(i, ui)
                    assert st["metric"] == st["contra_sum"], (name, i, ui)
            images = d_out.cpu().numpy().reshape(n, 6144).copy()
        print("C/N %.1f dB, C/I %d dB, %d tone(s): unweighted payload bit errors %s, weighted %s"
              % (XC.OP_CN_DB, XC.OP_CI_DB, XC.OP_TONES, [s["bit_errors"] for s in got["unweighted"][15:]], [s["bit_errors"] for s in got["weighted"][15:]]))
        assert all(s["bit_errors"] > 0 for s in got["unweighted"][15:])
        assert all(s["bit_errors"] == 0 and s["n_bits"] > 0 for s in got["weighted"][15:])
        keep = M.payload_mask(layout)
        assert np.array_equal(images[15:][:, keep], eti[:n - 15][:, keep])
        # the tone's carriers in the state: 40.37 spacings up lies between bins 40 and 41, carrier positions 39 and 40 -- the
        # smallest weights of the frame
        w = md.carrier_state(n - 1)["w"]
        assert set(np.argsort(w)[:2]) == {39, 40} and w[39] < 0.1 and np.median(w) > 0.7
    finally:
        md.close()


# --------------------------------------------------------------------------- 6. dabmod_file --csi, --carrier-mer
def test_dabmod_file_csi_loopback_and_carrier_mer(tmp_path):
    """The operating point's stream behind the channel emulator's white noise at OP_CN_DB: --loopback --soft --csi decodes (exit
    0, the IQ file is the one without the option), --carrier-mer writes one line per frame and carrier with the MER the noise
    gives (C/N 8 dB on the samples: 9.25 dB on a carrier); --csi without --soft is refused."""
    import os
    import subprocess
    from tests import decode_cases as K
    from tests.conftest import ROOT
    exe = os.path.join(ROOT, "odr-dabmod_amd", "host", "dabmod_file")
    fin = str(tmp_path / "in.eti")
    eti, _ = K.stream(SC.OP_FRAMES, SC.OP_SUBCHANNELS, SC.OP_MODE)
    eti.tofile(fin)
    base = ["--gpu-frontend", "--mode", "%d" % SC.OP_MODE, "--batch", "%d" % SC.OP_FRAMES, "--fir", "default", "--loopback",
            "--channel-cn", "%.1f" % XC.OP_CN_DB, "--channel-seed", "%d" % CC.OP_SEED, "--soft"]
    mer = str(tmp_path / "mer.txt")
    outs = []
    for extra in ([], ["--csi", "--carrier-mer", mer]):
        fout = str(tmp_path / ("out%d" % len(outs)))
        r = subprocess.run([exe, fin, fout] + base + extra, capture_output=True, text=True, timeout=300)
        print(r.stderr[-700:])
        assert r.returncode == 0, r.stderr[-2000:]
        assert "loopback: soft decisions, metric " in r.stderr
        outs.append(np.fromfile(fout, np.uint8))
    assert outs[0].size and np.array_equal(outs[0], outs[1])
    nK = MODES[SC.OP_MODE][1]
    rows = np.loadtxt(mer)
    assert rows.shape == (SC.OP_FRAMES * nK, 4)
    assert np.array_equal(rows[:, 0], np.repeat(np.arange(SC.OP_FRAMES), nK)) and np.array_equal(rows[:, 1], np.tile(np.arange(nK), SC.OP_FRAMES))
    # C/N 8 dB on the samples is 8 + 10 log10(N / K) = 9.25 dB on a carrier (tests/test_csi_cpu.py derives the figure); the
    # median of 6912 values whose scatter is sqrt(2 / 75) = 0.7 dB each lies within 0.05 dB of it, the folded amplitude reads
    # a little high on a point this noisy (the model: 9.30 dB): held to 0.3 dB
    assert abs(np.median(rows[:, 2]) - (XC.OP_CN_DB + 10 * np.log10(512 / 384))) < 0.3
    assert 0.9 < np.median(rows[:, 3]) < 1.1 and rows[:, 3].max() <= X.MAX_WEIGHT
    assert "carrier-mer: %d frames behind the channel, window 44 samples early, %d carriers: median " % (SC.OP_FRAMES, nK) in r.stderr
    r = subprocess.run([exe, fin, str(tmp_path / "refused"), "--gpu-frontend", "--loopback", "--csi"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and r.stderr.startswith("dabmod_file: --csi does not go without --loopback --soft")
    assert not os.path.exists(str(tmp_path / "refused"))
