"""Soft decisions on the device (include/dabgpu.h: dabgpu_demod_soft*, dabgpu_decode_soft*): the receiver's int8
metrics against the float64 model, the soft Viterbi decoder against the integer model (tests/soft_model.py) byte for byte and
figure for figure, hard and soft streams side by side on one context, and the whole loop at the C/N where soft decisions
decode what hard decisions lose (found on the models by tests/test_soft_cpu.py)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import decode_cases as K
from tests import decode_model as M
from tests import demod_cases as DC
from tests import soft_cases as SC
from tests import soft_model as S
from tests.conftest import ROOT, record_bound
from tests.golden.synth import synth_eti

pytestmark = pytest.mark.gpu
HOST = os.path.join(ROOT, "odr-dabmod_amd", "host")
G, F = 1, 2
BAR_SIGNAL, BAR_QUADRATURE = 4 * 1.036e-7, 4 * 1.128e-7          # tests/test_demod_gpu.py: the sums repeat to these

# Share of the device's softs one step from the float64 model's, on cfg 2 output with noise 8 dB below the data symbols, two
# frames per mode.  A step is 1/64 of the clean level and the fp32 transform lies 1e-7 from the model: a soft differs where the
# exact value lies that close to a rounding boundary.  Measured on the device: 2 of 460 800 softs in Mode I and 1 of 230 400 in
# Mode IV (a share of 4.34e-6 each), none in modes II and III (profiles/soft_measured_bounds.jsonl).  The
# softs repeat bit for bit, so the share does too on the same input; the bar is four times the worst measured share, under
# the cap of 1e-3.
ONE_STEP_SHARE_MEASURED = 4.34e-6
ONE_STEP_SHARE_BAR = min(4 * ONE_STEP_SHARE_MEASURED, 1e-3)


def _cfg3(pkg, mode, n, s16=False):
    md = pkg.Modulator(mode=mode, max_frames=n)
    md.set_gain(2, 1.0, (32767.0 if s16 else 1.0) / 50000.0, 4.0)
    md.set_fir_taps(None)
    if s16:
        md.set_output_format("s16")
    return md


def _stats_agree(a, b):
    assert (a["bit_errors"], a["n_bits"], a["min_margin"]) == (b["bit_errors"], b["n_bits"], b["min_margin"])
    assert abs(a["sum_signal"] / b["sum_signal"] - 1.0) <= BAR_SIGNAL
    assert abs(a["sum_quadrature"] / b["sum_quadrature"] - 1.0) <= BAR_QUADRATURE


# --------------------------------------------------------------------------- 1. clean output
@pytest.mark.parametrize("mode,s16", [(1, False), (2, False), (3, False), (4, False), (1, True)])
def test_clean_cfg3_output_gives_softs_of_the_bits_sign_and_the_hard_calls_figures(pkg, mode, s16):
    md = _cfg3(pkg, mode, 2, s16)
    try:
        per = md.geometry["tf_input_bytes"]
        bits = DC.case_bits(mode, 2, per)
        iq = md.chain(bits, G | F)
        soft, got = md.demod_soft(iq, early=44, ref_bits=bits, want_bits=True)
        st_soft = [md.monitor_stats(f) for f in range(2)]
        assert soft.shape == (2, 8 * per) and soft.dtype == np.int8
        assert np.array_equal(soft > 0, np.unpackbits(bits, axis=1) == 1) and not (soft == 0).any()
        print("mode %d s16 %s: clean softs %d ... %d" % (mode, s16, np.abs(soft.astype(int)).min(), np.abs(soft.astype(int)).max()))
        hard = md.demod(iq, early=44, ref_bits=bits)
        st_hard = [md.monitor_stats(f) for f in range(2)]
        assert np.array_equal(got, hard) and np.array_equal(hard, bits)
        for a, b in zip(st_soft, st_hard):
            _stats_agree(a, b)
            assert a["bit_errors"] == 0 and a["n_bits"] == 8 * per
        # softs alone, no reference: the hard figures all the same
        assert np.array_equal(md.demod_soft(iq, early=44), soft) and md.monitor_stats(1)["n_bits"] == 0
    finally:
        md.close()


def test_soft_calls_share_the_hard_calls_refusals(pkg):
    import torch
    md = pkg.Modulator(mode=3, max_frames=1)
    try:
        g = md.geometry
        d_y = torch.zeros(g["tf_samples"], dtype=torch.complex64, device="cuda")
        d_soft = torch.zeros(8 * g["tf_input_bytes"], dtype=torch.int8, device="cuda")
        for bad in (-1, 64):
            with pytest.raises(pkg.DabGpuError, match="cyclic prefix"):
                md.demod_soft_dev(d_y, 1, d_soft, bad)
        with pytest.raises(pkg.DabGpuError, match="soft buffer"):
            md.demod_soft_dev(d_y, 1, d_soft[:-8])
        with pytest.raises(pkg.DabGpuError):
            md.demod_soft(np.zeros(2 * g["tf_samples"], np.int8))
        with pytest.raises(pkg.DabGpuError, match="max_frames"):
            md.demod_soft(np.zeros(2 * g["tf_samples"], np.complex64))
        # an all-zero frame: P = 0, every soft 0
        md.demod_soft_dev(d_y, 1, d_soft.fill_(5))
        assert not d_soft.cpu().numpy().any()
    finally:
        md.close()


# --------------------------------------------------------------------------- 2. against the float64 model
@pytest.mark.parametrize("mode", [1, 2, 3, 4])
def test_softs_follow_the_float64_model_on_a_noisy_signal(pkg, mode):
    md = pkg.Modulator(mode=mode, max_frames=2)
    try:
        per = md.geometry["tf_input_bytes"]
        bits = DC.case_bits(mode, 2, per)
        y = md.chain(bits, 0).reshape(2, -1)
        noisy = S.add_noise(y, mode, 8.0, 50 + mode).astype(np.complex64)
        soft = md.demod_soft(noisy, early=0).astype(np.int64)
        want = np.stack([S.demod_soft_model(noisy[f], mode, 0) for f in range(2)]).astype(np.int64)
        for v in (127, -127, 0):
            assert (want == v).any(), v
        diff = np.abs(soft - want)
        share = float((diff == 1).mean())
        print("mode %d: %d of %d softs one step from the model (share %.3g), worst %d" % (mode, (diff == 1).sum(), diff.size, share, diff.max()))
        assert diff.max() <= 1
        assert record_bound("demod_soft share one step from the float64 model, mode %d" % mode, share, ONE_STEP_SHARE_BAR)
    finally:
        md.close()


# --------------------------------------------------------------------------- 3. run geometry
@pytest.mark.parametrize("mode", [1, 3])
def test_run_geometry_and_repetition_give_the_same_soft_bytes(pkg, mode):
    md = pkg.Modulator(mode=mode, max_frames=2)
    try:
        per = md.geometry["tf_input_bytes"]
        nblocks = md.geometry["nb_symbols"] - 1
        bits = DC.case_bits(mode, 2, per)
        noisy = S.add_noise(md.chain(bits, 0).reshape(2, -1), mode, 8.0, 60 + mode).astype(np.complex64)
        # the same frames as s16: scaled into the format's range and truncated, as test_clock_gpu.py does
        scale = 20000.0 / float(np.abs(noisy.view(np.float32)).max())
        q = np.trunc(noisy.view(np.float32).reshape(2, -1) * scale).astype(np.int16)
        for frames in (noisy, q):
            md.set_demod_run_symbols(0)
            first = md.demod_soft(frames)
            assert len(np.unique(first)) > 200
            assert np.array_equal(md.demod_soft(frames), first)
            for spr in (1, 2, 7, nblocks):
                md.set_demod_run_symbols(spr)
                soft, got = md.demod_soft(frames, want_bits=True)
                assert np.array_equal(soft, first), (frames.dtype, spr)
                assert np.array_equal(got, md.demod(frames)), (frames.dtype, spr)
    finally:
        md.close()


# --------------------------------------------------------------------------- 4. the decoder against the integer model
@pytest.fixture(scope="module")
def mods(pkg):
    ms = {m: pkg.Modulator(mode=m, max_frames=17) for m in (1, 2, 3, 4)}
    yield ms
    for m in ms.values():
        m.close()


def _model_check(md, layout, soft, ref, images, n):
    want_images, want, valid = S.decode_soft_stream(layout, soft, ref)
    assert np.array_equal(images, want_images)
    for i in range(n):
        for ui in range(len(want[i])):
            st = md.decode_soft_stats(i, ui)
            assert st.pop("valid") == int(valid[i])
            assert st == want[i][ui], (i, ui)
            assert st["metric"] == st["contra_sum"]
    return want


DECODER_LAYOUTS = [("nst0", ())] + [("%d_%#x" % p, ((0,) + p,)) for p in K.PADDING_AND_SMALLEST] + \
                  [("multi", K.MULTI), ("full_cif", K.SHAPES["full_cif"])]


@pytest.mark.parametrize("name,sub", DECODER_LAYOUTS, ids=[n for n, _ in DECODER_LAYOUTS])
def test_decode_soft_equals_the_hard_decoder_on_unit_softs_and_the_model_on_any_int8(pkg, mods, name, sub):
    """Mode II, 17 transmission frames: two outputs.  full_cif (864 CU) is the LDS maximum, 55 296 B of punctured softs."""
    md = mods[2]
    eti, bits = K.stream(17, sub, 2, seed=77)
    layout = pkg.Modulator.frontend_describe(eti[0])
    ref = K.reference_rows(eti, 17)
    md.frontend_configure(eti[0])
    n_units = 1 + len(sub)
    # (a) +-1 softs of bits with one per cent flipped: the hard decoder's images and counts, ties included
    got = bits ^ K.dense_flips(bits.shape, seed=13, rate=0.01)
    hard_images, _ = md.decode(got, ref)
    hard = [[md.decode_stats(i, ui) for ui in range(n_units)] for i in range(17)]
    images, _ = md.decode_soft(S.soft_of_bits(got), ref)
    assert np.array_equal(images, hard_images) and images[15:].any()
    total = 0
    for i in range(17):
        for ui in range(n_units):
            st, h = md.decode_soft_stats(i, ui), hard[i][ui]
            assert st["metric"] == st["contra_sum"] == st["corrected"] == h["corrected"], (i, ui)
            assert (st["valid"], st["coded_bits"], st["bit_errors"], st["n_bits"]) == (h["valid"], h["coded_bits"], h["bit_errors"], h["n_bits"])
            assert st["erasures"] == 0 and st["soft_sum"] == st["coded_bits"]
            total += st["corrected"]
    assert total > 0
    # (b) any int8
    md.decode_reset()
    soft = SC.random_soft((17, 8 * bits.shape[1]), seed=17)
    assert (soft == 0).mean() > 0.09 and (soft == 127).any() and (soft == -127).any() and (soft == -128).any()
    images, _ = md.decode_soft(soft, ref)
    want = _model_check(md, layout, soft, ref, images, 17)
    assert all(st["metric"] > 0 and st["erasures"] > 0 for st in want[16])


@pytest.mark.parametrize("mode,n_tf", [(1, 4), (2, 16), (3, 16), (4, 8)])
def test_fic_shapes_of_every_mode(pkg, mods, mode, n_tf):
    md = mods[mode]
    eti, bits = K.stream(n_tf * M.CIFS[mode], (), mode, seed=5)
    layout = pkg.Modulator.frontend_describe(eti[0])
    n = eti.shape[0]
    ref = K.reference_rows(eti, n)
    md.frontend_configure(eti[0])
    soft = SC.random_soft((n_tf, 8 * bits.shape[1]), seed=30 + mode)
    images, _ = md.decode_soft(soft, ref)
    _model_check(md, layout, soft, ref, images, n)
    # and clean +-64: the payload comes back with nothing to correct
    md.decode_reset()
    images, stats = md.decode_soft(S.soft_of_bits(bits, 64), ref)
    keep = M.payload_mask(layout)
    assert np.array_equal(images[15:][:, keep], eti[:n - 15][:, keep])
    assert all(s["metric"] == 0 and s["bit_errors"] == 0 and s["soft_sum"] == 64 * s["coded_bits"] for s in stats)


def test_a_mode_one_stream_in_one_call_frame_by_frame_and_in_uneven_calls(pkg, mods):
    md = mods[1]
    eti, bits = K.stream(20, K.MULTI, 1, seed=4321)
    layout = pkg.Modulator.frontend_describe(eti[0])
    ref = K.reference_rows(eti, 20)
    soft = SC.random_soft((5, 8 * bits.shape[1]), seed=8)
    md.frontend_configure(eti[0])

    def run(pieces):
        images, stats = [], []
        for a, b in pieces:
            im, _ = md.decode_soft(soft[a:b], ref[4 * a:4 * b])
            images.append(im)
            stats += [[md.decode_soft_stats(i, u) for u in range(-1, 6)] for i in range(4 * (b - a))]
        return np.concatenate(images), stats

    one = run([(0, 5)])
    _model_check(md, layout, soft, ref, one[0], 20)
    for pieces in ([(k, k + 1) for k in range(5)], [(0, 1), (1, 4), (4, 5)]):
        md.decode_reset()
        other = run(pieces)
        assert np.array_equal(other[0], one[0]) and other[1] == one[1]


# --------------------------------------------------------------------------- 5. hard and soft side by side
def test_hard_and_soft_streams_on_one_context_do_not_see_each_other(pkg):
    eti, bits = K.stream(17, ((0, 24, 1),), 2, seed=3)
    ref = K.reference_rows(eti, 17)
    hard_in = bits ^ K.dense_flips(bits.shape, seed=2, rate=0.02)
    soft_in = SC.random_soft((17, 8 * bits.shape[1]), seed=4)
    md = pkg.Modulator(mode=2, max_frames=17)
    try:
        md.frontend_configure(eti[0])
        alone_hard = md.decode(hard_in, ref)
        alone_soft = md.decode_soft(soft_in, ref)
        assert alone_hard[0][15:].any() and not np.array_equal(alone_hard[0], alone_soft[0])

        def mixed():
            h1 = md.decode(hard_in[:8], ref[:8])
            s1 = md.decode_soft(soft_in[:5], ref[:5])
            h2 = md.decode(hard_in[8:], ref[8:])
            s2 = md.decode_soft(soft_in[5:], ref[5:])
            return (np.concatenate([h1[0], h2[0]]), h1[1] + h2[1]), (np.concatenate([s1[0], s2[0]]), s1[1] + s2[1])

        # without a reset the histories of the two runs above are still there: the first outputs are "valid" and differ
        stale = mixed()
        assert stale[0][1][0]["valid"] == 1 and stale[1][1][0]["valid"] == 1
        md.decode_reset()
        h, s = mixed()
        assert np.array_equal(h[0], alone_hard[0]) and h[1] == alone_hard[1]
        assert np.array_equal(s[0], alone_soft[0]) and s[1] == alone_soft[1]
        # refusals leave both histories and the last statistics alone
        md.decode_reset()
        md.decode(hard_in[:8], ref[:8])
        md.decode_soft(soft_in[:8], ref[:8])
        before = ([md.decode_stats(i) for i in range(8)], [md.decode_soft_stats(i) for i in range(8)])
        out = np.empty(6144, np.uint8)
        ob = C.c_size_t()
        part = np.ascontiguousarray(soft_in[8:10])
        assert md._lib.dabgpu_decode_soft(md._h, part.ctypes.data, 2, out.ctypes.data, out.nbytes, None, C.byref(ob)) == -4
        assert ob.value == 2 * 6144
        assert md._lib.dabgpu_decode_soft(md._h, part.ctypes.data, 0, out.ctypes.data, out.nbytes, None, C.byref(ob)) == -1
        with pytest.raises(pkg.DabGpuError, match="max_frames"):
            md.decode_soft(np.zeros((18, 8 * bits.shape[1]), np.int8))
        with pytest.raises(pkg.DabGpuError, match="input size"):
            md.decode_soft(np.zeros(8 * bits.shape[1] - 8, np.int8))
        assert before == ([md.decode_stats(i) for i in range(8)], [md.decode_soft_stats(i) for i in range(8)])
        h2, s2 = md.decode(hard_in[8:], ref[8:]), md.decode_soft(soft_in[8:], ref[8:])
        assert np.array_equal(h2[0], alone_hard[0][8:]) and h2[1] == alone_hard[1][8:]
        assert np.array_equal(s2[0], alone_soft[0][8:]) and s2[1] == alone_soft[1][8:]
    finally:
        md.close()


def test_soft_refusals_before_a_layout_and_on_an_overlapping_one(pkg):
    md = pkg.Modulator(mode=1, max_frames=2)
    try:
        per = 8 * md.geometry["tf_input_bytes"]
        with pytest.raises(pkg.DabGpuError, match="decode: not configured"):
            md.decode_soft(np.zeros(per, np.int8))
        with pytest.raises(pkg.DabGpuError, match="no soft decoder statistics"):
            md.decode_soft_stats(0)
        over, _ = K.stream(4, K.SHAPES["overlap_last_wins"], 1)
        md.frontend_configure(over[0])
        with pytest.raises(pkg.DabGpuError, match="overlap at capacity unit 50"):
            md.decode_soft(np.zeros(per, np.int8))
    finally:
        md.close()


# --------------------------------------------------------------------------- 6. end to end, where soft beats hard
def test_at_the_operating_point_the_soft_loop_decodes_what_the_hard_loop_loses(pkg):
    """ETI -> chain_eti (cfg 3) -> the CPU test's noise at L (tests/soft_cases.py), added on the device -> demod / demod_soft
    -> decode / decode_soft."""
    import torch
    eti, bits, ref = SC.op_stream()
    layout = pkg.Modulator.frontend_describe(eti[0])
    n = SC.OP_FRAMES
    md = _cfg3(pkg, SC.OP_MODE, n)
    try:
        md.frontend_configure(eti[0])
        iq = md.chain_eti(eti, G | F).reshape(n, -1)
        noise = S.add_noise(iq, SC.OP_MODE, SC.OP_LEVEL_DB, SC.OP_SEED) - iq.astype(np.complex128)
        d_iq = (torch.from_numpy(iq).cuda() + torch.from_numpy(noise.astype(np.complex64)).cuda()).contiguous()
        per = md.geometry["tf_input_bytes"]
        d_bits = torch.zeros((n, per), dtype=torch.uint8, device="cuda")
        d_soft = torch.zeros((n, 8 * per), dtype=torch.int8, device="cuda")
        d_ref = torch.from_numpy(ref).cuda()
        d_out = torch.zeros(n * 6144, dtype=torch.uint8, device="cuda")
        md.demod_dev(d_iq, n, SC.OP_EARLY, d_bits)
        md.decode_dev(d_bits, n, d_out, d_ref)
        hard = [md.decode_stats(i)["bit_errors"] for i in range(15, n)]
        md.demod_soft_dev(d_iq, n, d_soft, SC.OP_EARLY)
        md.decode_soft_dev(d_soft, n, d_out, d_ref)
        torch.cuda.synchronize()
        soft_stats = [md.decode_soft_stats(i) for i in range(n)]
        print("C/N %.1f dB: hard payload bit errors %s, soft %s, soft metric / soft_sum %s"
              % (SC.OP_LEVEL_DB, hard, [s["bit_errors"] for s in soft_stats[15:]],
                 ["%d/%d" % (s["metric"], s["soft_sum"]) for s in soft_stats[15:]]))
        assert all(e > 0 for e in hard)
        assert all(s["bit_errors"] == 0 and s["n_bits"] > 0 for s in soft_stats[15:])
        images = d_out.cpu().numpy().reshape(n, 6144)
        keep = M.payload_mask(layout)
        assert np.array_equal(images[15:][:, keep], eti[:n - 15][:, keep])
        _model_check(md, layout, d_soft.cpu().numpy(), ref, images, n)
    finally:
        md.close()


# --------------------------------------------------------------------------- 7. dabmod_file --soft
def _dabmod_file(fin, fout, opts):
    return subprocess.run([os.path.join(HOST, "dabmod_file"), fin, fout] + opts, capture_output=True, text=True, timeout=300)


def test_dabmod_file_soft_loopback(tmp_path):
    """20 frames in Mode I: five come back; the clean loop has metric 0 and no erasures, and the IQ file is the one without
    the option.  --soft without --loopback is refused."""
    fin = str(tmp_path / "in.eti")
    synth_eti(20, subchannels=K.MULTI, mid=1).tofile(fin)
    us, _ = M.units(load_layout(fin))
    coded = 5 * sum(u["coded_bits"] for u in us)
    outs = []
    for extra in ([], ["--soft"]):
        fout = str(tmp_path / ("out%d" % len(outs)))
        r = _dabmod_file(fin, fout, ["--gpu-frontend", "--fir", "default", "--loopback"] + extra)
        assert r.returncode == 0, r.stderr[-2000:]
        assert r.stdout.split() == ["20", "5", "5"]
        assert "loopback: 5 frames compared, 0 FIC and 0 MSC payload bit errors in" in r.stderr
        assert ("loopback: soft decisions, metric 0 / soft_sum " in r.stderr) == bool(extra), r.stderr
        if extra:
            line = [ln for ln in r.stderr.splitlines() if "soft decisions" in ln][0]
            soft_sum = int(line.split("soft_sum ")[1].split(",")[0])
            assert 32 * coded < soft_sum <= 127 * coded and line.endswith(", 0 erasures")
        outs.append(np.fromfile(fout, np.uint8))
    assert outs[0].size and np.array_equal(outs[0], outs[1])
    fout = str(tmp_path / "refused")
    r = _dabmod_file(fin, fout, ["--gpu-frontend", "--soft"])
    assert r.returncode == 2 and r.stderr.startswith("dabmod_file: --soft does not go without --loopback")
    assert not os.path.exists(fout)


def load_layout(path):
    from tests.conftest import load_pkg
    return load_pkg().Modulator.frontend_describe(np.fromfile(path, np.uint8, 6144))
