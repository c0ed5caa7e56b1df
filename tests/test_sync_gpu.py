"""The synchroniser on the device (sync.hip; include/dabgpu.h, "the synchroniser"): on every capture of tests/sync_cases.py the
integers of the float64 model (tests/sync_model.py) exactly and its real figures and extracted frames within measured bars; the
whole receiver on the device, capture -> sync -> extract -> demod (-> decode), back to the input bits; byte-identical repeats;
frames that do not fit the buffer; refusals.  tests/test_sync_cpu.py checks on the model that every integer decision asked
for here is far from going the other way.

The eight cases visit one start residue per mode on the block grid B = N / 32, shifts up to -20, max_shift 31 and two frames.
tests/test_sync_axes_gpu.py sweeps the rest with the bars below (tests/sync_cases.py::FAMILIES): start residues 0 ... 2 B and
the last block of the search range; max_shift 0, 1, 7, 31 with the offset at both ends of the shift loop and |eps| up to 0.48;
more frames than the context takes, more slots than candidates, a candidate before the buffer, a frame that ends on the last
sample and one that ends a sample past it, the shortest capture; s16 in Modes II - IV; one echo; TII at shift 31; a fine start
exactly N / 2 off the coarse one.  slack = null - NB B is 32 / 8 / 1 / 16 samples in Modes I - IV: the coarse window at block
boundary b B lies inside a null symbol at s when 0 <= b B - s <= slack.  Equality is asked only where
tests/test_sync_axes_cpu.py has shown on the model that the chosen window's S is exactly 0 or wins over EVERY other window by
1e-3 (the device adds block powers in fp32, relative error about B 2^-24 <= 4e-6: 1e-3 is 250 times that), the runner-up
|D|^2 and |c|^2 are at most 0.6 of the peak and eps is at least 1e-3 away from +-1/2."""
import numpy as np
import pytest

from tests import decode_cases as K
from tests import decode_model as M
from tests import sync_cases as SY
from tests.conftest import record_bound
from tests.sync_model import extract_model, extract_slots, geometry, sync_model

pytestmark = pytest.mark.gpu

# Deviation of the device's figures from the float64 model on the same samples, worst over the eight cases, two frames each;
# measured on the device (profiles/sync.txt; one run on one box).  Each bar is four times its worst value, the project's
# margin for box-to-box variation.  eps: absolute, in carrier spacings; quality, null_depth: relative; extraction: relative
# RMS of a frame.  (The fp32 transform's own error is 1.1e-7.  eps comes from float64 sums of exact products of fp32 samples on
# both sides, the model's exactly rounded: it agrees to the last bit or two.  The worst values below are rounded up in their
# third digit.)
WORST_EPS = 5.6e-17
WORST_QUALITY = 1.68e-7
WORST_NULL_DEPTH = 2.98e-8
WORST_EXTRACT = 3.93e-8


def _bar(worst):
    return 4.0 * worst if worst is not None else 0.0


@pytest.fixture(scope="module")
def mods(pkg):
    """one context per mode, two frames, shared"""
    ms = {m: pkg.Modulator(mode=m, max_frames=2) for m in (1, 2, 3, 4)}
    yield ms
    for m in ms.values():
        m.close()


def _model(name, tail=None):
    """the model's verdict on a named capture, once per process"""
    key = (name, tail)
    if key not in _model.cache:
        x, mode, _, _, _ = SY.named(name, tail)
        r = sync_model(x, mode, SY.MAX_SHIFT, 2)
        r["extracted"] = extract_model(x, mode, r["frames"], extract_slots(SY.n_samples(x), mode, 2))
        _model.cache[key] = r
    return _model.cache[key]


_model.cache = {}


def _device(md, x):
    """sync_dev + sync_extract_dev on the capture -> (records, record bytes, frames as numpy, the device tensors)"""
    import torch
    d_x = torch.from_numpy(np.array(x)).cuda()
    md.sync_dev(d_x, SY.MAX_SHIFT)
    d_out = torch.full((md.sync_slots(SY.n_samples(x)), md.geometry["tf_samples"]), 7.0, dtype=torch.complex64, device="cuda")
    md.sync_extract_dev(d_x, d_out)
    torch.cuda.synchronize()
    return md.sync_result(), md.sync_result_bytes(), d_out.cpu().numpy(), d_x, d_out


def _same_integers(got, want):
    assert len(got) == want["n_frames"], (len(got), want["n_frames"])
    for k, (a, b) in enumerate(zip(got, want["frames"])):
        assert (a["start"], a["shift"], a["valid"]) == (b["start"], b["shift"], b["valid"]), (k, a, b)


# --------------------------------------------------------------------------- 1 - 4. every case
@pytest.mark.parametrize("name", sorted(SY.CASES))
def test_every_case_gives_the_models_integers_figures_frames_and_the_input_bits(mods, name):
    """(1) n_frames, start, shift, valid EQUAL to the model's; eps, quality, null_depth within the bars.  (2) the extracted
    frames against the model's, relative RMS per frame.  (3) sync_dev -> sync_extract_dev -> demod_dev(early = CP / 2) gives the
    input bits, bit_errors 0.  (4) a second sync_dev + extract on the same buffer: the same bytes."""
    import torch
    x, mode, bits, _, _ = SY.named(name)
    md = mods[mode]
    g = geometry(mode)
    want = _model(name)
    got, raw, frames, d_x, d_out = _device(md, x)
    _same_integers(got, want)
    dev_e = dev_q = dev_n = dev_x = 0.0
    for k, (a, b) in enumerate(zip(got, want["frames"])):
        dev_e = max(dev_e, abs(a["eps"] - b["eps"]))
        dev_q = max(dev_q, abs(a["quality"] / b["quality"] - 1.0))
        if b["null_depth"] == 0.0:
            assert a["null_depth"] == 0.0
        else:
            dev_n = max(dev_n, abs(a["null_depth"] / b["null_depth"] - 1.0))
        assert a["cfo_hz"] == (a["shift"] + a["eps"]) * 2048000.0 / g["N"]
        ref = want["extracted"][k]
        dev_x = max(dev_x, float(np.linalg.norm(frames[k] - ref) / np.linalg.norm(ref)))
    print("%s: deviation eps %.3g, quality %.3g, null_depth %.3g, extraction rel-RMS %.3g" % (name, dev_e, dev_q, dev_n, dev_x))
    # (3) the receiver behind it, on the device
    d_bits = torch.zeros((2, md.geometry["tf_input_bytes"]), dtype=torch.uint8, device="cuda")
    md.demod_dev(d_out, 2, g["CP"] // 2, d_bits, torch.from_numpy(bits.copy()).cuda())
    torch.cuda.synchronize()
    assert np.array_equal(d_bits.cpu().numpy(), bits)
    assert all(md.monitor_stats(f)["bit_errors"] == 0 and md.monitor_stats(f)["n_bits"] == 8 * bits.shape[1] for f in range(2))
    # (4) again
    md.sync_dev(d_x, SY.MAX_SHIFT)
    d_again = torch.full_like(d_out, 3.0)
    md.sync_extract_dev(d_x, d_again)
    torch.cuda.synchronize()
    assert md.sync_result_bytes() == raw and len(raw) == 2 * 48
    assert torch.equal(d_again.view(torch.float32), d_out.view(torch.float32))
    ok = [record_bound("sync eps vs float64 model, %s" % name, dev_e, _bar(WORST_EPS)),
          record_bound("sync quality vs float64 model, %s" % name, dev_q, _bar(WORST_QUALITY)),
          record_bound("sync null_depth vs float64 model, %s" % name, dev_n, _bar(WORST_NULL_DEPTH)),
          record_bound("sync extraction rel-RMS vs float64 model, %s" % name, dev_x, _bar(WORST_EXTRACT))]
    assert all(ok), (dev_e, dev_q, dev_n, dev_x)


def test_host_entries_give_what_the_device_entries_give(mods):
    x, mode, _, _, _ = SY.named("m3_cfg2")
    md = mods[mode]
    _, raw, frames, _, _ = _device(md, x)
    assert md.sync(np.array(x), SY.MAX_SHIFT) == md.sync_result() and md.sync_result_bytes() == raw
    assert np.array_equal(md.sync_extract(np.array(x)).view(np.float32), frames.view(np.float32))


# --------------------------------------------------------------------------- 3b. on through the channel decoder
def test_mode_2_capture_of_an_eti_fed_chain_decodes_to_the_eti_payload(pkg):
    """ETI -> chain_eti (cfg 2, Mode II, 19 frames) -> a capture of 18 of them at start 333, 5.3 spacings off -> sync ->
    extract -> demod -> decode: coded bits and payload equal."""
    import torch
    n = 18
    eti, bits = K.stream(n + 1, K.MULTI, 2, seed=31)
    md = pkg.Modulator(mode=2, max_frames=n + 1)
    try:
        md.frontend_configure(eti[0])
        y = md.chain_eti(eti, 0)
        x = SY.capture_of(y, 2, 333, 5.3, 0.9, None, 0, n_frames=n)
        d_x = torch.from_numpy(x).cuda()
        md.sync_dev(d_x, SY.MAX_SHIFT)
        assert md.sync_slots(x.size) == n
        d_out = torch.empty((n, md.geometry["tf_samples"]), dtype=torch.complex64, device="cuda")
        md.sync_extract_dev(d_x, d_out)
        d_bits = torch.zeros((n, md.geometry["tf_input_bytes"]), dtype=torch.uint8, device="cuda")
        md.demod_dev(d_out, n, geometry(2)["CP"] // 2, d_bits)
        torch.cuda.synchronize()
        res = md.sync_result()
        assert [(r["start"], r["shift"], r["valid"]) for r in res] == [(333 + k * 49152, 5, 1) for k in range(n)]
        assert all(abs(r["shift"] + r["eps"] - 5.3) <= 1e-3 for r in res)
        got = d_bits.cpu().numpy()
        assert np.array_equal(got, bits[:n])
        layout = pkg.Modulator.frontend_describe(eti[0])
        keep = M.payload_mask(layout)
        images, stats = md.decode(got, K.reference_rows(eti[:n], n))
        assert np.array_equal(images[15:][:, keep], eti[:n - 15][:, keep])
        assert all(s["corrected"] == 0 and s["bit_errors"] == 0 for s in stats)
    finally:
        md.close()


# --------------------------------------------------------------------------- 5. frames that do not fit the buffer
def _check_against_model_with_invalid_frames(md, x, mode, want):
    got, _, frames, _, _ = _device(md, x)
    _same_integers(got, want)
    for k, b in enumerate(want["frames"]):
        ref = want["extracted"][k]
        if b["valid"]:
            assert np.linalg.norm(frames[k] - ref) / np.linalg.norm(ref) <= _bar(WORST_EXTRACT), k
        else:
            assert not frames[k].view(np.float32).any(), k
    for k in range(len(want["frames"]), frames.shape[0]):
        assert not frames[k].view(np.float32).any(), k              # (slots past the candidates)


def test_trimmed_tail_follows_the_models_verdict(mods):
    """The cfg 3 capture with B / 2 samples behind its last frame: whether the last candidate refines to start + tf > n is the
    model's to say; valid, the zeros of a frame that is not, and the other frames are asserted on its verdict."""
    g = geometry(1)
    x, mode, _, _, _ = SY.named("m1_cfg3", g["B"] // 2)
    _check_against_model_with_invalid_frames(mods[mode], x, mode, _model("m1_cfg3", g["B"] // 2))


def test_a_frame_that_starts_before_the_buffer_is_not_valid_and_is_written_as_zeros(mods):
    """The clean Mode II capture without its first five samples: frame 0 refines to start -5 (valid 0, zeros), frame 1 is found
    and extracted as ever."""
    g = geometry(2)
    x = np.array(SY.named("m2_clean", g["null"] + 16)[0][5:])
    want = sync_model(x, 2, SY.MAX_SHIFT, 2)
    want["extracted"] = extract_model(x, 2, want["frames"], extract_slots(x.size, 2, 2))
    assert [(f["start"], f["valid"]) for f in want["frames"]] == [(-5, 0), (g["tf"] - 5, 1)]
    _check_against_model_with_invalid_frames(mods[2], x, 2, want)


# --------------------------------------------------------------------------- 6. refusals
def test_refusals_queue_nothing_and_a_valid_call_follows(pkg):
    import torch
    x, mode, _, _, _ = SY.named("m3_cfg2")
    g = geometry(mode)
    md = pkg.Modulator(mode=mode, max_frames=2)
    try:
        d_x = torch.from_numpy(np.array(x)).cuda()
        d_out = torch.zeros((2, g["tf"]), dtype=torch.complex64, device="cuda")
        with pytest.raises(pkg.DabGpuError) as e:
            md.sync_extract_dev(d_x, d_out)                           # before any sync
        assert "no dabgpu_sync* call" in str(e.value)
        with pytest.raises(pkg.DabGpuError) as e:
            md.sync_result()
        assert "no synchroniser result" in str(e.value)
        with pytest.raises(pkg.DabGpuError) as e:
            md.sync_dev(d_x[:2 * g["tf"] + g["null"] - 1], SY.MAX_SHIFT)
        assert "too short" in str(e.value)
        with pytest.raises(pkg.DabGpuError) as e:
            md.sync_dev(torch.zeros(2 * x.size, dtype=torch.uint8, device="cuda"), SY.MAX_SHIFT)
        assert "format" in str(e.value)
        with pytest.raises(pkg.DabGpuError) as e:
            md.sync_dev(d_x, 32)
        assert "max_shift" in str(e.value)
        rc = md._lib.dabgpu_sync_dev(md._h, d_x.data_ptr() + 4, 0, x.size - 1, SY.MAX_SHIFT, None)      # four bytes off
        assert rc != 0 and b"aligned" in md._lib.dabgpu_last_error(md._h)
        with pytest.raises(pkg.DabGpuError):
            md.sync_result()                                          # (still nothing queued, nothing to report)
        got, _, frames, _, _ = _device(md, x)
        want = _model("m3_cfg2")
        _same_integers(got, want)
        with pytest.raises(pkg.DabGpuError) as e:
            md.sync_extract_dev(d_x[:-1], d_out)                      # another n_samples than the sync before it
        assert "no dabgpu_sync* call" in str(e.value)
        assert np.array_equal(md.sync_extract(np.array(x)).view(np.float32), frames.view(np.float32))
    finally:
        md.close()
