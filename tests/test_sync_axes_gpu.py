"""The synchroniser on the device across the swept families of tests/sync_cases.py: start residues on the block grid, offset x
search range, frame count and buffer ends, s16 outside Mode I, one echo, TII at the edge of the range.  One test is one family
in one mode.  On every capture n_frames and every record's start, shift and valid EQUAL the float64 model's
(tests/test_sync_axes_cpu.py shows on the model that no decision asked for here is close); eps, quality, null_depth and the
extracted frames lie within the bars tests/test_sync_gpu.py carries; frames of candidates that are not valid and slots past the
candidates are zeros in a buffer prefilled with something else (the records past the candidates are not handed out:
dabgpu_get_sync_result copies n_frames of them, and exactly 48 n_frames bytes are asserted); a repeat gives the same bytes; and demod_dev behind it gives
the chain's bits wherever the CPU file showed that the numpy receiver does."""
import numpy as np
import pytest

from tests import sync_cases as SY
from tests.conftest import record_bound
from tests.sync_model import geometry
from tests.test_sync_gpu import WORST_EPS, WORST_EXTRACT, WORST_NULL_DEPTH, WORST_QUALITY, _bar

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def contexts(pkg):
    """one context per (mode, max_frames), made when first asked for, shared"""
    made = {}

    def get(mode, max_frames):
        if (mode, max_frames) not in made:
            made[mode, max_frames] = pkg.Modulator(mode=mode, max_frames=max_frames)
        return made[mode, max_frames]
    yield get
    for md in made.values():
        md.close()


def _sync_and_extract(md, d_x, n, max_shift, fill):
    import torch
    md.sync_dev(d_x, max_shift)
    d_out = torch.full((md.sync_slots(n), md.geometry["tf_samples"]), fill, dtype=torch.complex64, device="cuda")
    md.sync_extract_dev(d_x, d_out)
    torch.cuda.synchronize()
    return md.sync_result(), md.sync_result_bytes(), d_out


def _demod_gives_the_bits(md, c, d_out, got, early):
    """demod_dev on the valid frames (runs of them: a frame of zeros is not a frame) -> the chain's bits, bit_errors 0"""
    import torch
    per = md.geometry["tf_input_bytes"]
    k = 0
    while k < len(got):
        if not got[k]["valid"]:
            k += 1
            continue
        e = k
        while e < len(got) and got[e]["valid"]:
            e += 1
        bits = np.stack([SY.family_frame_bits(c, got[j]["start"]) for j in range(k, e)])
        d_bits = torch.zeros((e - k, per), dtype=torch.uint8, device="cuda")
        md.demod_dev(d_out[k:e], e - k, early, d_bits, torch.from_numpy(bits).cuda())
        torch.cuda.synchronize()
        assert np.array_equal(d_bits.cpu().numpy(), bits), (c.label, k, e)
        stats = [md.monitor_stats(f) for f in range(e - k)]
        assert all(s["bit_errors"] == 0 and s["n_bits"] == 8 * per for s in stats), (c.label, stats)
        k = e


@pytest.mark.parametrize("fam,mode", SY.FAMILY_MODES)
def test_family_gives_the_models_integers_figures_zeros_and_the_input_bits(contexts, fam, mode):
    import torch
    g = geometry(mode)
    tf = g["tf"]
    dev_e = dev_q = dev_n = dev_x = 0.0
    for i, c in enumerate(SY.family(fam, mode)):
        md = contexts(mode, c.max_frames)
        x = SY.family_capture(c)
        n = SY.n_samples(x)
        want = SY.family_model(c, x)
        d_x = torch.from_numpy(np.ascontiguousarray(x)).cuda()
        got, raw, d_out = _sync_and_extract(md, d_x, n, c.max_shift, 7.0)
        frames = d_out.cpu().numpy()
        # integers
        assert frames.shape == (want["slots"], tf) and len(raw) == 48 * want["n_frames"], (c.label, frames.shape, len(raw))
        assert len(got) == want["n_frames"], (c.label, len(got), want["n_frames"])
        for k, (a, b) in enumerate(zip(got, want["frames"])):
            assert (a["start"], a["shift"], a["valid"]) == (b["start"], b["shift"], b["valid"]), (c.label, k, a, b)
            assert a["cfo_hz"] == (a["shift"] + a["eps"]) * 2048000.0 / g["N"]
        assert (want["slots"], tuple((a["start"], a["valid"]) for a in got)) == c.expect, c.label
        # figures
        for k, (a, b) in enumerate(zip(got, want["frames"])):
            dev_e = max(dev_e, abs(a["eps"] - b["eps"]))
            dev_q = max(dev_q, abs(a["quality"] / b["quality"] - 1.0))
            if b["null_depth"] == 0.0:
                assert a["null_depth"] == 0.0, (c.label, a)
            else:
                dev_n = max(dev_n, abs(a["null_depth"] / b["null_depth"] - 1.0))
            if b["valid"]:
                ref = want["extracted"][k]
                dev_x = max(dev_x, float(np.linalg.norm(frames[k] - ref) / np.linalg.norm(ref)))
        # zeros: candidates that are not valid, slots past the candidates
        for k in range(want["slots"]):
            if k >= want["n_frames"] or not want["frames"][k]["valid"]:
                assert not frames[k].view(np.float32).any(), (c.label, k)
        # the host entries, where the family is about the sample format
        if fam == "D":
            assert md.sync(np.array(x), c.max_shift) == got and md.sync_result_bytes() == raw
            assert np.array_equal(md.sync_extract(np.array(x)).view(np.float32), frames.view(np.float32))
        # again: the same bytes
        if i == 0 or fam == "D":
            again, raw2, d_again = _sync_and_extract(md, d_x, n, c.max_shift, 3.0)
            assert raw2 == raw and again == got, c.label
            assert torch.equal(torch.view_as_real(d_again), torch.view_as_real(d_out)), c.label
        # behind it
        if c.receiver:
            _demod_gives_the_bits(md, c, d_out, got, g["CP"] // 2)
    print("sync axes %s mode %d: deviation eps %.3g, quality %.3g, null_depth %.3g, extraction rel-RMS %.3g"
          % (fam, mode, dev_e, dev_q, dev_n, dev_x))
    ok = [record_bound("sync axes %s %d: eps vs float64 model" % (fam, mode), dev_e, _bar(WORST_EPS)),
          record_bound("sync axes %s %d: quality vs float64 model" % (fam, mode), dev_q, _bar(WORST_QUALITY)),
          record_bound("sync axes %s %d: null_depth vs float64 model" % (fam, mode), dev_n, _bar(WORST_NULL_DEPTH)),
          record_bound("sync axes %s %d: extraction rel-RMS vs float64 model" % (fam, mode), dev_x, _bar(WORST_EXTRACT))]
    assert all(ok), (dev_e, dev_q, dev_n, dev_x)


@pytest.mark.parametrize("mode", (1, 2, 3, 4))
def test_one_sample_less_than_the_shortest_capture_is_refused_through_the_device_entry(pkg, contexts, mode):
    """C (e): 2 tf + null is taken (family C, "the shortest capture"); 2 tf + null - 1 is not, and queues nothing."""
    import torch
    g = geometry(mode)
    md = contexts(mode, 2)
    d_x = torch.zeros(2 * g["tf"] + g["null"] - 1, dtype=torch.complex64, device="cuda")
    with pytest.raises(pkg.DabGpuError) as e:
        md.sync_dev(d_x, SY.MAX_SHIFT)
    assert "too short" in str(e.value)
