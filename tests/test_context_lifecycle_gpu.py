"""A context that has used every receive-side stage, and a lane beside lane 0, is destroyed and built again: the second
one computes what the first did.  Every device buffer of a context frees itself when the context goes (DevBuf, csrc/devbuf.h);
this is the run in which each of them holds memory at that moment."""
import numpy as np
import pytest

from tests.golden.synth import synth_bits

pytestmark = pytest.mark.gpu

N_FRAMES = 4


def _one_context(pkg):
    """Mode II, four frames: the context's own chain output through every stage once -> what it computed, by name"""
    import torch
    md = pkg.Modulator(mode=2, max_frames=N_FRAMES)
    try:
        g = md.geometry
        guard = g["sym_size"] - g["spacing"]
        md.set_tii(True, comb=3, pattern=11)
        stages = pkg.STAGE_GAIN | pkg.STAGE_FIR                       # (native rate, complexf)
        bits = synth_bits(N_FRAMES * g["tf_input_bytes"], seed=7).reshape(N_FRAMES, -1)
        capture = np.array(md.chain(bits, stages)).reshape(-1)
        got = {"capture": capture.tobytes()}

        md.sync(capture)
        got["sync"] = md.sync_result_bytes()
        got["extract"] = md.sync_extract(capture).tobytes()
        md.tii_scan(capture, early=(g["null_size"] - g["spacing"]) // 2)
        got["tii_scan"] = md.tii_scan_result_bytes()
        md.cir(capture, early=guard // 2)
        got["cir"] = md.cir_result_bytes()
        md.set_channel([(0, 1.0 + 0.0j, 0.0)], sigma=0.0)
        got["channel"] = md.channel(capture).tobytes()
        got["demod"] = md.demod(capture, early=guard // 2).tobytes()
        soft, soft_bits = md.demod_soft(capture, early=guard // 2, want_bits=True)
        got["demod_soft"] = soft.tobytes() + soft_bits.tobytes()
        md.spectrum(capture)
        st = md.spectrum_stats()
        got["spectrum"] = st["raw"].tobytes() + st["segments"].to_bytes(8, "little")

        # two calls on the context's own stream rotate over the lanes: lane 1 holds scratch when the context dies
        md.set_lanes(3)
        d_bits = torch.from_numpy(bits).cuda()
        d_out = torch.empty((N_FRAMES, md.out_samples_per_frame(stages)), dtype=torch.complex64, device="cuda")
        for call in range(2):
            md.chain_dev(d_bits, N_FRAMES, stages, d_out)
            got["chain_dev %d" % call] = d_out.cpu().numpy().tobytes()
        assert md.lanes_info()[0] >= 2
        return got
    finally:
        md.close()


def test_context_lifecycle_with_every_stage(pkg):
    """sync, sync_extract, tii_scan, cir, channel, demod, demod_soft and spectrum once each on four Mode II frames of the
    context's own output, then two chain calls over three lanes; the context is closed, a second one repeats the run.  Every
    result of the second pass EQUALS the first byte for byte: the stages sum in a fixed order, so a fresh context on the
    same input has nothing to differ by."""
    first = _one_context(pkg)
    second = _one_context(pkg)
    assert sorted(first) == sorted(second)
    for name in sorted(first):
        assert len(first[name]) > 0, name
        assert first[name] == second[name], name
    assert len(first["sync"]) > 0 and any(first["demod"])
