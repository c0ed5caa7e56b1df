#!/usr/bin/env python3
"""What the carrier state costs (demod.hip): demod_csi_dev next to demod_soft_dev, in the same run.

Mode I, device buffers, HIP events, ONE process: both calls on the cfg 3 chain's complexf output at early 44, bits stored, at
16 / 256 / 4096 frames per call; besides them the state alone (demod_carrier_state_dev: the first transform pass and the
weights), which with demod_soft_dev's time makes up the weighted call.  Compulsory traffic per frame: the capture read twice
(2 x 1 572 864 B), 28 800 B of bits, 230 400 B of softs, 24 576 B of sums written and read, 6 144 B of weights.

Method as in tools/time_gpu_frontend.py (warm-up by time, five repetitions, the median and the spread).  Nothing is asserted.
The text above the table in profiles/csi.txt (the searches of tests/test_csi_cpu.py) is not this tool's.

usage (GPU box): python tools/time_csi.py >> profiles/csi.txt"""
import importlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from time_gpu_frontend import timed_device  # noqa: E402

P = importlib.import_module("odr-dabmod_amd")
CFG3 = P.STAGE_GAIN | P.STAGE_FIR
BATCHES = (16, 256, 4096)


def main():
    print("device: " + torch.cuda.get_device_name(0))
    print("weighted softs next to unweighted ones; device buffers, HIP events; one process; one run on one box; median of 5 repetitions")
    dev = torch.device("cuda", 0)
    side = torch.cuda.Stream(device=dev)
    s = side.cuda_stream
    print("the receiver, Mode I, cfg 3 output, early 44, bits stored: demod_soft_dev, demod_csi_dev, demod_carrier_state_dev")
    print("%8s %12s %12s %12s %9s %14s" % ("frames", "soft us", "csi us", "state us", "csi/soft", "csi frames/s"))
    for B in BATCHES:
        md = P.Modulator(mode=1, max_frames=B)
        md.set_gain(2, 1.0, 1 / 50000.0, 4.0)
        md.set_fir_taps(None)
        g = md.geometry
        with torch.cuda.stream(side):
            bits = np.random.RandomState(7).randint(0, 256, B * g["tf_input_bytes"]).astype(np.uint8)
            d_bits = torch.from_numpy(bits).to(dev)
            d_iq = torch.empty((B, md.out_samples_per_frame(CFG3)), dtype=torch.complex64, device=dev)
            d_dec = torch.empty(B * g["tf_input_bytes"], dtype=torch.uint8, device=dev)
            d_soft = torch.empty(8 * B * g["tf_input_bytes"], dtype=torch.int8, device=dev)
            md.chain_dev(d_bits, B, CFG3, d_iq, stream=s)
        side.synchronize()
        ts, slo, shi, _ = timed_device(lambda: md.demod_soft_dev(d_iq, B, d_soft, 44, d_dec, d_bits, stream=s), side)
        tc, clo, chi, _ = timed_device(lambda: md.demod_csi_dev(d_iq, B, d_soft, 44, d_dec, d_bits, stream=s), side)
        tp, plo, phi, _ = timed_device(lambda: md.demod_carrier_state_dev(d_iq, B, 44, stream=s), side)
        print("%8d %12.1f %12.1f %12.1f %9.3f %14.0f   (soft %.1f ... %.1f, csi %.1f ... %.1f, state %.1f ... %.1f us)"
              % (B, ts * 1e6, tc * 1e6, tp * 1e6, tc / ts, B / tc, slo * 1e6, shi * 1e6, clo * 1e6, chi * 1e6, plo * 1e6, phi * 1e6), flush=True)
        md.close()
        del d_bits, d_iq, d_dec, d_soft
        torch.cuda.empty_cache()
    print("not measured: the form that leaves unclamped metrics in scratch for an elementwise second pass (not built); hardware counters")


if __name__ == "__main__":
    main()
