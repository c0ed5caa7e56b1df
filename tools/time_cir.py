#!/usr/bin/env python3
"""What the channel estimator costs (cir.hip): one call.

Mode I, 2 / 16 / 64 frames of the cfg 3 chain, complexf and s16, early 252, Hann weights, device buffers, HIP events, ONE process
on one box: cir_dev (one workgroup per frame for the two float64 transforms of the phase reference symbol, one workgroup for
the decision).  The result of the last call is printed so that the run shows what was timed.  No rate is asked for and none is
held; the figures are one run on one box.  Method as in tools/time_gpu_frontend.py (warm-up by time, five repetitions, the
median and the spread).  Nothing is asserted.

usage (GPU box): python tools/time_cir.py > profiles/cir.txt   (the measured deviations from the float64 model, printed by
tests/test_cir_gpu.py, are appended by hand)"""
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
BATCHES = (2, 16, 64)
EARLY, TF = 252, 196608


def frames_of(md, frames, dev, s16):
    """frames of the cfg 3 chain, built on the device"""
    bits = np.random.RandomState(7).randint(0, 256, frames * md.geometry["tf_input_bytes"]).astype(np.uint8)
    d_y = torch.empty((frames, TF), dtype=torch.complex64, device=dev)
    md.chain_dev(torch.from_numpy(bits).to(dev), frames, P.STAGE_GAIN | P.STAGE_FIR, d_y)
    torch.cuda.synchronize()
    if not s16:
        return d_y
    scale = 20000.0 / float(d_y.abs().max())
    return torch.view_as_real(d_y * scale).round().to(torch.int16).reshape(frames, -1)


def main():
    print("device: " + torch.cuda.get_device_name(0))
    print("the channel estimator, Mode I, frames of the cfg 3 chain, early %d, Hann weights; device buffers, HIP events;"
          " one process, one run on one box" % EARLY)
    dev = torch.device("cuda", 0)
    side = torch.cuda.Stream(device=dev)
    s = side.cuda_stream
    for B in BATCHES:
        md = P.Modulator(mode=1, max_frames=B)
        md.set_gain(P.GAIN_VAR, 1.0, 1.0 / 50000.0, 4.0)
        md.set_fir_taps(None)
        md.trace(True)
        print("%d frames per call" % B)
        for s16 in (False, True):
            d_x = frames_of(md, B, dev, s16)
            with torch.cuda.stream(side):
                torch.cuda.synchronize()
                t, lo, hi, calls = timed_device(lambda: md.cir_dev(d_x, B, EARLY, stream=s), side)
                print("  %-26s %9.1f us per call  (median of 5 x %d calls: %.1f ... %.1f us)\n      kernels: %s"
                      % ("cir, " + ("s16" if s16 else "complexf"), t * 1e6, calls, lo * 1e6, hi * 1e6,
                         "; ".join(md.last_variant())), flush=True)
                side.synchronize()
                head, paths = md.cir_result()
                print("  n_peaks %d, floor / peak %.3g; paths: %s"
                      % (head["n_peaks"], head["floor"] / head["peak"],
                         ["delay %+.0f fine %+.3f level %.2f dB" % (p["delay"], p["fine"], 10.0 * np.log10(p["power"] / head["peak"]))
                          for p in paths]))
            del d_x
        md.close()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
