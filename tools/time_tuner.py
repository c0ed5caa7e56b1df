#!/usr/bin/env python3
"""What the tuner costs (tuner.hip): one tuner_dev call on 2^24 input samples, complexf in and out.

Device buffers, HIP events, ONE process on one box: 8.192 -> 2.048 MS/s wide (P = 128) and channel (P = 384), 2.4 -> 2.048 MS/s
wide (64/75, P = 64) and 10.0 -> 2.048 MS/s channel (128/625, P = 480), each with an offset, so that the mixer runs; a call is
two launches (the samples, the P - 1 samples of history).  Each line gives the time, the input rate in MS/s and how many
2.048 MS/s blocks that is in real time, next to a device-to-device copy of the same input bytes measured in the same process
on the same box.  No rate is asked for and none is held; the figures are one run on one box.  Method as in
tools/time_gpu_frontend.py (warm-up by time, five repetitions, the median and the spread).  Nothing is asserted.

usage (GPU box): python tools/time_tuner.py > profiles/tuner.txt"""
import importlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

from time_gpu_frontend import timed_device  # noqa: E402

P = importlib.import_module("odr-dabmod_amd")
N = 1 << 24
CASES = (("8.192 -> 2.048 wide", 8192000, 0, 333333.3), ("8.192 -> 2.048 channel", 8192000, 1, 333333.3),
         ("2.4 -> 2.048 wide", 2400000, 0, 123456.7), ("10.0 -> 2.048 channel", 10000000, 1, 1712000.0))


def main():
    print("device: " + torch.cuda.get_device_name(0))
    print("the tuner, %d input samples per call, complexf in and out; device buffers, HIP events; one process, one run on one box"
          % N)
    dev = torch.device("cuda", 0)
    side = torch.cuda.Stream(device=dev)
    s = side.cuda_stream
    md = P.Modulator(mode=2, max_frames=1)
    md.trace(True)
    with torch.cuda.stream(side):
        d_x = torch.view_as_complex(torch.randn((N, 2), dtype=torch.float32, device=dev))
        d_c = torch.empty_like(d_x)
        d_y = torch.empty(N + 2, dtype=torch.complex64, device=dev)
        torch.cuda.synchronize()
        t_copy, lo, hi, calls = timed_device(lambda: d_c.copy_(d_x), side)
        print("  device-to-device copy of the input   %9.1f us  (median of 5 x %d copies: %.1f ... %.1f us)  %.2f TB/s read + written"
              % (t_copy * 1e6, calls, lo * 1e6, hi * 1e6, 16.0 * N / t_copy * 1e-12), flush=True)
        for tag, rate, sel, off in CASES:
            L, M, taps = P.tuner_geometry(rate, sel)
            md.set_tuner(rate, sel, off)
            t, lo, hi, calls = timed_device(lambda: md.tuner_dev(d_x, d_y, stream=s), side)
            traffic = 8.0 * N + 8.0 * P.tuner_count(rate, sel, N)
            print("  %-24s L/M = %d/%d, P = %3d  %9.1f us per call  (median of 5 x %d calls: %.1f ... %.1f us)  %.0f MS/s in ="
                  " %.0f x real time; %.2f TB/s of %.0f MB compulsory traffic; %.1f x the copy's time\n      kernels: %s"
                  % (tag, L, M, taps, t * 1e6, calls, lo * 1e6, hi * 1e6, N / t * 1e-6, N / t / rate, traffic / t * 1e-12,
                     traffic * 1e-6, t / t_copy, "; ".join(md.last_variant())), flush=True)
        side.synchronize()
    md.close()


if __name__ == "__main__":
    main()
