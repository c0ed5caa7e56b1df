#!/usr/bin/env python3
"""What the clock costs (clock.hip): one clock_dev call on 2^24 samples, one sco_dev call per frame in Mode I.

Device buffers, HIP events, ONE process on one box: the resampler at 0, 20 and 1000 ppm, complexf in and out, and at 20 ppm
s16 in and out; a call is two launches (the samples, the 31 samples of history).  Each line gives the time and the rate of the
compulsory traffic, 8 B read + 8 B written per sample (4 + 4 for s16), next to the box's copy rate that DESIGN 6 records
(4.8 TB/s).  The estimator: 1 and 16 Mode I frames per call (two launches), time per frame and the rate of the frames' bytes.
No rate is asked for and none is held; the figures are one run on one box.  Method as in tools/time_gpu_frontend.py (warm-up
by time, five repetitions, the median and the spread).  Nothing is asserted.

usage (GPU box): python tools/time_clock.py > profiles/clock.txt"""
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
COPY_TBS = 4.8
SCO_FRAMES = (1, 16)


def main():
    print("device: " + torch.cuda.get_device_name(0))
    print("the clock, %d samples per resampler call; device buffers, HIP events; one process, one run on one box; the box's copy"
          " rate (DESIGN 6): %.1f TB/s" % (N, COPY_TBS))
    dev = torch.device("cuda", 0)
    side = torch.cuda.Stream(device=dev)
    s = side.cuda_stream
    md = P.Modulator(mode=1, max_frames=max(SCO_FRAMES))
    md.trace(True)
    tf = md.geometry["tf_samples"]
    with torch.cuda.stream(side):
        d_x = torch.view_as_complex(torch.randn((N, 2), dtype=torch.float32, device=dev))
        d_y = torch.empty(P.clock_out_max(N), dtype=torch.complex64, device=dev)
        d_q = (torch.view_as_real(d_x) * 8000.0).round().to(torch.int16).reshape(-1)
        d_r = torch.empty(2 * P.clock_out_max(N), dtype=torch.int16, device=dev)
        torch.cuda.synchronize()

        def line(tag, call, traffic, unit="call", per=1):
            t, lo, hi, calls = timed_device(call, side)
            print("  %-34s %9.1f us per %s  (median of 5 x %d calls: %.1f ... %.1f us)  %.2f TB/s of %.0f MB compulsory traffic"
                  " (%.0f %% of the copy rate)\n      kernels: %s"
                  % (tag, t * 1e6 / per, unit, calls, lo * 1e6 / per, hi * 1e6 / per, traffic / t * 1e-12, traffic * 1e-6,
                     100.0 * traffic / t * 1e-12 / COPY_TBS, "; ".join(md.last_variant())), flush=True)

        for ppm in (0.0, 20.0, 1000.0):
            md.set_clock(ppm)
            line("resampler, %6.1f ppm, complexf" % ppm, lambda: md.clock_dev(d_x, d_y, stream=s), 16.0 * N)
        md.set_clock(20.0)
        line("resampler,   20.0 ppm, s16", lambda: md.clock_dev(d_q, d_r, stream=s), 8.0 * N)
        side.synchronize()
        print("  stream position after the run: %d" % md.clock_position())
        for n in SCO_FRAMES:
            d_f = d_x[:n * tf]
            line("estimator, Mode I, %2d frames" % n, lambda: md.sco_dev(d_f, n, 0, stream=s), 8.0 * n * tf, "frame", n)
    md.close()


if __name__ == "__main__":
    main()
