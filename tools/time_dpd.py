#!/usr/bin/env python3
"""What the DPD measurement's two kernels cost (dpd.hip).

Mode I frames of 196 608 samples, 1 / 16 / 256 frames per call in ONE process, device buffers, HIP events; tx complexf and
s16, rx complexf (a scaled copy of tx plus noise: the content does not change the work):
  - dpd_xspectrum_dev (dpd_xspectrum_kernel + dpd_xspectrum_reduce_kernel) at rx_offset 7,
  - dpd_measure_dev (dpd_stats_kernel) with lag 7, tau 0.37, 64 bins,
each against its compulsory traffic: the bytes of tx and rx (8 or 4, plus 8, per sample).
A cost only: no rate is asked for and none is held.  Method as in tools/time_gpu_frontend.py (warm-up by time, five
repetitions, the median and the spread).  Nothing is asserted.

usage (GPU box): python tools/time_dpd.py > profiles/dpd.txt"""
import importlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

from time_gpu_frontend import timed_device  # noqa: E402

P = importlib.import_module("odr-dabmod_amd")
BATCHES = (1, 16, 256)
SAMPLES = 196608


def main():
    print("device: " + torch.cuda.get_device_name(0))
    print("the DPD measurement's kernels, Mode I frames; device buffers, HIP events; one process")
    dev = torch.device("cuda", 0)
    side = torch.cuda.Stream(device=dev)
    s = side.cuda_stream
    al = {"lag": 7, "tau": 0.37, "gain": 1.25 - 0.1j}
    for B in BATCHES:
        n = B * SAMPLES
        print("%d frames per call (%d samples)" % (B, n))
        with torch.cuda.stream(side):
            g = torch.Generator(device=dev).manual_seed(7)
            x = torch.randn(n, 2, device=dev, generator=g) * 0.18
            rx = torch.view_as_complex((0.8 * x + 1e-3 * torch.randn(n, 2, device=dev, generator=g)).contiguous())
            for name, tx, bytes_per, peak in (("complexf", torch.view_as_complex(x.contiguous()), 8, 0.75),
                                              ("s16", (x * 20000.0).round().to(torch.int16).reshape(-1), 4, 15000.0)):
                md = P.Modulator(mode=1, max_frames=1)
                md.trace(True)
                traffic = n * (bytes_per + 8)
                for tag, step in (("cross-spectrum", lambda: md.dpd_xspectrum_dev(tx, rx, 7, stream=s)),
                                  ("statistics", lambda: md.dpd_measure_dev(tx, rx, al, peak, 64, stream=s))):
                    t, lo, hi, calls = timed_device(step, side)
                    print("  %-15s tx %-8s %9.1f us per call  (median of 5 x %d calls: %.1f ... %.1f us)  %.0f GB/s of %.1f MB "
                          "compulsory input\n      kernels: %s" % (tag, name, t * 1e6, calls, lo * 1e6, hi * 1e6, traffic / t * 1e-9,
                                                                    traffic * 1e-6, "; ".join(md.last_variant())), flush=True)
                side.synchronize()
                st = md.dpd_stats()
                print("      segments %d; samples used %d, above the peak %d" % (md.dpd_xspectrum_result()["segments"],
                                                                                  st["samples_used"], st["overflow"]))
                md.close()
            del x, rx
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
