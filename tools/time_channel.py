#!/usr/bin/env python3
"""What the channel emulator costs (channel.hip): one channel_dev call on 2^24 samples.

Device buffers, HIP events, ONE process on one box: 1 / 4 / 16 / 64 paths (seeded delays 0 ... 2047 and gains), static and with
a Doppler on every path, noise off and on, complexf in and out; one path with noise, s16 in and out, once.  A call is two
launches (the samples, the 2047 samples of history).  Each line gives the time and the rate of the compulsory traffic, 8 B read
+ 8 B written per sample (4 + 4 for s16), next to the box's copy rate that DESIGN 6 records (4.8 TB/s).  No rate is asked for
and none is held; the figures are one run on one box.  Method as in tools/time_gpu_frontend.py (warm-up by time, five
repetitions, the median and the spread).  Nothing is asserted.

usage (GPU box): python tools/time_channel.py >> profiles/channel.txt   (behind the operating point's search, which
tests/test_channel_cpu.py reads there)"""
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
N = 1 << 24
COPY_TBS = 4.8


def paths(n, doppler):
    rs = np.random.RandomState(n)
    delays = rs.randint(0, 2048, n)
    delays[0] = 0
    gains = (rs.standard_normal(n) + 1j * rs.standard_normal(n)) / np.sqrt(2.0 * n)
    hz = rs.uniform(-200.0, 200.0, n) if doppler else np.zeros(n)
    return [(int(d), complex(g), float(f)) for d, g, f in zip(delays, gains, hz)]


def main():
    print("device: " + torch.cuda.get_device_name(0))
    print("the channel emulator, %d samples per call; device buffers, HIP events; one process, one run on one box; the box's copy"
          " rate (DESIGN 6): %.1f TB/s" % (N, COPY_TBS))
    dev = torch.device("cuda", 0)
    side = torch.cuda.Stream(device=dev)
    s = side.cuda_stream
    md = P.Modulator(mode=1, max_frames=1)
    md.trace(True)
    with torch.cuda.stream(side):
        d_x = torch.view_as_complex(torch.randn((N, 2), dtype=torch.float32, device=dev))
        d_y = torch.empty(N, dtype=torch.complex64, device=dev)
        d_q = (torch.view_as_real(d_x) * 8000.0).round().to(torch.int16).reshape(-1)
        d_r = torch.empty(2 * N, dtype=torch.int16, device=dev)
        torch.cuda.synchronize()

        def line(tag, d_in, d_out, traffic):
            t, lo, hi, calls = timed_device(lambda: md.channel_dev(d_in, d_out, stream=s), side)
            print("  %-34s %9.1f us per call  (median of 5 x %d calls: %.1f ... %.1f us)  %.2f TB/s of %.0f MB compulsory traffic"
                  " (%.0f %% of the copy rate)\n      kernels: %s"
                  % (tag, t * 1e6, calls, lo * 1e6, hi * 1e6, traffic / t * 1e-12, traffic * 1e-6, 100.0 * traffic / t * 1e-12 / COPY_TBS,
                     "; ".join(md.last_variant())), flush=True)

        for n in (1, 4, 16, 64):
            for doppler in (False, True):
                for sigma in (0.0, 0.5):
                    md.set_channel(paths(n, doppler), sigma, 1)
                    line("%2d paths, %s, noise %s" % (n, "Doppler" if doppler else "static ", "on" if sigma else "off"), d_x, d_y, 16.0 * N)
        md.set_channel(paths(1, False), 100.0, 1)
        line(" 1 path, static, noise on, s16", d_q, d_r, 8.0 * N)
        side.synchronize()
        print("  stream position after the run: %d" % md.channel_position())
    md.close()


if __name__ == "__main__":
    main()
