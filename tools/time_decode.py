#!/usr/bin/env python3
"""What the channel decoder costs (decode.hip): the decode call alone.

Mode I, decode_dev on device buffers (coded bits in, ETI images out, with reference frames), 4 / 64 / 1024 ETI frames per call
in ONE process, HIP events.  Layouts: cfg 1 (one 96-CU sub-channel, EEP 3-A), `multi` (five sub-channels), `full_cif` (one
864-CU sub-channel: the longest trellis, 27 654 steps beside the FIC's 774) and `nst0` (the FIC alone).  The input is the CPU
front-end's bits of a 64-frame stream, repeated: the decoder's work does not depend on the data.  Per line: seconds per call
(median, min, max), ETI frames per second and the multiple of real time (an ETI frame is 24 ms).  The last column divides the
call's time at 4 frames by the steps of the layout's longest unit: an UPPER bound on the time of one trellis step of one wave
(the call also holds two small launches, two memsets, the history copy and the traceback).

Method as in tools/time_gpu_frontend.py (warm-up by time, five repetitions, the median and the spread).  Nothing is asserted.

usage (GPU box): python tools/time_decode.py > profiles/decode.txt"""
import importlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from time_gpu_frontend import timed_device  # noqa: E402
from tests.golden.frontend_cases import ETI_CASES  # noqa: E402
from tests.golden.synth import synth_eti  # noqa: E402

P = importlib.import_module("odr-dabmod_amd")
LAYOUTS = (("cfg1", ((0, 48, 0x22),)), ("multi", ETI_CASES["multi"]["kw"]["subchannels"]), ("full_cif", ((0, 432, 0x22),)),
           ("nst0", ()))
FRAMES = (4, 64, 1024)


def main():
    print("device: " + torch.cuda.get_device_name(0))
    print("the channel decoder, Mode I, decode_dev with reference frames; device buffers, HIP events; one process; one run on one box")
    dev = torch.device("cuda", 0)
    side = torch.cuda.Stream(device=dev)
    fe = importlib.import_module("odr-dabmod_amd.frontend").Frontend()
    print("%-9s %6s %8s %11s %11s %11s %12s %9s %14s" % ("layout", "units", "frames", "s/call", "min", "max", "ETI frames/s", "x real", "ns/step bound"))
    for name, subs in LAYOUTS:
        eti = synth_eti(64, subchannels=subs, mid=1)
        bits = fe.eti_to_bits(eti, 1)
        steps = max([8 * 96 + 6] + [64 * s[1] + 6 for s in subs])
        md = P.Modulator(mode=1, max_frames=FRAMES[-1] // 4)
        md.frontend_configure(eti[0])
        first = None
        for n in FRAMES:
            reps = (n + 63) // 64
            with torch.cuda.stream(side):
                d_bits = torch.from_numpy(np.tile(bits, (reps, 1))[:n // 4].copy()).to(dev)
                d_ref = torch.from_numpy(np.tile(eti, (reps, 1))[:n].copy()).to(dev)
                d_out = torch.empty(n * 6144, dtype=torch.uint8, device=dev)
            side.synchronize()
            med, lo, hi, calls = timed_device(lambda: md.decode_dev(d_bits, n // 4, d_out, d_ref, stream=side.cuda_stream), side)
            first = med if first is None else first
            print("%-9s %6d %8d %11.3e %11.3e %11.3e %12.0f %9.1f %14s"
                  % (name, 1 + len(subs), n, med, lo, hi, n / med, n / med * 0.024, "%.1f" % (first / steps * 1e9) if n == FRAMES[0] else ""))
        md.close()
    print("not measured: hardware counters, occupancy, the serial traceback against the forward pass")


if __name__ == "__main__":
    main()
