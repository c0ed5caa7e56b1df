#!/usr/bin/env python3
"""What the synchroniser costs (sync.hip): one sync call and one extraction.

Mode I, a capture of 2 / 16 / 64 frames of the cfg 2 chain (start 1234, 3.37 carrier spacings off, a tail of 2 B + N samples),
complexf and s16, device buffers, HIP events, ONE process on one box:
  - sync_dev (block power, coarse start, one workgroup per candidate frame), max_shift 31;
  - sync_extract_dev, against its compulsory traffic of 8 B (4 B for s16) read + 8 B written per sample of a frame.
The records of the last call are printed so that the run shows what was timed.  No rate is asked for and none is held; the
figures are one run on one box.  Method as in tools/time_gpu_frontend.py (warm-up by time, five repetitions, the median and the
spread).  Nothing is asserted.

usage (GPU box): python tools/time_sync.py > profiles/sync.txt   (the measured deviations from the float64 model, printed by
tests/test_sync_gpu.py, are appended by hand)"""
import importlib
import math
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
START, CFO, TAIL, N, TF = 1234, 3.37, 2 * 64 + 2048, 2048, 196608


def capture(md, frames, dev, s16):
    """frames + 1 frames of the cfg 2 chain as a capture, built on the device"""
    bits = np.random.RandomState(7).randint(0, 256, (frames + 1) * md.geometry["tf_input_bytes"]).astype(np.uint8)
    d_y = torch.empty((frames + 1, TF), dtype=torch.complex64, device=dev)
    md.chain_dev(torch.from_numpy(bits).to(dev), frames + 1, 0, d_y)
    x = torch.cat([d_y[frames][TF - START:], d_y[:frames].reshape(-1), d_y[frames][:TAIL]])
    i = torch.arange(x.numel(), dtype=torch.float64, device=dev)
    x = (x.to(torch.complex128) * torch.polar(torch.ones_like(i), 2.0 * math.pi * CFO * i / N)).to(torch.complex64)
    if not s16:
        return x
    scale = 20000.0 / float(x.abs().max())
    return torch.view_as_real(x * scale).round().to(torch.int16).reshape(-1)


def main():
    print("device: " + torch.cuda.get_device_name(0))
    print("the synchroniser, Mode I, capture of the cfg 2 chain at start %d, %.2f carrier spacings off; device buffers, HIP events;"
          " one process, one run on one box" % (START, CFO))
    dev = torch.device("cuda", 0)
    side = torch.cuda.Stream(device=dev)
    s = side.cuda_stream
    for B in BATCHES:
        md = P.Modulator(mode=1, max_frames=B + 1)
        md.trace(True)
        print("%d frames per call" % B)
        for s16 in (False, True):
            d_x = capture(md, B, dev, s16)
            n = d_x.numel() // (2 if s16 else 1)
            with torch.cuda.stream(side):
                d_out = torch.empty((md.sync_slots(n), TF), dtype=torch.complex64, device=dev)
                torch.cuda.synchronize()

                def line(tag, step, traffic=None):
                    t, lo, hi, calls = timed_device(step, side)
                    extra = ""
                    if traffic:
                        extra = "  %.2f TB/s of %.1f MB compulsory traffic per call" % (traffic / t * 1e-12, traffic * 1e-6)
                    print("  %-26s %9.1f us per call  (median of 5 x %d calls: %.1f ... %.1f us)%s\n      kernels: %s"
                          % (tag, t * 1e6, calls, lo * 1e6, hi * 1e6, extra, "; ".join(md.last_variant())), flush=True)

                fmt = "s16" if s16 else "complexf"
                line("sync, " + fmt, lambda: md.sync_dev(d_x, 31, stream=s))
                line("extract, " + fmt, lambda: md.sync_extract_dev(d_x, d_out, stream=s), traffic=B * TF * (12 if s16 else 16))
                side.synchronize()
                res = md.sync_result()
                print("  found %d frames: first start %d, last start %d, shift + eps %.6f ... %.6f, quality >= %.4f, all valid %s"
                      % (len(res), res[0]["start"], res[-1]["start"], min(r["shift"] + r["eps"] for r in res),
                         max(r["shift"] + r["eps"] for r in res), min(r["quality"] for r in res), all(r["valid"] for r in res)))
            del d_x, d_out
        md.close()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
