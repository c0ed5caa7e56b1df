#!/usr/bin/env python3
"""What the CIC equaliser costs in the fused chain (dabgpu_set_cic_equalizer).

cfg 3 (gain var + FIRFilter), Mode I, 4096 frames per call, device buffers, HIP events:
  - from coded bits without the equaliser (one frame kernel);
  - from coded bits with it (carriers_from_bits_kernel -> the from-carriers chain);
  - the from-carriers chain by itself (dabgpu_symbols_process_dev), which is what the second line adds the carriers kernel to;
  - the carriers kernel alone (dabgpu_carriers_process_dev; the launch trace names it), against its algorithmic traffic of
    28 800 B in plus (nb_symbols + 1) x K x 8 B out per frame.

Method as in tools/time_gpu_frontend.py (warm-up by time, five repetitions, the median and the spread).  Nothing is asserted.

usage (GPU box): python tools/time_cic_chain.py > profiles/cic_chain.txt"""
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
B, CIC = 4096, (2048, 8)


def context(cic):
    md = P.Modulator(mode=1, max_frames=B)
    md.set_gain(2, 1.0, 1 / 50000.0, 4.0)
    md.set_fir_taps(None)
    if cic:
        md.set_cic_equalizer(True, *CIC)
    md.trace(True)
    return md


def main():
    print("device: " + torch.cuda.get_device_name(0))
    print("cfg 3 (gain var + FIRFilter), Mode I, %d frames per call, CicEqualizer(1536, %d, %d); device buffers, HIP events" % ((B,) + CIC))
    dev = torch.device("cuda", 0)
    side = torch.cuda.Stream(device=dev)
    off, on = context(None), context(CIC)
    g = off.geometry
    car_per = (g["nb_symbols"] + 1) * g["carriers"]
    with torch.cuda.stream(side):
        bits = np.random.RandomState(7).randint(0, 256, B * g["tf_input_bytes"]).astype(np.uint8)
        d_bits = torch.from_numpy(bits).to(dev)
        d_iq = torch.empty((B, off.out_samples_per_frame(CFG3)), dtype=torch.complex64, device=dev)
        d_car = torch.empty(B * car_per, dtype=torch.complex64, device=dev)
        rows = []

        def line(tag, md, step, traffic=None):
            t, lo, hi, calls = timed_device(step, side)
            names = "; ".join(md.last_variant())
            extra = ""
            if traffic:
                extra = "  %.2f TB/s of %.1f MB algorithmic traffic per call" % (traffic / t * 1e-12, traffic * 1e-6)
            print("  %-34s %9.1f us per call  %10.0f frames/s  (median of 5 x %d calls: %.1f ... %.1f us)%s\n      kernels: %s"
                  % (tag, t * 1e6, B / t, calls, lo * 1e6, hi * 1e6, extra, names), flush=True)
            rows.append((tag, t))

        s = side.cuda_stream
        line("coded bits, CIC off", off, lambda: off.chain_dev(d_bits, B, CFG3, d_iq, stream=s))
        line("coded bits, CIC on", on, lambda: on.chain_dev(d_bits, B, CFG3, d_iq, stream=s))
        on.carriers_dev(d_bits, B, d_car, stream=s)
        line("from carriers (CIC off context)", off, lambda: off.symbols_dev(d_car, B, CFG3, d_iq, stream=s))
        line("carriers kernel alone, CIC on", on, lambda: on.carriers_dev(d_bits, B, d_car, stream=s),
             traffic=B * (g["tf_input_bytes"] + car_per * 8))
        side.synchronize()
    t = dict(rows)
    print("  carriers kernel + from-carriers chain = %.1f us; measured together %.1f us"
          % ((t["carriers kernel alone, CIC on"] + t["from carriers (CIC off context)"]) * 1e6, t["coded bits, CIC on"] * 1e6))
    off.close()
    on.close()


if __name__ == "__main__":
    main()
