#!/usr/bin/env python3
"""What the receiver costs (demod.hip): the kernel alone and the cfg 3 chain call with and without the monitor.

Mode I, cfg 3 (gain var + FIRFilter), 16 / 256 / 4096 frames per call in ONE process, device buffers, HIP events:
  - demod_dev on the chain's complexf output at early 44, with reference bits and without a bit output (what the monitor
    runs), against its compulsory traffic of 1 572 864 B read (196 608 samples x 8 B) + 28 800 B written per frame -- the
    written figure is the bit output's, which the second line stores;
  - the same with the bit output;
  - the chain call with the monitor off, and with it on (same context settings otherwise; the trace names the launches).
Then the MER the monitor reports on the clean cfg 3, CFR and s16 outputs of five frames (tests/demod_cases.py's settings).

Method as in tools/time_gpu_frontend.py (warm-up by time, five repetitions, the median and the spread).  Nothing is asserted.

usage (GPU box): python tools/time_demod.py > profiles/demod.txt"""
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
READ, WRITTEN = 196608 * 8, 28800


def context(frames, monitor):
    md = P.Modulator(mode=1, max_frames=frames)
    md.set_gain(2, 1.0, 1 / 50000.0, 4.0)
    md.set_fir_taps(None)
    md.set_monitor(monitor)
    md.trace(True)
    return md


def clean_mer():
    print("MER the monitor reports on clean outputs, Mode I, five frames (dB per frame; no threshold):")
    bits = np.frombuffer(np.random.RandomState(701).bytes(5 * 28800), np.uint8).reshape(5, 28800)
    for name, setup in (("cfg 3", lambda md: None), ("cfg 3 + CFR (50, 0.1)", lambda md: md.set_cfr(True, 50.0, 0.1)),
                        ("cfg 3, s16 at normalise 1.0", lambda md: (md.set_gain(2, 1.0, 1.0, 4.0), md.set_output_format("s16")))):
        md = context(5, True)
        setup(md)
        md.chain(bits, CFG3)
        st = [md.monitor_stats(f) for f in range(5)]
        print("  %-30s %s   bit errors %d, worst margin %.4f"
              % (name, " ".join("%.2f" % s["mer_db"] for s in st), sum(s["bit_errors"] for s in st), min(s["min_margin"] for s in st)))
        md.close()


def main():
    print("device: " + torch.cuda.get_device_name(0))
    print("the receiver, Mode I, cfg 3 (gain var + FIRFilter), early 44; device buffers, HIP events; one process")
    dev = torch.device("cuda", 0)
    side = torch.cuda.Stream(device=dev)
    s = side.cuda_stream
    for B in BATCHES:
        off, on = context(B, False), context(B, True)
        g = off.geometry
        with torch.cuda.stream(side):
            bits = np.random.RandomState(7).randint(0, 256, B * g["tf_input_bytes"]).astype(np.uint8)
            d_bits = torch.from_numpy(bits).to(dev)
            d_iq = torch.empty((B, off.out_samples_per_frame(CFG3)), dtype=torch.complex64, device=dev)
            d_dec = torch.empty(B * g["tf_input_bytes"], dtype=torch.uint8, device=dev)
            off.chain_dev(d_bits, B, CFG3, d_iq, stream=s)
            side.synchronize()
            print("%d frames per call" % B)

            def line(tag, md, step, traffic=None):
                t, lo, hi, calls = timed_device(step, side)
                extra = ""
                if traffic:
                    extra = "  %.2f TB/s of %.1f MB compulsory traffic per call" % (traffic / t * 1e-12, traffic * 1e-6)
                print("  %-34s %9.1f us per call  %10.0f frames/s  (median of 5 x %d calls: %.1f ... %.1f us)%s\n      kernels: %s"
                      % (tag, t * 1e6, B / t, calls, lo * 1e6, hi * 1e6, extra, "; ".join(md.last_variant())), flush=True)
                return t

            line("receiver alone, errors counted", off, lambda: off.demod_dev(d_iq, B, 44, None, d_bits, stream=s), traffic=B * READ)
            line("receiver alone, bits stored", off, lambda: off.demod_dev(d_iq, B, 44, d_dec, d_bits, stream=s),
                 traffic=B * (READ + WRITTEN))
            t0 = line("chain call, monitor off", off, lambda: off.chain_dev(d_bits, B, CFG3, d_iq, stream=s))
            t1 = line("chain call, monitor on", on, lambda: on.chain_dev(d_bits, B, CFG3, d_iq, stream=s))
            print("  the monitor adds %.1f us per call (%.0f %%)" % ((t1 - t0) * 1e6, 100.0 * (t1 - t0) / t0))
            side.synchronize()
            print("  bit errors the monitor counted in the last call: %d" % sum(on.monitor_stats(f)["bit_errors"] for f in range(B)))
        off.close()
        on.close()
        del d_bits, d_iq, d_dec
        torch.cuda.empty_cache()
    clean_mer()


if __name__ == "__main__":
    main()
