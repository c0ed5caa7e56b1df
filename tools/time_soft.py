#!/usr/bin/env python3
"""What soft decisions cost (demod.hip, decode.hip): the soft calls next to the hard ones, in the same run.

Mode I, device buffers, HIP events, ONE process:
  - demod_soft_dev next to demod_dev on the cfg 3 chain's complexf output at early 44, bits stored, at 16 / 256 / 4096 frames
    per call.  Compulsory traffic per frame: 1 572 864 B read + 28 800 B of bits, and 230 400 B of softs in the soft call.
  - decode_soft_dev next to decode_dev for cfg 1, `multi`, `full_cif` and `nst0` at 4 / 64 / 1024 ETI frames per call, with
    the bound on the time of one trellis step of tools/time_decode.py (the call at 4 frames over the longest unit's steps).
    The softs are +-64 of the CPU front-end's bits: the decoder's work does not depend on the data.
The file ends with the operating point tests/test_soft_cpu.py finds on the numpy models (tests/soft_cases.py), which
tests/test_soft_gpu.py runs on the device.

Method as in tools/time_gpu_frontend.py (warm-up by time, five repetitions, the median and the spread).  Nothing is asserted.

usage (GPU box): python tools/time_soft.py > profiles/soft.txt"""
import importlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from time_gpu_frontend import timed_device  # noqa: E402
from tests import soft_cases as SC  # noqa: E402
from tests.golden.frontend_cases import ETI_CASES  # noqa: E402
from tests.golden.synth import synth_eti  # noqa: E402

P = importlib.import_module("odr-dabmod_amd")
CFG3 = P.STAGE_GAIN | P.STAGE_FIR
BATCHES = (16, 256, 4096)
LAYOUTS = (("cfg1", ((0, 48, 0x22),)), ("multi", ETI_CASES["multi"]["kw"]["subchannels"]), ("full_cif", ((0, 432, 0x22),)),
           ("nst0", ()))
FRAMES = (4, 64, 1024)


def demod_part(dev, side):
    s = side.cuda_stream
    print("the receiver, Mode I, cfg 3 output, early 44, bits stored: hard (demod_dev) and soft (demod_soft_dev)")
    print("%8s %12s %12s %8s %14s %14s" % ("frames", "hard us", "soft us", "soft/hard", "hard frames/s", "soft frames/s"))
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
        th, hlo, hhi, _ = timed_device(lambda: md.demod_dev(d_iq, B, 44, d_dec, d_bits, stream=s), side)
        ts, slo, shi, _ = timed_device(lambda: md.demod_soft_dev(d_iq, B, d_soft, 44, d_dec, d_bits, stream=s), side)
        print("%8d %12.1f %12.1f %8.3f %14.0f %14.0f   (hard %.1f ... %.1f, soft %.1f ... %.1f us)"
              % (B, th * 1e6, ts * 1e6, ts / th, B / th, B / ts, hlo * 1e6, hhi * 1e6, slo * 1e6, shi * 1e6), flush=True)
        md.close()
        del d_bits, d_iq, d_dec, d_soft
        torch.cuda.empty_cache()


def decode_part(dev, side):
    s = side.cuda_stream
    fe = importlib.import_module("odr-dabmod_amd.frontend").Frontend()
    print("the channel decoder, Mode I, with reference frames: hard (decode_dev) and soft (decode_soft_dev)")
    print("%-9s %6s %8s %11s %11s %9s %14s %14s" % ("layout", "units", "frames", "hard s", "soft s", "soft/hard", "hard ns/step", "soft ns/step"))
    for name, subs in LAYOUTS:
        eti = synth_eti(64, subchannels=subs, mid=1)
        bits = fe.eti_to_bits(eti, 1)
        steps = max([8 * 96 + 6] + [64 * sub[1] + 6 for sub in subs])
        md = P.Modulator(mode=1, max_frames=FRAMES[-1] // 4)
        md.frontend_configure(eti[0])
        for n in FRAMES:
            reps = (n + 63) // 64
            with torch.cuda.stream(side):
                d_bits = torch.from_numpy(np.tile(bits, (reps, 1))[:n // 4].copy()).to(dev)
                d_ref = torch.from_numpy(np.tile(eti, (reps, 1))[:n].copy()).to(dev)
                d_out = torch.empty(n * 6144, dtype=torch.uint8, device=dev)
                # +-64 of the same bits, eight per byte, MSB first
                shifts = torch.arange(7, -1, -1, dtype=torch.uint8, device=dev)
                d_soft = ((((d_bits.reshape(-1, 1) >> shifts) & 1).to(torch.int8) * 2 - 1) * 64).reshape(-1).contiguous()
            side.synchronize()
            th = timed_device(lambda: md.decode_dev(d_bits, n // 4, d_out, d_ref, stream=s), side)[0]
            ts = timed_device(lambda: md.decode_soft_dev(d_soft, n // 4, d_out, d_ref, stream=s), side)[0]
            per = ("%14.1f %14.1f" % (th / steps * 1e9, ts / steps * 1e9)) if n == FRAMES[0] else ""
            print("%-9s %6d %8d %11.3e %11.3e %9.3f %s" % (name, 1 + len(subs), n, th, ts, ts / th, per), flush=True)
            del d_bits, d_ref, d_out, d_soft
        md.close()
        torch.cuda.empty_cache()


def main():
    print("device: " + torch.cuda.get_device_name(0))
    print("soft decisions next to hard ones; device buffers, HIP events; one process; one run on one box")
    dev = torch.device("cuda", 0)
    side = torch.cuda.Stream(device=dev)
    demod_part(dev, side)
    decode_part(dev, side)
    print("not measured: hardware counters, occupancy, the gather of the punctured softs against the forward pass")
    print("where soft beats hard, found on the numpy models by tests/test_soft_cpu.py (Mode II, 18 frames, FIC + 24 CU at 3-A, cfg 3,")
    print("noise seeds %s tried in order; L = the highest C/N in 0.5 dB steps with a hard payload bit error in every returned frame):"
          % ", ".join(map(str, SC.OP_SEEDS_TRIED)))
    print("operating point: seed %d, L = %.1f dB" % (SC.OP_SEED, SC.OP_LEVEL_DB))


if __name__ == "__main__":
    main()
