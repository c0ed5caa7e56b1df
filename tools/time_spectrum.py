#!/usr/bin/env python3
"""What the spectrum monitor costs (spectrum.hip): the two kernels alone and chain calls with and without it.

Mode I, 16 / 256 / 4096 frames per call in ONE process, device buffers, HIP events:
  - spectrum_dev on a chain's output, complexf and s16, Blackman-Harris window, against its compulsory traffic: the input
    bytes (196 608 samples x 8 resp. 4 B per frame); what the kernels write (16 KiB per workgroup, 16 KiB of sums) is not
    counted.  Next to it stands profiles/demod.txt: demod_kernel reads the same complexf bytes.
  - the cfg 3 (gain var + FIRFilter) and cfg 4 (+ Resampler x4 + MemlessPoly) chain calls with the spectrum monitor off and on
    (same context settings otherwise; the trace names the launches).
Then the two accuracy figures of tests/test_spectrum_gpu.py for every format x window, formed here against the same model.

Method as in tools/time_gpu_frontend.py (warm-up by time, five repetitions, the median and the spread).  Nothing is asserted.

usage (GPU box): python tools/time_spectrum.py > profiles/spectrum.txt"""
import importlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from time_gpu_frontend import timed_device  # noqa: E402
from tests.golden.synth import POLY_AM, POLY_PM  # noqa: E402

P = importlib.import_module("odr-dabmod_amd")
CFG3 = P.STAGE_GAIN | P.STAGE_FIR
CFG4 = CFG3 | P.STAGE_RESAMPLE | P.STAGE_POLY
BATCHES = (16, 256, 4096)
SAMPLES = 196608


def context(frames, spectrum, cfg4=False, fmt=None):
    md = P.Modulator(mode=1, max_frames=frames)
    md.set_gain(2, 1.0, 1.0 if fmt else 1 / 50000.0, 4.0)
    md.set_fir_taps(None)
    if cfg4:
        md.set_resampler(2048000, 8192000)
        md.set_poly(POLY_AM, POLY_PM)
    if fmt:
        md.set_output_format(fmt)
    md.set_spectrum_monitor(spectrum, 2)
    md.trace(True)
    return md


def accuracy():
    """The two figures of tests/test_spectrum_gpu.py, test 1, on its signal: every format x window against the float64 model."""
    from tests import spectrum_cases as SC
    from tests import spectrum_model as SM
    print("accuracy against the float64 model (tests/spectrum_model.py) on the synthetic signal, 79 segments:")
    print("  (a) max |dev - model| / model over bins >= 1e-4 max;  (b) max |dev - model| / (model + 1e-9 mean) over all bins")
    md = P.Modulator(mode=1, max_frames=1)
    worst = [0.0, 0.0]
    for fmt in SC.FORMATS:
        for window in SC.WINDOWS:
            md.spectrum(SC.samples(fmt), window)
            dev = md.spectrum_stats()["raw"]
            model, _ = SM.welch_raw(SC.samples(fmt), P.spectrum_window(window))
            err = np.abs(dev - model)
            strong = model >= 1e-4 * model.max()
            a, b = float(np.max(err[strong] / model[strong])), float(np.max(err / (model + 1e-9 * model.mean())))
            worst = [max(worst[0], a), max(worst[1], b)]
            print("  %-5s window %d   (a) %.3e   (b) %.3e" % (fmt, window, a, b))
    md.close()
    print("  worst             (a) %.3e   (b) %.3e" % tuple(worst))


def main():
    print("device: " + torch.cuda.get_device_name(0))
    print("the spectrum monitor, Mode I, Blackman-Harris window; device buffers, HIP events; one process")
    dev = torch.device("cuda", 0)
    side = torch.cuda.Stream(device=dev)
    s = side.cuda_stream
    for B in BATCHES:
        print("%d frames per call" % B)
        with torch.cuda.stream(side):
            bits = np.random.RandomState(7).randint(0, 256, B * 28800).astype(np.uint8)
            d_bits = torch.from_numpy(bits).to(dev)

            def line(tag, md, step, traffic=None):
                t, lo, hi, calls = timed_device(step, side)
                extra = ""
                if traffic:
                    extra = "  %.0f GB/s of %.1f MB compulsory input per call" % (traffic / t * 1e-9, traffic * 1e-6)
                print("  %-40s %9.1f us per call  %10.0f frames/s  (median of 5 x %d calls: %.1f ... %.1f us)%s\n      kernels: %s"
                      % (tag, t * 1e6, B / t, calls, lo * 1e6, hi * 1e6, extra, "; ".join(md.last_variant())), flush=True)
                return t

            for fmt, dtype, width, bytes_per in ((None, torch.complex64, 1, 8), ("s16", torch.int16, 2, 4)):
                md = context(B, False, fmt=fmt)
                d_iq = torch.empty((B, width * SAMPLES), dtype=dtype, device=dev)
                md.chain_dev(d_bits, B, CFG3, d_iq, stream=s)
                side.synchronize()
                line("spectrum alone, %s" % (fmt or "complexf"), md, lambda: md.spectrum_dev(d_iq, 2, stream=s),
                     traffic=B * SAMPLES * bytes_per)
                side.synchronize()
                print("      segments %d" % md.spectrum_stats()["segments"])
                md.close()
                del d_iq
            for name, stages, cfg4 in (("cfg 3", CFG3, False), ("cfg 4", CFG4, True)):
                off, on = context(B, False, cfg4), context(B, True, cfg4)
                d_iq = torch.empty((B, off.out_samples_per_frame(stages)), dtype=torch.complex64, device=dev)
                t0 = line("%s chain call, spectrum monitor off" % name, off, lambda: off.chain_dev(d_bits, B, stages, d_iq, stream=s))
                t1 = line("%s chain call, spectrum monitor on" % name, on, lambda: on.chain_dev(d_bits, B, stages, d_iq, stream=s))
                print("  the spectrum monitor adds %.1f us per %s call (%.0f %%)" % ((t1 - t0) * 1e6, name, 100.0 * (t1 - t0) / t0))
                side.synchronize()
                st = on.spectrum_stats()
                res = P.check_mask(st["raw"], st["rate_hz"])
                print("  %s: %d segments at %.0f Hz so far, out-of-band maximum %.2f dB at %.0f Hz (no threshold)"
                      % (name, st["segments"], st["rate_hz"], res["oob_max_db"], res["oob_freq_hz"]))
                off.close()
                on.close()
                del d_iq
        del d_bits
        torch.cuda.empty_cache()
    accuracy()

if __name__ == "__main__":
    main()
