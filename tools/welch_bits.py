#!/usr/bin/env python3
"""The bits of the two Welch measurements (spectrum.hip, dpd.hip; welch.h), for comparing two builds: SHA-256 of
spectrum_stats()["raw"] and of the cross-spectrum's S, p_tx, p_rx on the inputs of tests/spectrum_cases.py and
tests/dpd_cases.py.  Spectrum: every format x window, at the default run length and at 7 segments per run.  DPD: complexf and
s16 tx at rx_offset 7 and -300, at the default run length and at 7.  Only the public Python API; nothing is asserted.  The
digests depend on nothing but the kernels' arithmetic and the order of their sums: two builds that print the same list
compute the same bits (profiles/welch_refactor.txt, part 2).

usage (GPU box): python tools/welch_bits.py"""
import hashlib
import importlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from tests import dpd_cases as DC  # noqa: E402
from tests import spectrum_cases as SC  # noqa: E402

P = importlib.import_module("odr-dabmod_amd")
MODE = {"cf32": 1, "s16": 2, "u8": 3, "s8": 4}       # Mode I reads the context's own twiddle table, the others the built one


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:32]


def main():
    cuda = lambda a: torch.from_numpy(np.array(a)).cuda()
    for fmt in SC.FORMATS:
        md = P.Modulator(mode=MODE[fmt], max_frames=1)
        d = cuda(SC.samples(fmt))
        for run in (0, 7):
            md.set_spectrum_run_segments(run)
            for window in SC.WINDOWS:
                md.spectrum_dev(d, window)
                st = md.spectrum_stats()
                print("spectrum %-4s window %d run %d: %d segments  raw %s" % (fmt, window, run, st["segments"], digest(st["raw"])))
        md.close()
    d_rx = cuda(DC.capture(0.37))
    for fmt in ("cf32", "s16"):
        md = P.Modulator(mode=MODE[fmt], max_frames=1)
        d_tx = cuda(DC.block() if fmt == "cf32" else DC.block_s16())
        for run in (0, 7):
            md.set_dpd_geometry(run_segments=run)
            for off in (7, -300):
                md.dpd_xspectrum_dev(d_tx, d_rx, off)
                x = md.dpd_xspectrum_result()
                print("dpd %-4s offset %4d run %d: %d segments  S %s  p_tx %s  p_rx %s"
                      % (fmt, off, run, x["segments"], digest(x["S"]), digest(x["p_tx"]), digest(x["p_rx"])))
        md.close()


if __name__ == "__main__":
    main()
