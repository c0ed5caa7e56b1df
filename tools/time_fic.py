#!/usr/bin/env python3
"""What the FIC reader costs (fic.hip): one scan, and the blind loop against the configured one.

Mode I, device buffers, HIP events, ONE process on one box.
  (a) fic_scan_dev on the decoder's output of 4 / 64 / 1024 transmission frames (16 / 256 / 4096 images, 48 / 768 / 12 288 FIBs,
      the first 45 of them the zero FIBs of the lead-in): three launches, no host round trip.
  (b) on the same coded bits of 64 transmission frames: the configured loop -- decode_dev -- and the blind loop -- decode_dev on
      a context configured with the bootstrap frame, fic_scan_dev, configure_from_fic (which waits: it reads the result on the
      host, uploads the tables and zeroes the histories), decode_dev again.  The blind loop is timed on the host clock around
      the whole sequence with a synchronise at its end, because configure_from_fic is host work; the configured loop both ways.
No rate is asked for and none is held; the figures are one run on one box, a first measurement with nothing to compare with.
Method as in tools/time_gpu_frontend.py (warm-up by time, five repetitions, the median and the spread).  Nothing is asserted.

usage (GPU box): python tools/time_fic.py > profiles/fic.txt"""
import importlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from time_gpu_frontend import timed_device, timed_host  # noqa: E402

from tests import fic_cases as FC  # noqa: E402
from tests.golden.frontend_cases import ETI_CASES  # noqa: E402
from tests.golden.synth import synth_eti  # noqa: E402

P = importlib.import_module("odr-dabmod_amd")
BATCHES = (4, 64, 1024)
MULTI = ETI_CASES["multi"]["kw"]["subchannels"]


def stream_bits(n_tf, dev):
    """(ETI frames with a real FIC, their coded bits on the device) -- the device front-end makes the bits"""
    eti = FC.with_fic(synth_eti(4 * n_tf, subchannels=MULTI, mid=1, seed=5), 1)
    md = P.Modulator(mode=1, max_frames=n_tf)
    md.frontend_configure(eti[0])
    d_bits = torch.empty(n_tf * md.geometry["tf_input_bytes"], dtype=torch.uint8, device=dev)
    md.eti_to_bits_dev(torch.from_numpy(eti).to(dev), 4 * n_tf, d_bits)
    torch.cuda.synchronize()
    md.close()
    return eti, d_bits


def main():
    print("device: " + torch.cuda.get_device_name(0))
    print("the FIC reader, Mode I, five sub-channels, a FIC with FIG 0/0, 0/1, 0/2, 1/0, 1/1 in every ETI frame; device buffers,"
          " HIP events; one process, one run on one box")
    dev = torch.device("cuda", 0)
    side = torch.cuda.Stream(device=dev)
    s = side.cuda_stream
    for B in BATCHES:
        eti, d_bits = stream_bits(B, dev)
        n = 4 * B
        rx = P.Modulator(mode=1, max_frames=B)
        rx.frontend_configure(P.fic_bootstrap_frame(1))
        rx.trace(True)
        d_out = torch.zeros(n * 6144, dtype=torch.uint8, device=dev)
        with torch.cuda.stream(side):
            rx.decode_dev(d_bits, B, d_out, stream=s)
            side.synchronize()
            t, lo, hi, calls = timed_device(lambda: rx.fic_scan_dev(d_out, n, stream=s), side)
            side.synchronize()
        res = rx.fic_result()
        print("%4d transmission frames: fic_scan_dev of %5d images %9.1f us per call  (median of 5 x %d calls: %.1f ... %.1f us)\n"
              "      kernels: %s\n      %d FIBs: %d good, %d bad, %d zero; EId 0x%04X; %d sub-channels"
              % (B, n, t * 1e6, calls, lo * 1e6, hi * 1e6, "; ".join(rx.last_variant()), res["fibs"], res["fibs_ok"], res["fibs_bad"],
                 res["fibs_zero"], res["eid"], res["n_subch"]), flush=True)
        if B == 64:
            tx = P.Modulator(mode=1, max_frames=B)
            tx.frontend_configure(eti[0])
            with torch.cuda.stream(side):
                td, lo, hi, calls = timed_device(lambda: tx.decode_dev(d_bits, B, d_out, stream=s), side)

                def configured():
                    tx.decode_dev(d_bits, B, d_out, stream=s)
                    side.synchronize()

                def blind():
                    rx.frontend_configure(P.fic_bootstrap_frame(1))
                    rx.decode_dev(d_bits, B, d_out, stream=s)
                    rx.fic_scan_dev(d_out, n, stream=s)
                    rx.configure_from_fic()
                    rx.decode_dev(d_bits, B, d_out, stream=s)
                    side.synchronize()

                th = timed_host(configured)
                tb = timed_host(blind)
            print("  64 transmission frames, the same coded bits:\n"
                  "      configured loop (decode_dev)                                %9.1f us per call between HIP events (%.1f ... %.1f),"
                  " %9.1f us on the host clock with the wait\n"
                  "      blind loop (bootstrap, decode, fic_scan, configure, decode)  %9.1f us on the host clock with the wait (%.1f ... %.1f)"
                  % (td * 1e6, lo * 1e6, hi * 1e6, th[0] * 1e6, tb[0] * 1e6, tb[1] * 1e6, tb[2] * 1e6), flush=True)
            tx.close()
        rx.close()
        del d_bits, d_out
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
