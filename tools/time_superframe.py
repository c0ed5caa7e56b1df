#!/usr/bin/env python3
"""What the superframe reader costs (superframe.hip), and the noisy point of its loop test.

Device buffers, HIP events, ONE process on one box; method as in tools/time_gpu_frontend.py (warm-up by time, five repetitions,
the median and the spread).  Nothing is asserted, no rate is asked for.
  (a) superframe_dev on 2048 images (2044 candidates, superframes from image 0 on) for s = 4 and s = 24: clean; every word of every
      superframe with 5 byte errors; random bytes (every word uncorrectable).  Only every fifth candidate is a superframe: the
      other four are mixtures of two, whose words are uncorrectable whatever the case -- the fivefold work the stage does by design.
  (b) beside it decode_soft_dev on a batch of the same 2048 ETI frames in Mode II with one sub-channel of that size (random int8
      metrics: the Viterbi's work does not depend on them), and decode_rs_char of the reference's lib/fec on one core on the
      clean and on the 5-error words of one candidate in five (where oracle/_ref was built), for scale.
  --sweep: the loop of tests/test_superframe_gpu.py (tests/superframe_cases.Loop) from 6 dB C/N down in 0.25 dB steps at the
      channel emulator's seed tests/superframe_cases.LOOP_SEED: payload bit errors behind decode_soft, RS bytes corrected, the
      most in one word, words failed, AUs ok / bad.  The test's point is the highest C/N with bit errors and at most 3
      corrections in any word.

usage (GPU box): python tools/time_superframe.py [--sweep] >> profiles/superframe.txt"""
import importlib
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from time_gpu_frontend import timed_device  # noqa: E402

from tests import superframe_cases as SC  # noqa: E402
from tests import superframe_model as SM  # noqa: E402
from tests.golden.synth import synth_eti  # noqa: E402

P = importlib.import_module("odr-dabmod_amd")
N_IMAGES = 2048


def inputs(s, offset):
    """clean, five errors per word, random: (n, 6144) uint8 each"""
    clean, placed = SM.stream_images(N_IMAGES, s, offset, 0, seed=s, fill="zero")
    rs = np.random.RandomState(50 + s)
    five = clean.copy()
    for f, _ in placed:
        sub = np.zeros(SM.N * s, np.uint8)
        for i in range(s):
            sub[i + s * rs.permutation(SM.N)[:5]] = rs.randint(1, 256, 5)
        five[f:f + 5, offset:offset + 24 * s] ^= sub.reshape(5, 24 * s)
    noise = rs.randint(0, 256, clean.shape).astype(np.uint8)
    return clean, five, noise, placed


def libfec_seconds(images, placed, s, offset):
    import oracle as O
    if not O.have_ref():
        return None
    fec = SC.Libfec()
    words = []
    for f, _ in placed[:100]:
        buf = images[f:f + 5, offset:offset + 24 * s].tobytes()
        words += [buf[i::s] for i in range(s)]
    t0 = time.perf_counter()
    for w in words:
        fec.decode(w)
    return (time.perf_counter() - t0) / len(words)


def timing():
    print("device: " + torch.cuda.get_device_name(0))
    print("the superframe reader, %d images per call, device buffers, HIP events; one process, one run on one box" % N_IMAGES)
    dev = torch.device("cuda", 0)
    side = torch.cuda.Stream(device=dev)
    h = side.cuda_stream
    for s in (4, 24):
        stl = 3 * s
        eti = synth_eti(4, subchannels=((0, stl, 0x22),), mid=2, seed=1)
        md = P.Modulator(mode=2, max_frames=N_IMAGES)
        md.frontend_configure(eti[0])
        md.trace(True)
        offset = P.Modulator.frontend_describe(eti[0])["subchannels"][0]["offset"]
        clean, five, noise, placed = inputs(s, offset)
        d_out = torch.zeros((N_IMAGES - 4) * 110 * s, dtype=torch.uint8, device=dev)
        print("s = %d (%d kbit/s), %d candidates, %d words per call:" % (s, 8 * s, N_IMAGES - 4, (N_IMAGES - 4) * s))
        for name, images in (("clean", clean), ("5 errors per word", five), ("random bytes", noise)):
            d = torch.from_numpy(images).to(dev)
            with torch.cuda.stream(side):
                t, lo, hi, calls = timed_device(lambda: md.superframe_dev(d, N_IMAGES, offset, 24 * s, d_out, stream=h), side)
                side.synchronize()
            res = md.superframe_result()
            print("  %-18s superframe_dev %9.1f us per call  (median of 5 x %d calls: %.1f ... %.1f us)  %d superframes, %d RS bytes"
                  " corrected, %d words failed, AUs %d ok / %d bad" % (name, t * 1e6, calls, lo * 1e6, hi * 1e6, res["superframes"],
                                                                       res["rs_corrected"], res["rs_failed"], res["aus_ok"], res["aus_bad"]), flush=True)
            if name != "random bytes":
                per = libfec_seconds(images, placed, s, offset)
                if per is not None:
                    print("  %-18s decode_rs_char, one core, through ctypes: %.2f us per word; the %d words of the in-phase candidates"
                          " %.0f us, the fivefold %.0f us" % ("", per * 1e6, len(placed) * s, per * 1e6 * len(placed) * s,
                                                             per * 1e6 * (N_IMAGES - 4) * s))
        print("      kernels: %s" % "; ".join(md.last_variant()))
        per = md.geometry["tf_input_bytes"]
        d_soft = torch.randint(-127, 128, (N_IMAGES, 8 * per), dtype=torch.int8, device=dev)
        d_img = torch.zeros(N_IMAGES * 6144, dtype=torch.uint8, device=dev)
        with torch.cuda.stream(side):
            t, lo, hi, calls = timed_device(lambda: md.decode_soft_dev(d_soft, N_IMAGES, d_img, stream=h), side)
            side.synchronize()
        print("  decode_soft_dev on %d ETI frames of this layout: %9.1f us per call  (median of 5 x %d calls: %.1f ... %.1f us)"
              % (N_IMAGES, t * 1e6, calls, lo * 1e6, hi * 1e6), flush=True)
        md.close()
        del d_soft, d_img, d_out
        torch.cuda.empty_cache()


def sweep():
    eti, placed = SC.loop_stream()
    lp = SC.Loop(P, eti)
    print("the loop of tests/test_superframe_gpu.py: Mode II, %d ETI frames, one 32 kbit/s EEP 3-A sub-channel, superframes from frame"
          " %d on; channel seed %d; 30 images behind the lead-in, 5 superframes, 30 AUs" % (SC.LOOP_FRAMES, SC.LOOP_PHASE, SC.LOOP_SEED))
    print("  C/N dB  payload bit errors  superframes  RS corrected  most in a word  words failed  AUs ok / bad")
    cn = 6.0
    while cn >= 2.0:
        got = lp.run(cn, SC.LOOP_SEED)
        r = got["result"]
        print("  %6.2f  %18d  %11d  %12d  %14d  %12d  %6d / %d" % (cn, got["bit_errors"], r["superframes"], r["rs_corrected"], r["rs_max"],
                                                                    r["rs_failed"], r["aus_ok"], r["aus_bad"]), flush=True)
        cn -= 0.25
    lp.close()


if __name__ == "__main__":
    sweep() if "--sweep" in sys.argv else timing()
