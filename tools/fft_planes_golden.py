#!/usr/bin/env python3
"""SHA-256 of the Mode I cfg 3 chain's output (coded bits -> [GainControl] -> guard -> 45-tap FIRFilter, complexf) on seeded
inputs, one digest per case and call -- the fixture behind tests/test_fft_planes_gpu.py.

The split-plane exchanges of the frame kernel's transform (csrc/fft_planes.h) move the same floats through other lanes: the
arithmetic is what it was, so the samples must be the same BYTES as before.  This tool is run once on the commit BEFORE the
change (or with DABGPU_LIB pointing at a library built from it; the Python side did not change) and its output committed:

    python tools/fft_planes_golden.py --write          # tests/golden/fft_planes_sha256.json
    python tools/fft_planes_golden.py                  # compare the library at hand with the fixture

Cases: batches of 1 and 3 frames x 1, 7 and 77 runs per frame (a run start at symbol 0, at symbol 1 and mid-frame) x gain
none / fix / var x TII off / on, two consecutive calls on one context each (with TII the second call starts on the other
parity of the frame counter when the batch is odd).
"""
import argparse
import hashlib
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "fft_planes_sha256.json")

BATCHES = (1, 3)
CHUNKS = (1, 7, 77)
GAINS = ("none", "fix", "var")
TII = (False, True)
CALLS = 2


def cases():
    return [(b, c, g, t) for b in BATCHES for c in CHUNKS for g in GAINS for t in TII]


def case_id(batch, chunks, gain, tii, call):
    return "frames%d-chunks%d-gain_%s-tii%d-call%d" % (batch, chunks, gain, int(tii), call)


def case_bits(batch, call, per):
    """Seeded coded bits of one call (every byte value occurs; the two calls of a case differ)."""
    rs = np.random.RandomState(4100 + 10 * batch + call)
    return np.frombuffer(rs.bytes(batch * per), np.uint8).reshape(batch, per)


def run_case(pkg, batch, chunks, gain, tii):
    """-> ([sha-256 per call], [kernel names per call])"""
    md = pkg.Modulator(mode=1, max_frames=batch, chunks_per_frame=chunks)
    try:
        stages = pkg.STAGE_FIR
        if gain == "fix":
            md.set_gain(pkg.GAIN_FIX, 1.0, 1.0, 4.0)
            stages |= pkg.STAGE_GAIN
        elif gain == "var":
            md.set_gain(pkg.GAIN_VAR, 1.0, 1.0 / 50000.0, 4.0)
            stages |= pkg.STAGE_GAIN
        if tii:
            md.set_tii(True, 3, 5, False)
        md.trace(True)
        digests, kernels = [], []
        for call in range(CALLS):
            y = md.chain(case_bits(batch, call, md.geometry["tf_input_bytes"]), stages)
            assert y.dtype == np.complex64 and y.shape[0] == batch, (y.dtype, y.shape)
            digests.append(hashlib.sha256(np.ascontiguousarray(y).tobytes()).hexdigest())
            kernels.append(md.last_variant())
        return digests, kernels
    finally:
        md.close()


def load_fixture():
    with open(FIXTURE) as f:
        return json.load(f)["sha256"]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--write", action="store_true", help="write the fixture instead of comparing with it")
    args = ap.parse_args()
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    pkg = importlib.import_module("odr-dabmod_amd")
    got = {}
    for b, c, g, t in cases():
        digests, _ = run_case(pkg, b, c, g, t)
        for call, d in enumerate(digests):
            got[case_id(b, c, g, t, call)] = d
    if args.write:
        with open(FIXTURE, "w") as f:
            json.dump({"what": "sha-256 of the complexf output of tools/fft_planes_golden.py's cases, written before the "
                               "split-plane FFT exchanges went in", "sha256": got}, f, indent=1, sort_keys=True)
            f.write("\n")
        print("wrote %d digests to %s" % (len(got), FIXTURE))
        return 0
    want = load_fixture()
    bad = sorted(k for k in want if got.get(k) != want[k])
    print("%d of %d cases differ from the fixture%s" % (len(bad), len(want), ": " + ", ".join(bad) if bad else ""))
    return 1 if bad or set(got) != set(want) else 0


if __name__ == "__main__":
    sys.exit(main())
