#!/usr/bin/env python3
"""One resampled stream on one context against the same stream split over 2 and 3 contexts on the same GPU
(odr-dabmod_amd/streams.py: PartitionedStream; include/dabgpu.h, "stream state").  A measurement, not a gate.

Workload: cfg 4 (gain var, default FIRFilter, x4 Resampler, MemlessPoly, complexf, coded bits and IQ device-resident), FRAMES
frames of ONE stream, at each of the given frames per call.
Configurations: "one" -- one context, ordinary chain calls on its own stream (calls with the Resampler stay on lane 0, in call
order); "part2" / "part3" -- PartitionedStream over 2 / 3 contexts: chunk j on context j mod N, seeded from frame start - 1.
Method: every configuration and shape is warmed up once; then REPS rounds, each running every configuration once in turn
(alternating inside one process, so that clock and temperature drift hits all alike); host clock from the first queued call to
the end of a final synchronise of every context; median and min ... max over the rounds.  The seed's share: the same seeds
queued ALONE on the same contexts (nothing between them to hide behind), as a fraction of the partitioned run's median.
usage (on the GPU box): python tools/time_partitioned_stream.py [--frames 4096] [--calls 16,256] [--reps 5] [--out FILE]"""
import argparse
import importlib
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--calls", default="16,256")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    P = importlib.import_module("odr-dabmod_amd")
    S = importlib.import_module("odr-dabmod_amd.streams")
    stages = P.STAGE_GAIN | P.STAGE_FIR | P.STAGE_RESAMPLE | P.STAGE_POLY
    n = args.frames
    reps = max(5, args.reps)

    def context():
        md = P.Modulator(mode=1, max_frames=1)
        md.set_gain(P.GAIN_VAR, 1.0, 1.0 / 50000.0, 4.0)
        md.set_resampler(2048000, 8192000)
        md.set_poly([1.0, 0.05, -0.01, 0.002, 0.0], [0.0, 0.02, 0.003, 0.0, 0.0])
        return md

    one = context()
    parts = {2: S.PartitionedStream([context() for _ in range(2)]), 3: S.PartitionedStream([context() for _ in range(3)])}
    gen = torch.Generator(device="cuda").manual_seed(1)
    bits = torch.randint(0, 256, (n, one.geometry["tf_input_bytes"]), dtype=torch.uint8, device="cuda", generator=gen)
    per = one.out_samples_per_frame(stages)
    out = torch.empty((n, per), dtype=torch.complex64, device="cuda")
    torch.cuda.synchronize()

    def run_one(chunk):
        t0 = time.perf_counter()
        for (a, b) in S.partition_chunks(n, chunk, 1)[0]:
            one.chain_dev_queued(bits[a:b], b - a, stages, out[a:b])
        one.synchronize()
        return time.perf_counter() - t0

    def run_part(k, chunk):
        t0 = time.perf_counter()
        parts[k].modulate(bits, stages, chunk, out=out)
        return time.perf_counter() - t0

    def run_seeds(k, chunk):
        mods = parts[k].mods
        t0 = time.perf_counter()
        for j, a in enumerate(range(0, n, chunk)):
            mods[j % k].seed_dev(bits[a - 1] if a else None, stages, a, queued=True)
        for md in mods:
            md.synchronize()
        return time.perf_counter() - t0

    lines = ["cfg 4, %d frames of one stream, device-resident; %d rounds, configurations alternating; host clock around a final "
             "synchronise" % (n, reps),
             "%-8s %-10s %12s %22s %12s %14s" % ("frames/", "config", "median ms", "min ... max ms", "frames/s", "vs one context")]
    for chunk in [int(c) for c in args.calls.split(",")]:
        configs = [("one", lambda c=chunk: run_one(c)), ("part2", lambda c=chunk: run_part(2, c)),
                   ("part3", lambda c=chunk: run_part(3, c)), ("seeds2", lambda c=chunk: run_seeds(2, c)),
                   ("seeds3", lambda c=chunk: run_seeds(3, c))]
        # one context's bytes, kept on the side: the split must reproduce them
        run_one(chunk)
        probe = slice(0, min(n, 4 * chunk + 1))
        want = out[probe].clone()
        for name, fn in configs:                       # warm-up: every shape, every context's scratch and TII / table state
            fn()
            if name.startswith("part"):
                same = (torch.view_as_real(out[probe]).view(torch.int32) == torch.view_as_real(want).view(torch.int32)).all(dim=2).all(dim=1)
                differ = [i for i, ok in enumerate(same.tolist()) if not ok]
                if differ:
                    raise SystemExit("%s at %d frames per call: frames %s are not one context's bytes" % (name, chunk, differ))
        del want
        t = {name: [] for name, _ in configs}
        for _ in range(reps):
            for name, fn in configs:
                t[name].append(fn())
        med = {k: statistics.median(v) for k, v in t.items()}
        for name in ("one", "part2", "part3"):
            lines.append("%-8d %-10s %12.2f %10.2f ... %-9.2f %12.0f %13.3fx" % (
                chunk, name, med[name] * 1e3, min(t[name]) * 1e3, max(t[name]) * 1e3, n / med[name], med["one"] / med[name]))
        for k in (2, 3):
            name = "seeds%d" % k
            lines.append("%-8d %-10s %12.2f %10.2f ... %-9.2f %12s   %5.1f %% of part%d" % (
                chunk, name + " alone", med[name] * 1e3, min(t[name]) * 1e3, max(t[name]) * 1e3, "%d seeds" % -(-n // chunk),
                100.0 * med[name] / med["part%d" % k], k))
    text = "\n".join(lines)
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    for md in [one] + parts[2].mods + parts[3].mods:
        md.close()


if __name__ == "__main__":
    main()
