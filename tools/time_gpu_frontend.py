#!/usr/bin/env python3
"""What the front-end on the device costs (include/dabgpu.h, "the front-end on the device").

  (a) the two front-end launches alone (dabgpu_frontend_process_dev, device buffers, HIP events) at 16 / 256 / 4096 Mode I
      transmission frames, with the cfg 1 layout (one sub-channel) and the `multi` layout (five), next to the cfg 3 chain
      call (dabgpu_chain_process_dev: gain var + FIRFilter) on the same batch in the same process;
  (b) dabgpu_chain_process_eti against dabgpu_chain_process on coded bits that are already there (host buffers, wall clock);
  (c) dabmod_file --batch 32 with and without --gpu-frontend for complexf / s16 / u8 (wall clock of the whole program).

Method as in tools/time_host_path.py: a warm-up by time (>= 0.3 s), then five repetitions of >= 0.2 s each; the line carries
the MEDIAN and the spread.  Nothing is asserted.

usage (GPU box): python tools/time_gpu_frontend.py [--skip-file] > profiles/gpu_frontend.txt"""
import importlib
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from tests.golden.frontend_cases import ETI_CASES  # noqa: E402
from tests.golden.synth import synth_eti  # noqa: E402

P = importlib.import_module("odr-dabmod_amd")
pc = time.perf_counter
LAYOUTS = {"cfg1": ((0, 48, 0x22),), "multi": ETI_CASES["multi"]["kw"]["subchannels"]}
CFG3 = P.STAGE_GAIN | P.STAGE_FIR


def stream_of(layout, n_tf):
    """n_tf Mode I transmission frames of ETI: 32 synthetic frames tiled (FP runs 0 ... 7, so every copy starts aligned)"""
    base = synth_eti(32, subchannels=LAYOUTS[layout], mid=1)
    return np.ascontiguousarray(np.tile(base, ((4 * n_tf + 31) // 32, 1))[:4 * n_tf])


def timed_device(step, stream, warm_s=0.3, rep_s=0.2, reps=5):
    """seconds per call of step(), between HIP events on `stream`: median, min, max of `reps` repetitions"""
    t0 = pc()
    n = 0
    while pc() - t0 < warm_s or n < 4:
        step(); n += 1
        stream.synchronize()
    per_call = (pc() - t0) / n
    calls = max(4, int(rep_s / per_call))
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        for _ in range(calls):
            step()
        b.record(stream)
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e-3 / calls)
    out.sort()
    return out[len(out) // 2], out[0], out[-1], calls


def timed_host(step, warm_s=0.3, rep_s=0.2, reps=5):
    t0 = pc()
    n = 0
    while pc() - t0 < warm_s or n < 4:
        step(); n += 1
    calls = max(4, int(rep_s / ((pc() - t0) / n)))
    out = []
    for _ in range(reps):
        t0 = pc()
        for _ in range(calls):
            step()
        out.append((pc() - t0) / calls)
    out.sort()
    return out[len(out) // 2], out[0], out[-1], calls


def part_a():
    print("(a) front-end launches alone vs the cfg 3 chain call, device buffers, HIP events; Mode I")
    dev = torch.device("cuda", 0)
    side = torch.cuda.Stream(device=dev)
    for B in (16, 256, 4096):
        md = P.Modulator(mode=1, max_frames=B)
        md.set_gain(2, 1.0, 1 / 50000.0, 4.0)
        md.set_fir_taps(None)
        with torch.cuda.stream(side):
            d_bits = torch.empty(B * 28800, dtype=torch.uint8, device=dev)
            d_iq = torch.empty((B, md.out_samples_per_frame(CFG3)), dtype=torch.complex64, device=dev)
            for layout in LAYOUTS:
                eti = stream_of(layout, B)
                d_eti = torch.from_numpy(eti).to(dev)
                md.frontend_configure(eti[0])
                t, lo, hi, calls = timed_device(lambda: md.eti_to_bits_dev(d_eti, 4 * B, d_bits, stream=side.cuda_stream), side)
                print("  B=%4d  front-end %-5s  %9.1f us per call  %10.0f frames/s  (median of 5 x %d calls: %.1f ... %.1f us)"
                      % (B, layout, t * 1e6, B / t, calls, lo * 1e6, hi * 1e6), flush=True)
            t, lo, hi, calls = timed_device(lambda: md.chain_dev(d_bits, B, CFG3, d_iq, stream=side.cuda_stream), side)
            print("  B=%4d  cfg 3 chain      %9.1f us per call  %10.0f frames/s  (median of 5 x %d calls: %.1f ... %.1f us)"
                  % (B, t * 1e6, B / t, calls, lo * 1e6, hi * 1e6), flush=True)
        side.synchronize()
        md.close()
        del d_bits, d_iq, d_eti


def part_b():
    print("(b) dabgpu_chain_process_eti vs dabgpu_chain_process on bits that are already there; host buffers, cfg 3, multi layout")
    for B in (1, 32):
        md = P.Modulator(mode=1, max_frames=B)
        md.set_gain(2, 1.0, 1 / 50000.0, 4.0)
        md.set_fir_taps(None)
        eti = stream_of("multi", B)
        md.frontend_configure(eti[0])
        bits = md.eti_to_bits(eti).copy()
        out = np.empty(B * md.out_samples_per_frame(CFG3), np.complex64)
        for tag, step in (("chain(bits)", lambda: md.chain(bits, CFG3, out=out)), ("chain_eti(eti)", lambda: md.chain_eti(eti, CFG3, out=out))):
            t, lo, hi, calls = timed_host(step)
            print("  B=%3d  %-15s %9.2f ms per call  %9.0f frames/s  (median of 5 x %d calls: %.2f ... %.2f ms)"
                  % (B, tag, t * 1e3, B / t, calls, lo * 1e3, hi * 1e3), flush=True)
        md.close()


def part_c():
    print("(c) dabmod_file --batch 32, whole program, 9600 ETI frames = 2400 transmission frames (cfg 1 layout), output to a file in the temporary directory")
    tool = os.path.join(ROOT, "odr-dabmod_amd", "host", "dabmod_file")
    with tempfile.TemporaryDirectory() as d:
        fin, fout = os.path.join(d, "in.eti"), os.path.join(d, "out.iq")
        np.tile(synth_eti(48), (200, 1)).tofile(fin)
        for fmt in ("complexf", "s16", "u8"):
            for extra in ([], ["--gpu-frontend"]):
                ts = []
                for _ in range(3):
                    t0 = pc()
                    r = subprocess.run([tool, fin, fout, "--format", fmt, "--batch", "32"] + extra, capture_output=True, text=True)
                    ts.append(pc() - t0)
                    if r.returncode:
                        print("  dabmod_file failed: " + r.stderr[-300:])
                        return
                ts.sort()
                print("  %-8s %-15s %6.3f s  %8.0f frames/s  (median of 3 runs: %.3f ... %.3f s; %s)"
                      % (fmt, " ".join(extra) or "CPU front-end", ts[1], 2400 / ts[1], ts[0], ts[2], r.stdout.strip()), flush=True)


if __name__ == "__main__":
    print("device: " + torch.cuda.get_device_name(0))
    part_a()
    part_b()
    if "--skip-file" not in sys.argv:
        part_c()
