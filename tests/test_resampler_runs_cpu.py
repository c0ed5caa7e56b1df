"""The resampler's run geometry without a device: resampler_runs.h (the one host function all four launchers size their grid
with) compiled by itself.  With nothing forced it is, number for number, the arithmetic the launchers had inline -- runs of
max(2, min(96, nhops / 512)) hops, and max(1, min(24, nhops / 1536)) for the hop-independent Mode I x2 / x4 kernel -- from a
one-hop call to the benchmark's 4096 frames; a forced value is taken as it is, and one above nhops gives one workgroup."""
import os
import re
import subprocess

from tests.conftest import ROOT, load_pkg

CSRC = os.path.join(ROOT, "odr-dabmod_amd", "csrc")
MAIN = r"""
#include "resampler_runs.h"
#include <cstdio>
#include <cstdlib>
int main(int argc, char **argv)
{
    for (int i = 1; i + 2 < argc; i += 3) {
        const size_t nhops = std::strtoull(argv[i], nullptr, 10);
        const int hpr = dabgpu::resampler_run_hops(nhops, std::atoi(argv[i + 1]) != 0, std::atoi(argv[i + 2]));
        std::printf("%d %u\n", hpr, dabgpu::resampler_run_grid(nhops, hpr));
    }
    return 0;
}
"""


def _ask(tmp_path, cases):
    src, exe = str(tmp_path / "runs.cpp"), str(tmp_path / "runs")
    with open(src, "w") as f:
        f.write(MAIN)
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", CSRC, src, "-o", exe], check=True, capture_output=True, timeout=120)
    args = [str(v) for c in cases for v in (c[0], int(c[1]), c[2])]
    out = subprocess.run([exe] + args, check=True, capture_output=True, text=True, timeout=60).stdout.split("\n")
    return [tuple(int(v) for v in line.split()) for line in out if line]


def test_default_run_geometry_is_the_arithmetic_the_launchers_had(tmp_path):
    frames = [1, 2, 3, 4, 5, 8, 15, 16, 17, 31, 32, 33, 64, 256, 511, 512, 513, 1000, 4096]
    hops = sorted(set([1, 2, 3, 49, 50, 95, 97, 511, 512, 1023, 1024, 1025, 1535, 1536, 1537, 3071, 3072, 3073, 36863, 36864,
                       36865, 49151, 49152, 49153] + [96 * f for f in frames] + [96 * f + 1 for f in frames]))
    cases = [(n, fam, 0) for n in hops for fam in (False, True)]
    got = _ask(tmp_path, cases)
    assert len(got) == len(cases)
    for (n, hop_independent, _), (hpr, grid) in zip(cases, got):
        want = max(1, min(24, n // 1536)) if hop_independent else max(2, min(96, n // 512))
        assert (hpr, grid) == (want, (n + want - 1) // want), (n, hop_independent, hpr, grid)
    # the benchmark's call: 4096 Mode I frames, runs of 24 (resampler16_kernel) and of 96 (the others)
    at = dict(zip([(c[0], c[1]) for c in cases], got))
    assert at[(4096 * 96, True)] == (24, 16384) and at[(4096 * 96, False)] == (96, 4096)
    assert at[(96, True)] == (1, 96) and at[(96, False)] == (2, 48) and at[(384, True)] == (1, 384) and at[(384, False)] == (2, 192)


def test_forced_run_length_sizes_the_grid(tmp_path):
    cases = [(n, fam, f) for n in (1, 2, 3, 49, 50, 96, 393216) for fam in (False, True) for f in (1, 2, 3, 5, 24, 96, n, n + 7, 2 ** 31 - 1)]
    got = _ask(tmp_path, cases)
    for (n, _, f), (hpr, grid) in zip(cases, got):
        assert hpr == f and grid == (n + f - 1) // f and (grid == 1 if f >= n else grid > 1), (n, f, hpr, grid)


def test_the_diagnostics_are_exported_bound_and_documented():
    pkg = load_pkg()
    header = open(os.path.join(ROOT, "include", "dabgpu.h")).read()
    comments = " ".join(re.findall(r"/\*.*?\*/", header, re.S))
    for name, method in (("dabgpu_debug_resampler_run_hops", "set_resampler_run_hops"),
                         ("dabgpu_debug_resampler_last_launch", "resampler_last_launch")):
        assert name in pkg.EXPORTS and hasattr(pkg.Modulator, method) and name in comments, name
