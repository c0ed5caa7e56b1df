"""The rule the two Welch measurements share (odr-dabmod_amd/csrc/welch.h: the segment count and the segment range of a sample
pair, the run split, the run of a workgroup, the walk of a lane over its run's samples), on the host alone: tools/welch_check.cpp
walks every run with a recording, bounds-checking loader and holds the split to the two-step rule it replaced.  A read past a
buffer's last segment fails no GPU test (it lands in the allocator's slack); here it does.  A plain executable that links no HIP
library, built with the address and undefined-behaviour sanitizers."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRCS = [os.path.join(ROOT, "tools", "welch_check.cpp")]
INCS = [os.path.join(ROOT, "odr-dabmod_amd", "csrc")]


def test_shared_rule_on_the_host(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "welch_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror"] + ["-I" + i for i in INCS] + SRCS
                          + ["-o", exe, "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stdout, r.stderr)
    assert r.stdout.strip() == "welch ok: 2928 runs walked, 3000010 splits, 37212201 sample pairs", r.stdout
