"""The channel coding that frontend.hip and decode.hip share (odr-dabmod_amd/csrc/conv_code.h: the mother code, keep_bits /
spread_bits, the segment lookup, delay_mask, the transmission-frame word to row rule), on the host alone: tools/conv_code_check.cpp
holds it to the CPU classes of odr-dabmod_amd/host/Frontend.cpp.  A plain executable that links no HIP library, built with the
address and undefined-behaviour sanitizers: a shift by 32 or a table index out of range ends it with an error."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "odr-dabmod_amd", "host")
SRCS = [os.path.join(ROOT, "tools", "conv_code_check.cpp")] + [os.path.join(HOST, n) for n in ("Frontend.cpp", "Buffer.cpp", "ModPlugin.cpp")]
INCS = [os.path.join(ROOT, "odr-dabmod_amd", "csrc"), HOST, os.path.join(ROOT, "include")]


def test_shared_code_against_the_cpu_classes(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "conv_code_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror"] + ["-I" + i for i in INCS] + SRCS
                          + ["-o", exe, "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stdout, r.stderr)
    assert r.stdout.strip() == "conv_code ok: 16384 code words, 26000 punctured words, 16 delays, 290 groups, 129816 row words", r.stdout
