"""What the streamed stages' entry points share (odr-dabmod_amd/csrc/dabgpu_ctx.h: check_stream_call, StreamHistory,
stream_from_host, stream_reset / _position / _run_samples), on the host alone: tools/stream_check.cpp defines the HIP calls
they make and the history launch as fakes, so the program is a plain executable that links no HIP library.  Built with the
address and undefined-behaviour sanitizers: an overflow in the bounds' arithmetic or a history index out of range ends it with
an error."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "stream_check.cpp")
INCS = [os.path.join(ROOT, "odr-dabmod_amd", "csrc"), os.path.join(ROOT, "include")]
HIP_INC = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")


def test_refusal_order_bounds_and_history_hand_over(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "stream_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-isystem", HIP_INC]
                          + ["-I" + i for i in INCS] + [SRC, "-o", exe, "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stdout, r.stderr)
    assert "stream ok: 8 history launches, 1 memset" in r.stdout, r.stdout
