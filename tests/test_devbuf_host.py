"""DevBuf (odr-dabmod_amd/csrc/devbuf.h), the owner of every device allocation of a context, on the host alone:
tools/devbuf_check.cpp defines hipMalloc / hipFree as counting fakes, so the program is a plain executable that links no HIP
library.  Built with the address and undefined-behaviour sanitizers: a double free or a leak ends it with an error."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "devbuf_check.cpp")
INC = os.path.join(ROOT, "odr-dabmod_amd", "csrc")
HIP_INC = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")


def test_devbuf_owns_its_allocation(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "devbuf_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-D__HIP_PLATFORM_AMD__",
                           "-isystem", HIP_INC, "-I", INC, SRC, "-o", exe,
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stdout, r.stderr)
    assert "devbuf ok" in r.stdout and "none live" in r.stdout, r.stdout
