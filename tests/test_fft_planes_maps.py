"""The index maps of the split-plane FFT exchanges (csrc/fft_planes.h), proved on the host: tools/fft_planes_check.cpp includes the
header the frame kernel includes and asserts that every map is a bijection, every exchange write lane-contiguous inside a wave,
every gather bank-conflict-free under the lane groups of ds_read_b128, and that a float64 transform moved through the maps alone
equals a direct DFT.  Built and run twice: plain, and with the address and undefined-behaviour sanitizers (a host program
with its own main)."""
import importlib.util
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "fft_planes_check.cpp")
INC = os.path.join(ROOT, "odr-dabmod_amd", "csrc")


def _cxx():
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    return cxx


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitized"])
def test_fft_planes_maps_hold_on_the_host(tmp_path, flags):
    exe = str(tmp_path / "fft_planes_check")
    subprocess.check_call([_cxx(), "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-I", INC, SRC, "-o", exe] + flags)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stdout, r.stderr)
    assert "maps, writes, gathers ok" in r.stdout, r.stdout


def test_byte_identity_fixture_covers_exactly_the_tools_cases():
    """tests/golden/fft_planes_sha256.json holds one digest for every case and call of tools/fft_planes_golden.py, no other."""
    spec = importlib.util.spec_from_file_location("fft_planes_golden", os.path.join(ROOT, "tools", "fft_planes_golden.py"))
    golden = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(golden)
    want = golden.load_fixture()
    ids = {golden.case_id(b, c, g, t, call) for b, c, g, t in golden.cases() for call in range(golden.CALLS)}
    assert set(want) == ids and len(ids) == 2 * 3 * 3 * 2 * 2
    assert all(len(v) == 64 and int(v, 16) >= 0 for v in want.values())
