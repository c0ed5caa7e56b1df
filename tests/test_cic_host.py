"""The CIC equaliser through the host mirror: dabmod_file --cic SPACING,R and DabGpuChain::Settings::cicSpacing / cicRatio give,
byte for byte, what Modulator.chain gives after set_cic_equalizer (the library against the oracle: tests/test_cic_chain_gpu.py)."""
import os
import subprocess

import numpy as np
import pytest

from tests.conftest import ROOT
from tests.golden.synth import synth_eti

pytestmark = pytest.mark.gpu

HOST = os.path.join(ROOT, "odr-dabmod_amd", "host")
G, F = 1, 2
NORMALISE = 1.0 / 50000.0


def same_bytes(a, b):
    a = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    b = np.ascontiguousarray(b).view(np.uint8).reshape(-1)
    return a.size == b.size and a.size > 0 and np.array_equal(a, b)


@pytest.fixture(scope="module")
def stream(pkg):
    """16 ETI frames (4 transmission frames of Mode I), the library's coded bits and its IQ with and without the equaliser"""
    eti = synth_eti(16)
    out = {}
    for cic in (None, (2048, 8)):
        md = pkg.Modulator(mode=1, max_frames=4)
        try:
            md.set_gain(2, 1.0, NORMALISE, 4.0)
            if cic:
                md.set_cic_equalizer(True, *cic)
            md.frontend_configure(eti[0])
            bits = md.eti_to_bits(eti)
            md.frontend_reset()
            out[cic] = md.chain_eti(eti, G | F)
            assert same_bytes(out[cic], md.chain(bits, G | F))
        finally:
            md.close()
    assert not same_bytes(out[None], out[(2048, 8)])
    return eti, bits, out[(2048, 8)]


@pytest.mark.parametrize("extra", [[], ["--batch", "2"], ["--gpu-frontend", "--batch", "2"], ["--batch", "2", "--contexts", "2"]],
                         ids=["frame-by-frame", "batch", "gpu-frontend", "contexts"])
def test_dabmod_file_cic_equals_the_library(tmp_path, stream, extra):
    eti, _, want = stream
    fin, fout = str(tmp_path / "in.eti"), str(tmp_path / "out.iq")
    eti.tofile(fin)
    r = subprocess.run([os.path.join(HOST, "dabmod_file"), fin, fout, "--cic", "2048,8", "--fir", "default", "--normalise",
                        repr(NORMALISE)] + extra, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert same_bytes(np.fromfile(fout, np.uint8), want)


def test_dabmod_file_refuses_half_a_cic_parameter_pair(tmp_path):
    fin = str(tmp_path / "in.eti")
    synth_eti(4).tofile(fin)
    for bad in ("2048", "0,8", "2048,0"):
        r = subprocess.run([os.path.join(HOST, "dabmod_file"), fin, str(tmp_path / "out"), "--cic", bad], capture_output=True,
                           text=True, timeout=60)
        assert r.returncode == 2 and r.stderr.startswith("usage:"), (bad, r.stderr[:200])


def test_host_selftest_pushes_the_cic_settings(tmp_path, stream):
    _, bits, want = stream
    fin, fout = str(tmp_path / "bits.bin"), str(tmp_path / "out.iq")
    bits.tofile(fin)
    r = subprocess.run([os.path.join(HOST, "host_selftest"), "cic", fin, "4", "2048", "8", fout], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "cic: 4 frames written" in r.stdout
    assert same_bytes(np.fromfile(fout, np.uint8), want)
