"""The CIC equaliser in the fused chain, what can be checked without a device: the C-ABI declares the entries, the Python
binding lists them, and install_fused.sh turns a configured dac_clk_rate into the chain's setting instead of refusing it."""
import os
import re
import shutil
import subprocess

import pytest

from tests.conftest import ROOT

HOST = os.path.join(ROOT, "odr-dabmod_amd", "host")
ENTRIES = ("dabgpu_set_cic_equalizer", "dabgpu_carriers_process", "dabgpu_carriers_process_dev")
have_ref = pytest.mark.skipif(not os.path.isdir("/root/reference/src"), reason="the reference tree is not on this machine")


def test_header_declares_the_cic_entries(pkg):
    text = open(os.path.join(ROOT, "include", "dabgpu.h")).read()
    for name in ENTRIES:
        assert len(re.findall(r"DABGPU_API\s+int\s+%s\s*\(" % name, text)) == 1, name
        assert name in pkg.EXPORTS
    # the setter: (ctx, enable, spacing, R); the host entry takes a byte count, the device entry frames and a stream
    assert re.search(r"dabgpu_set_cic_equalizer\(dabgpu_ctx \*ctx, int enable, size_t spacing, int R\)", text)
    assert re.search(r"dabgpu_carriers_process_dev\([^)]*size_t n_frames[^)]*void \*stream\)", text, re.S)
    for method in ("set_cic_equalizer", "carriers", "carriers_dev"):
        assert callable(getattr(pkg.Modulator, method))


def test_host_settings_carry_the_cic_parameters():
    text = open(os.path.join(HOST, "GpuStages.h")).read()
    assert re.search(r"size_t cicSpacing = 0;", text) and re.search(r"int cicRatio = 0;", text)
    assert "dabgpu_set_cic_equalizer(dev, 1, s.cicSpacing, s.cicRatio)" in open(os.path.join(HOST, "GpuStages.cpp")).read()


@have_ref
def test_install_fused_writes_the_cic_decision_instead_of_refusing(tmp_path):
    """A text check on a scratch copy of the reference's src/ (nothing of it is kept): the refusal is gone, the edited
    DabModulator.cpp assigns the chain's two settings from clockRate / outputRate, and the anchors still hold."""
    src = tmp_path / "src"
    shutil.copytree("/root/reference/src", str(src))
    for script in ("install_dropins.sh", "install_fused.sh"):
        subprocess.check_call(["sh", os.path.join(HOST, script), str(src)])
    text = open(str(src / "DabModulator.cpp")).read()
    assert "the CIC equaliser is not part of the fused chain" not in text
    assert len(re.findall(r"gs\.cicRatio\s*=", text)) == 1 and len(re.findall(r"gs\.cicSpacing\s*=", text)) == 1
    assert "m_settings.clockRate / m_settings.outputRate / 4" in text and "400000000" in text
    assert text.index("DabGpuChain::Settings gs;") < text.index("gs.cicRatio") < text.index("make_shared<DabGpuChain>(gs, live)")
    # the stage objects of the replaced block are gone with it
    assert "make_shared<CicEqualizer>" not in text
