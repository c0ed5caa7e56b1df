"""The layout half of the device front-end (dabgpu_frontend_describe: host code, no device) against the CPU front-end's
classes (odr-dabmod_amd.frontend.Frontend, itself bit-exact against the reference: tests/test_frontend.py).  What the
kernels then compute from this layout is checked on the GPU (tests/test_gpu_frontend_gpu.py)."""
import importlib

import numpy as np
import pytest

from tests.conftest import load_pkg
from tests.golden.synth import synth_eti

CIF_END = "FrameMultiplexer: sub-channel beyond the end of the CIF"


def _fe():
    return importlib.import_module("odr-dabmod_amd.frontend").Frontend()


def _frame(subchannels, mid=1):
    """One ETI frame whose header names `subchannels` (SAD, STL, TPL); the payload is whatever fits (describe reads FC and STC)."""
    f = synth_eti(1, subchannels=(), mid=mid)[0]
    f[5] = 0x80 | len(subchannels)
    for i, (sad, stl, tpl) in enumerate(subchannels):
        f[8 + 4 * i:12 + 4 * i] = ((i << 2) & 0xfc | (sad >> 8) & 3, sad & 0xff, ((tpl & 0x3f) << 2) | (stl >> 8) & 3, stl & 0xff)
    return f


def _describe(pkg, frame):
    """-> (layout, None) or (None, message)"""
    try:
        return pkg.Modulator.frontend_describe(frame), None
    except pkg.DabGpuError as e:
        return None, str(e)


@pytest.fixture(scope="module")
def sweep():
    """describe and the CPU classes over STL 3 ... 288 x TPL 0 ... 63, once: {(stl, tpl): (layout, message, profile, punctured)}"""
    pkg, fe = load_pkg(), _fe()
    pkg.build()
    out = {}
    for stl in range(3, 289):
        for tpl in range(64):
            lay, msg = _describe(pkg, _frame(((0, stl, tpl),)))
            prof = fe.subchannel_profile(stl, tpl)
            try:
                punct = int(fe.puncture(np.zeros(32 * stl + 3, np.uint8), stl, tpl).size)
            except ValueError:
                punct = None
            out[(stl, tpl)] = (lay, msg, prof, punct)
    return out


def test_describe_accepts_exactly_what_the_cpu_puncturer_accepts(sweep):
    """A frame is refused for its protection profile exactly where Frontend.puncture fails; 736 pairs pass (UEP 256, EEP-A
    384, EEP-B 96).  24 of them are larger than a CIF (e.g. STL 288 at EEP 1-A: 1152 CU): the puncturer takes them, the
    multiplexer does not -- describe refuses those with the FrameMultiplexer's message, which it checks LAST, so that message
    says that every check of the puncturer passed."""
    passed = {k for k, (lay, msg, _, _) in sweep.items() if lay is not None or msg == CIF_END}
    cpu = {k for k, v in sweep.items() if v[3] is not None}
    assert passed == cpu
    assert len(passed) == 736
    forms = [sum(1 for (_, tpl) in passed if sel(tpl)) for sel in
             (lambda t: t < 32, lambda t: t >= 32 and (t >> 2) & 7 == 0, lambda t: t >= 32 and (t >> 2) & 7 == 1)]
    assert forms == [256, 384, 96]
    too_large = {k for k, (lay, msg, _, _) in sweep.items() if msg == CIF_END}
    assert too_large == {k for k in cpu if sweep[k][2][1] > 864} and len(too_large) == 24


def test_rules_sizes_and_padding_byte_equal_the_cpu_profile(sweep):
    padded = []
    smallest = None
    for (stl, tpl), (lay, _, prof, punct) in sweep.items():
        if lay is None:
            continue
        assert lay["nst"] == 1 and lay["mode"] == 1 and lay["fic_bytes"] == 96
        s = lay["subchannels"][0]
        rules, cu, _ = prof
        assert (s["sad"], s["stl"], s["tpl"], s["framesize"]) == (0, stl, tpl, 8 * stl)
        # (a PuncturingRule's length is in bytes of mother-code output; the layout counts 4-byte groups)
        assert [(4 * g, p) for g, p in s["rules"]] == rules and 1 <= len(rules) <= 4
        assert s["cu"] == cu and punct == 8 * cu
        # no accepted profile needs the rule list to cycle: the rules cover the mother code's output exactly once
        assert sum(g for g, _ in s["rules"]) == 8 * stl
        bits = sum(g * bin(p).count("1") for g, p in s["rules"]) + 12
        assert s["padding_byte"] == (1 if (bits + 7) // 8 == 8 * cu - 1 else 0) and (bits + 7) // 8 in (8 * cu, 8 * cu - 1)
        if s["padding_byte"]:
            padded.append((stl, tpl))
        if smallest is None or cu < smallest[0]:
            smallest = (cu, stl, tpl)
    assert len(padded) == 32 and {(21, 1), (24, 1), (30, 1)} <= set(padded)
    assert smallest == (4, 3, 0x23)
    assert all(lay["tail"] == (3, 0xcccccc) for lay, _, _, _ in sweep.values() if lay)


def test_the_largest_sub_channel_that_fits_a_cif():
    pkg = load_pkg()
    lay, msg = _describe(pkg, _frame(((0, 432, 0x22),)))
    assert msg is None and lay["subchannels"][0]["cu"] == 864
    assert _describe(pkg, _frame(((1, 432, 0x22),)))[1] == CIF_END


def test_fic_layout_per_mode():
    pkg = load_pkg()
    for mid, mode, fic, groups in ((1, 1, 96, 84), (2, 2, 96, 84), (3, 3, 128, 116), (0, 4, 96, 84)):
        lay, msg = _describe(pkg, _frame((), mid=mid))
        assert msg is None
        assert (lay["mode"], lay["fic_bytes"], lay["nst"], lay["fic_offset"]) == (mode, fic, 0, 12)
        assert lay["fic_rules"] == [(groups, 0xeeeeeeee), (12, 0xeeeeeeec)]
        # 2304 (3072) punctured bits per ETI frame: BlockPartitioner's FIC size
        assert sum(g * bin(p).count("1") for g, p in lay["fic_rules"]) + 12 == (3072 if mode == 3 else 2304)


def test_each_refusal_carries_the_message_of_the_class_that_throws():
    pkg = load_pkg()
    no_fic = _frame(((0, 48, 0x22),))
    no_fic[5] &= 0x7f
    assert _describe(pkg, no_fic)[1] == "FIC must be present to modulate!"
    # a profile without rules: no UEP profile for 8 x 5 / 3 kbit/s; unknown EEP option
    assert _describe(pkg, _frame(((0, 5, 0),)))[1] == "SubchannelSource UEP puncturing rules do not exist!"
    assert _describe(pkg, _frame(((0, 48, 0x28),)))[1] == "SubchannelSource::SubchannelSource unknown protection option!"
    # ... without a size: EEP-B below 32 kbit/s
    assert _describe(pkg, _frame(((0, 6, 0x24),)))[1] == "SubchannelSource::framesizeCu protection not yet coded!"
    # a punctured size that is neither 8 CU nor 8 CU - 1 (EEP 3-A off the 8 kbit/s grid)
    msg = _describe(pkg, _frame(((0, 4, 0x22),)))[1]
    assert msg.startswith("PuncturingEncoder encoder initialisation failed.  CU: 6 block_size: ")
    assert _describe(pkg, _frame(((800, 48, 0x22),)))[1] == CIF_END                  # 800 + 96 CU
    assert _describe(pkg, _frame(((768, 48, 0x22),)))[1] is None                     # ends AT 864
    # payload that overruns the frame: 96 + 6 x 8 x 126 bytes of payload
    many = tuple((130 * i, 126, 0x23) for i in range(6))
    assert _describe(pkg, _frame(many))[1] == "EtiReader: stream characterisation exceeds the 6144-byte ETI frame"
    assert _describe(pkg, _frame(many[:5]))[1] is None
    # the first refusal in the CPU's order wins: the overrun is seen before a sub-channel's size is asked for
    assert _describe(pkg, _frame(many + ((0, 4, 0x22),)))[1].startswith("EtiReader")


def test_payload_offsets_for_nst_0_1_and_12():
    pkg = load_pkg()
    assert _describe(pkg, _frame(()))[0]["subchannels"] == []
    lay = _describe(pkg, _frame(((10, 48, 0x22),)))[0]
    assert lay["fic_offset"] == 16 and lay["subchannels"][0]["offset"] == 16 + 96
    subs = tuple((60 * i, (3, 6, 12, 24, 48, 21)[i % 6], (0x23, 0x23, 0x23, 0x22, 0x22, 1)[i % 6]) for i in range(12))
    lay = _describe(pkg, _frame(subs, mid=3))[0]
    assert lay["nst"] == 12 and lay["fic_offset"] == 12 + 48 and lay["fic_bytes"] == 128
    at = 12 + 48 + 128
    for s, (sad, stl, tpl) in zip(lay["subchannels"], subs):
        assert (s["sad"], s["stl"], s["tpl"], s["offset"]) == (sad, stl, tpl, at)
        at += 8 * stl
    # the same STC words on the frames synth_eti lays out: its payload starts where the layout says
    eti = synth_eti(1, subchannels=subs, mid=3)[0]
    assert _describe(pkg, eti)[0] == lay


@pytest.mark.parametrize("opts,word", [(["--batch", "4", "--contexts", "2"], "--contexts above 1"), (["--bits-only"], "--bits-only"),
                                       (["--separate-converter"], "--separate-converter")])
def test_dabmod_file_refuses_gpu_frontend_with_options_it_cannot_honour(tmp_path, opts, word):
    """Decided before any file or device is opened: the time interleaver's history is not part of the state a second chain is
    seeded with, and the coded bits never reach the host."""
    import os
    import subprocess
    from tests.conftest import ROOT
    fin, fout = str(tmp_path / "in.eti"), str(tmp_path / "out")
    synth_eti(8).tofile(fin)
    r = subprocess.run([os.path.join(ROOT, "odr-dabmod_amd", "host", "dabmod_file"), fin, fout, "--gpu-frontend"] + opts,
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and r.stderr.startswith("dabmod_file: --gpu-frontend does not go with") and word in r.stderr
    assert not os.path.exists(fout)
