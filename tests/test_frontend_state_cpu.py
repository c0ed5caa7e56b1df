"""The front-end's stream state in the C-ABI, the parts that need no GPU: the seven entry points are declared and exported,
the lead-in range in front of a chunk is the documented one, and dabmod_file refuses --state-in / --state-out without the
front-end on the device before it opens anything."""
import os
import re
import subprocess

import pytest

from tests.conftest import ROOT, load_pkg

HOST = os.path.join(ROOT, "odr-dabmod_amd", "host")
NAMES = ("dabgpu_frontend_state_bytes", "dabgpu_frontend_get_state", "dabgpu_frontend_set_state", "dabgpu_frontend_seed",
         "dabgpu_frontend_seed_dev", "dabgpu_chain_seed_eti", "dabgpu_chain_seed_eti_dev")


def test_header_declares_and_library_exports_the_front_end_state_entry_points():
    pkg = load_pkg()
    pkg.build()
    text = open(os.path.join(ROOT, "include", "dabgpu.h")).read()
    declared = set(re.findall(r"DABGPU_API[^;]*?\b(dabgpu_[a-z_0-9]+)\s*\(", text, re.S))
    lib = pkg.load_library()
    for name in NAMES:
        assert name in declared, name
        assert name in pkg.EXPORTS, name
        assert hasattr(lib, name), "libdabgpu.so does not export %s" % name
    assert re.search(r"^#define DABGPU_FE_HISTORY_FRAMES 15$", text, re.M)
    assert pkg.FE_HISTORY_FRAMES == 15
    # the blob has one size for every layout: the documented header and fifteen CIFs (a static_assert holds the other end),
    # and the size needs no device
    assert "DABGPU_FE_STATE_HEADER_BYTES 540" in text
    assert lib.dabgpu_frontend_state_bytes(None) == 0
    # the existing stream-state blob is what it was
    assert "DABGPU_STREAM_STATE_VERSION 1u" in text and "DABGPU_STREAM_STATE_HEADER_BYTES 40" in text


def streams_module():
    import importlib
    load_pkg()
    return importlib.import_module("odr-dabmod_amd.streams")


# e -> (start, stop): fifteen frames back for the time interleaver; with the chain, the transmission frame in front of e
# whole and the fifteen frames in front of that one; never before the start of the stream
LEADIN = {
    (4, True): {0: (0, 0), 4: (0, 4), 8: (0, 8), 12: (0, 12), 16: (0, 16), 20: (1, 20), 40: (21, 40)},
    (4, False): {0: (0, 0), 4: (0, 4), 8: (0, 8), 12: (0, 12), 16: (1, 16), 20: (5, 20), 40: (25, 40)},
    (1, True): {0: (0, 0), 4: (0, 4), 8: (0, 8), 12: (0, 12), 16: (0, 16), 20: (4, 20), 40: (24, 40)},
    (1, False): {0: (0, 0), 4: (0, 4), 8: (0, 8), 12: (0, 12), 16: (1, 16), 20: (5, 20), 40: (25, 40)},
}


@pytest.mark.parametrize("with_chain", [True, False])
@pytest.mark.parametrize("cifs", [4, 1])
def test_eti_leadin_is_the_range_the_seeds_ask_for(cifs, with_chain):
    st = streams_module()
    for e, want in LEADIN[(cifs, with_chain)].items():
        got = st.eti_leadin(e, cifs, with_chain)
        assert got == want, (e, got)
        # ... which is the rule of include/dabgpu.h: n_leadin = min(e, 15 [+ cifs]) frames that end at e
        assert got[1] == e and got[1] - got[0] == min(e, 15 + (cifs if with_chain else 0))
    assert st.eti_leadin(20, 4) == st.eti_leadin(20, 4, True)                 # the chain's lead-in is the default
    with pytest.raises(ValueError):
        st.eti_leadin(6, 4)                                                    # not the start of a transmission frame
    with pytest.raises(ValueError):
        st.eti_leadin(-4, 4)


@pytest.mark.parametrize("option", ["--state-in", "--state-out"])
def test_dabmod_file_refuses_stream_state_files_without_the_gpu_frontend(tmp_path, option):
    """Exit status 2 with the message, before any file or device is opened: the input does not even exist, and neither the
    output nor the state file appears."""
    fin, fout, state = str(tmp_path / "missing.eti"), str(tmp_path / "out"), str(tmp_path / "state")
    r = subprocess.run([os.path.join(HOST, "dabmod_file"), fin, fout, "--batch", "4", option, state],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 2, r.stderr[-2000:]
    assert option + " does not go with" in r.stderr and "--gpu-frontend" in r.stderr
    assert "cannot read" not in r.stderr
    assert not os.path.exists(fout) and not os.path.exists(state)
