"""The split-plane exchanges of the frame kernel's transform (csrc/fft_planes.h, Fft::run_planes) change which lane holds which
element between the FFT stages and nothing of the arithmetic: the Mode I cfg 3 chain with complexf output must produce the
same BYTES as the commit before them.  tools/fft_planes_golden.py ran its seeded cases on that commit and left their sha-256
in tests/golden/fft_planes_sha256.json; the same function runs them here.

Cases (the frame, 77 symbols, is the smallest unit): 1 and 3 frames x 1, 7 and 77 runs per frame (a run start at symbol 0, at
symbol 1 and mid-frame) x gain none / fix / var x TII off / on, two consecutive calls on one context."""
import importlib.util
import os

import pytest

from tests.conftest import load_pkg

pytestmark = pytest.mark.gpu

_TOOL = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "fft_planes_golden.py")
_spec = importlib.util.spec_from_file_location("fft_planes_golden", _TOOL)
golden = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(golden)


@pytest.fixture(scope="module")
def pkg():
    return load_pkg()


@pytest.fixture(scope="module")
def want():
    return golden.load_fixture()


@pytest.mark.parametrize("batch,chunks,gain,tii", golden.cases(),
                         ids=[golden.case_id(*c, 0)[:-6] for c in golden.cases()])
def test_cfg3_complexf_output_is_byte_identical_to_the_commit_before_the_split_plane_exchanges(pkg, want, batch, chunks, gain, tii):
    digests, kernels = golden.run_case(pkg, batch, chunks, gain, tii)
    name = "tf_kernel<logn=11 bits=1 gain=%d guard=1 fir=1 nt=45 cfr=0 gvar=0 zonly=0 ofmt=0 win=0 eq=1>" % (gain != "none")
    for call, (d, k) in enumerate(zip(digests, kernels)):
        # the kernel under test ran (with TII, the kernels that build or add the null symbol's segment around it)
        assert k.count(name) == 1 and sum(x.startswith("tf_kernel<logn=11 bits=1") for x in k) == 1, (call, k)
        assert d == want[golden.case_id(batch, chunks, gain, tii, call)], \
            "call %d: the samples are not the bytes the parent commit produced" % call
