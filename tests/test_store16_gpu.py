"""The Mode I cfg 3 kernels with complexf output leave their last FFT stage with pairs of consecutive samples and store a symbol's
body and cyclic prefix 16 bytes per lane (csrc/fft_planes.h: out_sample, body_lane, prefix_lane; tf_kernel.h: put16).  The digests
of tests/test_fft_planes_gpu.py hold the samples; this file tests what wider stores can get wrong and a digest cannot see:

* every byte of the frames is written by EVERY call -- the output is filled with 0xFF bytes before each of two consecutive calls
  and no dword of that pattern (a NaN no chain produces) may remain: a missing store otherwise hides behind the previous call's
  bytes, which are the same at the same position of the stream only when the input is, and stale ones in any case;
* nothing else is written -- 256 samples of 0xFF on either side of the output stay intact (a stray store of a wave reaches 128
  samples);
* an output pointer that is sample-aligned and no more (8 bytes off a 16-byte boundary, which is all dabgpu_chain_process_dev
  promises) gives the same bytes as the aligned call, guards intact;
* the kernel that ran is the one frame kernel under test.

Cases: 2 frames x 1, 7 and 77 runs per frame x TII off / on, gain var."""
import numpy as np
import pytest

from tests.conftest import load_pkg

pytestmark = pytest.mark.gpu

GUARD = 256          # samples of 0xFF in front of and behind the output
FRAMES = 2
KERNEL = "tf_kernel<logn=11 bits=1 gain=1 guard=1 fir=1 nt=45 cfr=0 gvar=0 zonly=0 ofmt=0 win=0 eq=1>"


@pytest.fixture(scope="module")
def pkg():
    return load_pkg()


def _bits(call, per):
    rs = np.random.RandomState(5200 + call)
    return np.frombuffer(rs.bytes(FRAMES * per), np.uint8).reshape(FRAMES, per).copy()


def _run(pkg, chunks, tii, shift):
    """Two consecutive calls on a fresh context into raw[GUARD + shift : GUARD + shift + n] (one int64 per complexf sample).
    -> [the frames' bytes per call, as a numpy int64 array]"""
    import torch

    md = pkg.Modulator(mode=1, device=0, max_frames=FRAMES, chunks_per_frame=chunks)
    try:
        md.set_gain(pkg.GAIN_VAR, 1.0, 1.0 / 50000.0, 4.0)
        stages = pkg.STAGE_GAIN | pkg.STAGE_FIR
        if tii:
            md.set_tii(True, 3, 5, False)
        md.trace(True)
        n = FRAMES * md.out_samples_per_frame(stages)
        raw = torch.empty(GUARD + 1 + n + GUARD, dtype=torch.int64, device="cuda:0")
        out = raw[GUARD + shift: GUARD + shift + n]
        assert raw.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 8 * shift and out.numel() * out.element_size() == 8 * n
        got = []
        for call in range(2):
            raw.fill_(-1)                                       # every byte 0xFF
            d_bits = torch.from_numpy(_bits(call, md.geometry["tf_input_bytes"])).to("cuda:0")
            assert md.chain_dev(d_bits, FRAMES, stages, out) == 8 * n
            k = md.last_variant()
            assert k.count(KERNEL) == 1 and sum(x.startswith("tf_kernel<logn=11 bits=1") for x in k) == 1, (call, k)
            host = raw.cpu().numpy()
            lo, hi = GUARD + shift, GUARD + shift + n
            assert (host[:lo] == -1).all(), "call %d: %d samples in front of the output were written" % (call, int((host[:lo] != -1).sum()))
            assert (host[hi:] == -1).all(), "call %d: %d samples behind the output were written" % (call, int((host[hi:] != -1).sum()))
            frames = host[lo:hi].copy()
            stale = np.flatnonzero(frames.view(np.int32) == -1)
            assert stale.size == 0, "call %d: %d dwords were not written, the first at sample %d of the output" % (
                call, stale.size, int(stale[0]) // 2)
            assert np.isfinite(frames.view(np.float32)).all()
            got.append(frames)
        return got
    finally:
        md.close()


@pytest.mark.parametrize("tii", [False, True], ids=["tii0", "tii1"])
@pytest.mark.parametrize("chunks", [1, 7, 77], ids=["chunks1", "chunks7", "chunks77"])
def test_sixteen_byte_stores_write_every_byte_of_the_frames_nothing_else_and_need_no_alignment(pkg, chunks, tii):
    aligned = _run(pkg, chunks, tii, 0)
    shifted = _run(pkg, chunks, tii, 1)
    for call in range(2):
        diff = np.flatnonzero(aligned[call] != shifted[call])
        assert diff.size == 0, "call %d: %d samples differ with an output pointer 8 bytes off a 16-byte boundary, the first at %d" % (
            call, diff.size, int(diff[0]))
    # (the two calls carry other bits: a call that left the previous call's samples in place would also show here)
    assert (aligned[0] != aligned[1]).any()
