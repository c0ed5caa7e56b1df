"""The channel decoder on the device (include/dabgpu.h, "the channel decoder"; odr-dabmod_amd/csrc/decode.hip): coded bits ->
the ETI payload.  Clean input: BYTE equality with the ETI frames the bits were made from (the CPU front-end's bits, or the
device's own IQ demodulated).  Input with errors: byte equality with the numpy model (tests/decode_model.py), figures included --
integer work under fixed rules, nothing to tolerate."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from tests import decode_cases as K
from tests import decode_model as M
from tests.conftest import ROOT
from tests.golden.frontend_cases import PUNCTURE_CASES
from tests.golden.synth import synth_eti

pytestmark = pytest.mark.gpu

HOST = os.path.join(ROOT, "odr-dabmod_amd", "host")
G, F = 1, 2


@pytest.fixture(scope="module")
def mods(pkg):
    """one context per mode, shared (every test configures its own layout, which starts a stream)"""
    ms = {m: pkg.Modulator(mode=m, max_frames=40) for m in (1, 2, 3, 4)}
    yield ms
    for m in ms.values():
        m.close()


@pytest.fixture(scope="module")
def multi(pkg):
    """the Mode I stream the error tests share: 20 ETI frames, bits, layout, reference rows (left unchanged)"""
    eti, bits = K.stream(20, K.MULTI, 1)
    return eti, bits, pkg.Modulator.frontend_describe(eti[0]), K.reference_rows(eti, 20)


def decode_whole(md, eti, bits, ref=True):
    md.frontend_configure(eti[0])
    n = bits.shape[0] * M.CIFS[md.geometry["mode"]]
    return md.decode(bits, K.reference_rows(eti, n) if ref else None)


def check_clean(pkg, md, eti, bits, what):
    """outputs 15 ... equal the stream's frames on the FIC and MST regions, zero elsewhere; the lead-in is zero and not valid"""
    layout = pkg.Modulator.frontend_describe(eti[0])
    keep = M.payload_mask(layout)
    us, _ = M.units(layout)
    images, stats = decode_whole(md, eti, bits)
    n = images.shape[0]
    assert n > 15 and np.array_equal(images[15:][:, keep], eti[:n - 15][:, keep]), what
    assert not images[:15].any() and not images[:, ~keep].any(), what
    for i in range(n):
        want = dict(valid=int(i >= 15), corrected=0, coded_bits=sum(u["coded_bits"] for u in us) if i >= 15 else 0, bit_errors=0,
                    n_bits=8 * int(keep.sum()) if i >= 15 else 0)
        assert stats[i] == want, (what, i)
    for ui, u in enumerate(us):
        st = md.decode_stats(n - 1, ui)
        assert (st["corrected"], st["coded_bits"], st["n_bits"]) == (0, u["coded_bits"], 8 * u["in_bytes"]), (what, ui)


# --------------------------------------------------------------------------- 1. clean round trip
@pytest.mark.parametrize("mode", [1, 2, 3, 4])
def test_clean_round_trip_in_every_mode(pkg, mods, mode):
    eti, bits = K.stream(32, K.MULTI, mode)
    check_clean(pkg, mods[mode], eti, bits, mode)


# --------------------------------------------------------------------------- 2. every protection profile
def test_every_accepted_puncture_profile_as_the_only_sub_channel(pkg, mods):
    """The list of test_every_accepted_puncture_case_as_the_only_sub_channel (tests/test_gpu_frontend_gpu.py): with 864 CU (the
    longest trellis, 27 654 steps), 4 CU and the padding-byte profiles.  18 frames in Mode II: three come out."""
    fe = K.cpu_front_end()
    pairs = [p for p in PUNCTURE_CASES if fe.subchannel_profile(*p) is not None]
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "golden.json")))["frontend"]
    assert len(pairs) == gold["puncture_cases"] - 2
    pairs += [(21, 1), (24, 1), (30, 1), (3, 0x23), (432, 0x22)]
    for stl, tpl in pairs:
        eti, bits = K.stream(18, ((0, stl, tpl),), 2, seed=stl * 64 + tpl)
        check_clean(pkg, mods[2], eti, bits, (stl, tpl))


# --------------------------------------------------------------------------- 3. layout shapes
@pytest.mark.parametrize("shape", ["nst0", "twelve_with_gaps", "ends_at_864", "stc_order_is_not_sad_order"])
def test_layout_shapes(pkg, mods, shape):
    eti, bits = K.stream(20, K.SHAPES[shape], 1, seed=78)
    check_clean(pkg, mods[1], eti, bits, shape)


def test_an_overlapping_layout_is_refused_and_the_history_stays(pkg, multi):
    eti, bits, _, ref = multi
    over, over_bits = K.stream(4, K.SHAPES["overlap_last_wins"], 1)
    a, b = pkg.Modulator(mode=1, max_frames=5), pkg.Modulator(mode=1, max_frames=5)
    try:
        a.frontend_configure(over[0])
        with pytest.raises(pkg.DabGpuError, match="overlap at capacity unit 50"):
            a.decode(over_bits)
        # the same context on the stream's layout: three frames, a refused call in between, the rest -- as one call elsewhere
        a.frontend_configure(eti[0])
        first = a.decode(bits[:3], ref[:12])[0]
        out = np.empty(6144, np.uint8)
        ob = C.c_size_t()
        part = np.ascontiguousarray(bits[3:5])
        assert a._lib.dabgpu_decode(a._h, part.ctypes.data, 2, out.ctypes.data, out.nbytes, None, C.byref(ob)) == -4
        assert ob.value == 8 * 6144
        rest = a.decode(bits[3:], ref[12:])[0]
        b.frontend_configure(eti[0])
        assert np.array_equal(np.concatenate([first, rest]), b.decode(bits, ref)[0])
    finally:
        a.close()
        b.close()


# --------------------------------------------------------------------------- 4. against the model, with errors
def _against_the_model(md, multi, got_bits):
    eti, bits, layout, ref = multi
    want_images, want_stats, _ = M.decode_stream(layout, got_bits, ref)
    md.frontend_configure(eti[0])
    images, _ = md.decode(got_bits, ref)
    assert np.array_equal(images, want_images)
    for i in range(20):
        for ui in range(len(want_stats[i])):
            st = md.decode_stats(i, ui)
            assert {k: st[k] for k in want_stats[i][ui]} == want_stats[i][ui], (i, ui)
    return images, want_stats


def test_sparse_errors_are_corrected_and_counted_as_the_model_does(mods, multi):
    eti, bits, layout, _ = multi
    _, fic_out = M.units(layout)
    mask, flips = K.sparse_flips(layout, 20, seed=7)
    images, stats = _against_the_model(mods[1], multi, K.bits_of_rows(M.rows_of(bits, 1, fic_out) ^ mask, 1, fic_out))
    keep = M.payload_mask(layout)
    assert np.array_equal(images[15:][:, keep], eti[:5][:, keep])
    for i in range(15, 20):
        assert [s["corrected"] for s in stats[i]] == flips[i - 15] and sum(flips[i - 15]) > 20


def test_four_percent_errors_give_the_models_bits_and_numpys_error_count(mods, multi):
    """The payload is not recoverable: what is compared is the decoder's wrong answer, tie rule included."""
    eti, bits, layout, ref = multi
    images, stats = _against_the_model(mods[1], multi, bits ^ K.dense_flips(bits.shape, seed=11))
    keep = M.payload_mask(layout)
    md = mods[1]
    total = 0
    for i in range(15, 20):
        errors = int(np.unpackbits(images[i, keep] ^ eti[i - 15, keep]).sum())
        assert md.decode_stats(i)["bit_errors"] == errors and md.decode_stats(i)["n_bits"] == 8 * int(keep.sum())
        total += errors
    assert total > 0


# --------------------------------------------------------------------------- 5. one stream in pieces
def test_a_stream_in_one_call_per_frame_and_in_three_uneven_calls(pkg, mods):
    eti, bits = K.stream(40, K.MULTI, 1, seed=4321)
    noisy = bits ^ K.dense_flips(bits.shape, seed=5, rate=0.01)      # (so that the figures are not all zero)
    ref = K.reference_rows(eti, 40)
    md = mods[1]

    def run(pieces):
        images, stats = [], []
        for a, b in pieces:
            im, _ = md.decode(noisy[a:b], ref[4 * a:4 * b])
            images.append(im)
            stats += [[md.decode_stats(i, u) for u in range(-1, 6)] for i in range(4 * (b - a))]
        return np.concatenate(images), stats

    md.frontend_configure(eti[0])
    one = run([(0, 10)])
    assert one[0][15:].any() and any(s[0]["corrected"] for s in one[1])
    md.decode_reset()
    each = run([(k, k + 1) for k in range(10)])
    md.decode_reset()
    three = run([(0, 3), (3, 4), (4, 10)])
    for other in (each, three):
        assert np.array_equal(other[0], one[0]) and other[1] == one[1]
    # without the reset the next stream's first frames interleave with the old history
    again = run([(0, 5)])
    assert not np.array_equal(again[0], one[0][:20]) and again[1][0][0]["valid"] == 1
    md.decode_reset()
    again = run([(0, 5)])
    assert np.array_equal(again[0], one[0][:20]) and again[1] == one[1][:20]


# --------------------------------------------------------------------------- 6. the device entry
def test_device_entry_on_a_torch_stream_in_two_calls_equals_the_host_entry(mods):
    import torch
    eti, bits = K.stream(24, K.MULTI, 1, seed=5)
    ref = K.reference_rows(eti, 24)
    md = mods[1]
    md.frontend_configure(eti[0])
    want, _ = md.decode(bits, ref)
    want_stats = [md.decode_stats(i) for i in range(8, 24)]
    md.decode_reset()
    dev = torch.device("cuda", 0)
    side = torch.cuda.Stream(device=dev)
    d_out = torch.ones(24 * 6144, dtype=torch.uint8, device=dev)
    with torch.cuda.stream(side):
        d_bits = torch.from_numpy(bits).to(dev)
        d_ref = torch.from_numpy(ref).to(dev)
        n1 = md.decode_dev(d_bits[:2], 2, d_out[:8 * 6144], d_ref[:8], stream=side.cuda_stream)
        n2 = md.decode_dev(d_bits[2:], 4, d_out[8 * 6144:], d_ref[8:], stream=side.cuda_stream)
    side.synchronize()
    assert (n1, n2) == (8 * 6144, 16 * 6144)
    assert np.array_equal(d_out.cpu().numpy().reshape(24, 6144), want)
    assert [md.decode_stats(i) for i in range(16)] == want_stats


# --------------------------------------------------------------------------- 7. the whole loop
def _unit_differences(layout, sent, received):
    """numpy: per (output >= 15, unit) the received coded bits that differ from the sent ones, on the unit's transmitted bits"""
    us, fic_out = M.units(layout)
    diff = M.rows_of(sent ^ received, layout["mode"], fic_out)
    n = diff.shape[0]
    diff = np.concatenate([np.zeros((15, diff.shape[1]), np.uint8), diff])
    return [[int(np.unpackbits(M.punctured(diff, t, u, fic_out))[:u["coded_bits"]].sum()) for u in us] for t in range(15, n)]


@pytest.mark.parametrize("mode,fmt,cfr", [(1, None, False), (1, "s16", False), (3, None, False), (3, "s16", False), (1, None, True)])
def test_eti_to_iq_to_bits_to_eti(pkg, mode, fmt, cfr):
    """ETI -> chain_eti (cfg 3) -> demod -> decode.  Without CFR every coded bit comes back and so does the payload, corrected = 0.
    With CFR (clip 50, error clip 0.1) the channel errors are whatever they are: per (frame, unit) `corrected` is numpy's count
    of differing coded bits of that unit whenever that unit's payload is exact (then the decoded codeword is the sent one), the
    monitor's bit errors are numpy's count over all coded bits -- and where every one of those lies inside a returned unit, the
    two totals are equal."""
    n = 20 if mode == 1 else 18
    eti, bits = K.stream(n, K.MULTI, mode, seed=31)
    n_tf = bits.shape[0]
    md = pkg.Modulator(mode=mode, max_frames=n_tf)
    try:
        md.set_gain(2, 1.0, (32767.0 if fmt else 1.0) / 50000.0, 4.0)
        md.set_fir_taps(None)
        if fmt:
            md.set_output_format(fmt)
        if cfr:
            md.set_cfr(True, 50.0, 0.1)
        md.set_monitor(True)
        md.frontend_configure(eti[0])
        iq = md.chain_eti(eti, G | F)
        monitor = sum(md.monitor_stats(f)["bit_errors"] for f in range(n_tf))
        got = md.demod(iq, early=44)
        layout = pkg.Modulator.frontend_describe(eti[0])
        keep = M.payload_mask(layout)
        us, _ = M.units(layout)
        ref = K.reference_rows(eti, n)
        images, stats = md.decode(got, ref)
        per_unit = [[md.decode_stats(i, ui) for ui in range(len(us))] for i in range(15, n)]
        assert monitor == int(np.unpackbits(got ^ bits).sum())
        if not cfr:
            assert monitor == 0 and np.array_equal(got, bits)
            assert np.array_equal(images[15:][:, keep], eti[:n - 15][:, keep])
            assert all(s["corrected"] == 0 and s["bit_errors"] == 0 for s in stats)
        diff = _unit_differences(layout, bits, got)
        exact = True
        for i, row in enumerate(per_unit):
            for ui, st in enumerate(row):
                if st["bit_errors"] == 0:
                    assert st["corrected"] == diff[i][ui], (i, ui)
                else:
                    exact = False
        print("loop mode %d fmt %s cfr %s: coded-bit errors %d, inside returned units %d, payload exact %s" %
              (mode, fmt, cfr, monitor, sum(map(sum, diff)), exact))
        if exact and monitor == sum(map(sum, diff)):
            assert sum(s["corrected"] for s in stats) == monitor
    finally:
        md.close()


# --------------------------------------------------------------------------- 8. refusals
def test_refusals(pkg, multi):
    eti, bits, _, _ = multi
    md = pkg.Modulator(mode=1, max_frames=4)
    try:
        with pytest.raises(pkg.DabGpuError, match="decode: not configured"):
            md.decode(bits[:1])
        with pytest.raises(pkg.DabGpuError, match="decode: not configured"):
            md.decode_reset()
        with pytest.raises(pkg.DabGpuError, match="no decoder statistics"):
            md.decode_stats(0)
        md.frontend_configure(eti[0])
        with pytest.raises(pkg.DabGpuError, match="max_frames"):
            md.decode(bits)
        out = np.empty(4 * 6144 - 1, np.uint8)
        ob = C.c_size_t()
        one = np.ascontiguousarray(bits[:1])
        assert md._lib.dabgpu_decode(md._h, one.ctypes.data, 1, out.ctypes.data, out.nbytes, None, C.byref(ob)) == -4
        assert ob.value == 4 * 6144
        assert md._lib.dabgpu_decode(md._h, one.ctypes.data, 0, out.ctypes.data, out.nbytes, None, C.byref(ob)) == -1
        images, stats = md.decode(bits[:4])
        assert not images[:15].any() and images[15].any() and [s["valid"] for s in stats] == [0] * 15 + [1]
        with pytest.raises(pkg.DabGpuError, match="unit is -1"):
            md.decode_stats(0, 6)
    finally:
        md.close()


# --------------------------------------------------------------------------- 9. dabmod_file --loopback
def _dabmod_file(fin, fout, opts):
    return subprocess.run([os.path.join(HOST, "dabmod_file"), fin, fout] + opts, capture_output=True, text=True, timeout=300)


@pytest.mark.parametrize("opts", [["--batch", "4", "--fir", "default"], ["--format", "s16", "--normalise", str(32767.0 / 50000.0)]])
def test_dabmod_file_loopback_gives_the_eti_payload_back(tmp_path, opts):
    """40 frames in Mode I: 25 come back from the decoder and are compared; the output file is the one without the option."""
    fin = str(tmp_path / "in.eti")
    synth_eti(40, subchannels=K.MULTI, mid=1).tofile(fin)
    layout_bits = 8 * (96 + 8 * sum(s[1] for s in K.MULTI))
    outs = []
    for loop in ([], ["--loopback"]):
        fout = str(tmp_path / ("out%d" % len(outs)))
        r = _dabmod_file(fin, fout, ["--gpu-frontend"] + opts + loop)
        assert r.returncode == 0, r.stderr[-2000:]
        assert r.stdout.split() == ["40", "10", "10"]
        outs.append(np.fromfile(fout, np.uint8))
        line = "loopback: 25 frames compared, 0 FIC and 0 MSC payload bit errors in %d bits, 0 corrected channel bits in" % (25 * layout_bits)
        assert (line in r.stderr) == bool(loop), r.stderr
    assert outs[0].size and np.array_equal(outs[0], outs[1])


def test_dabmod_file_loopback_is_refused_without_the_device_front_end(tmp_path):
    fin, fout = str(tmp_path / "in.eti"), str(tmp_path / "out")
    synth_eti(8).tofile(fin)
    for opts, word in (([], "--gpu-frontend"), (["--gpu-frontend", "--format", "u8"], "u8 / s8"),
                       (["--gpu-frontend", "--rate", "4096000"], "--rate")):
        r = _dabmod_file(fin, fout, ["--loopback"] + opts)
        assert r.returncode == 2 and r.stderr.startswith("dabmod_file: --loopback does not go with") and word in r.stderr
        assert not os.path.exists(fout)
