"""The channel decoder without a device: the numpy model (tests/decode_model.py) that the GPU tests compare the kernel with,
bit for bit, must itself be right -- it returns the ETI payload from the CPU front-end's coded bits and corrects isolated
errors; the layout check (dabgpu_decode_check_layout: host code) and the header's surface."""
import os
import re

import numpy as np
import pytest

from tests import decode_cases as K
from tests import decode_model as M
from tests.conftest import ROOT, load_pkg

ENTRIES = ("dabgpu_decode_check_layout", "dabgpu_decode_reset", "dabgpu_decode_dev", "dabgpu_decode", "dabgpu_get_decode_stats")


@pytest.fixture(scope="module")
def pkg():
    p = load_pkg()
    p.build()
    return p


def _round_trip(pkg, n, subchannels, mode, seed=1234):
    eti, bits = K.stream(n, subchannels, mode, seed)
    layout = pkg.Modulator.frontend_describe(eti[0])
    images, stats, valid = M.decode_stream(layout, bits)
    keep = M.payload_mask(layout)
    assert images.shape == (n, 6144) and valid.sum() == n - 15 and not images[:15].any()
    assert np.array_equal(images[15:][:, keep], eti[:n - 15][:, keep])
    assert not images[:, ~keep].any()
    us, _ = M.units(layout)
    for i in range(n):
        for ui, u in enumerate(us):
            assert stats[i][ui]["corrected"] == 0
            assert stats[i][ui]["coded_bits"] == (u["coded_bits"] if valid[i] else 0)


def test_model_returns_the_payload_of_the_multi_layout_in_mode_1(pkg):
    _round_trip(pkg, 20, K.MULTI, 1)


@pytest.mark.parametrize("stl,tpl", K.PADDING_AND_SMALLEST)
def test_model_returns_the_payload_of_the_padding_byte_profiles_and_the_smallest_sub_channel(pkg, stl, tpl):
    _round_trip(pkg, 18, ((0, stl, tpl),), 2, seed=stl * 64 + tpl)


def test_model_corrects_one_flip_per_512_transmitted_bits_and_counts_them(pkg):
    """An isolated flip on a code of free distance 10 leaves every competitor at distance >= 9 against 1: the payload comes
    back exactly and `corrected` is the number of flips inside each unit -- a property of the code, not a tolerance."""
    n = 20
    eti, bits = K.stream(n, K.MULTI, 1)
    layout = pkg.Modulator.frontend_describe(eti[0])
    us, fic_out = M.units(layout)
    mask, flips = K.sparse_flips(layout, n, seed=7)
    assert sum(map(sum, flips)) > 100 and any(flips[0][ui] == 0 for ui in range(1, len(us)))      # (some units are left alone)
    got = K.bits_of_rows(M.rows_of(bits, 1, fic_out) ^ mask, 1, fic_out)
    assert got.shape == bits.shape and np.unpackbits(got ^ bits).sum() > 100
    ref = K.reference_rows(eti, n)
    images, stats, valid = M.decode_stream(layout, got, ref)
    keep = M.payload_mask(layout)
    assert np.array_equal(images[15:][:, keep], eti[:n - 15][:, keep])
    for i in range(15, n):
        assert [s["corrected"] for s in stats[i]] == flips[i - 15], i
        assert all(s["bit_errors"] == 0 and s["n_bits"] == 8 * u["in_bytes"] for s, u in zip(stats[i], us))


def test_check_layout_accepts_the_front_end_shapes_and_refuses_an_overlap(pkg):
    for name, subs in K.SHAPES.items():
        frame = K.synth_eti(1, subchannels=subs, mid=1)[0]
        if name == "overlap_last_wins":
            with pytest.raises(pkg.DabGpuError, match="sub-channels 0 and 1 of the STC list overlap at capacity unit 50"):
                pkg.decode_check_layout(frame)
        else:
            pkg.decode_check_layout(frame)
    pkg.decode_check_layout(K.synth_eti(1, subchannels=K.MULTI, mid=1)[0])


def test_header_declares_the_five_entries_and_none_is_a_process_entry(pkg):
    text = open(os.path.join(ROOT, "include", "dabgpu.h")).read()
    names = set(re.findall(r"DABGPU_API[^;]*?\b(dabgpu_[a-z_0-9]+)\s*\(", text, re.S))
    for name in ENTRIES:
        assert name in names and name in pkg.EXPORTS and not name.endswith("_process")
    assert not [n for n in names if "decode" in n and n.endswith("_process")]
    assert "typedef struct dabgpu_decode_stats" in text
