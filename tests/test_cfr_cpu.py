"""Crest-factor reduction across its clip / error-clip range, on the CPU: the oracle against the float64 model
(tests/cfr_model.py) on every input and regime of tests/cfr_cases.py, the regimes being what their names say, and the
ambiguity sets staying as small as tests/test_cfr_gpu.py needs them."""
import numpy as np
import pytest

import oracle as O
from tests import cfr_cases as CC
from tests.cfr_model import AMBIGUITY_CAP, TAU_CLIP, TAU_ERR

MER_INDEX = 5


def _ids(v):
    return "m%d-%s" % v if isinstance(v, tuple) else str(v)


@pytest.mark.parametrize("regime", list(CC.REGIMES))
@pytest.mark.parametrize("inp", CC.INPUTS, ids=_ids)
def test_oracle_against_the_float64_model(inp, regime):
    mode, kind = inp
    K, N, nsym = CC.geometry(mode)
    clip, eclip = CC.thresholds(regime, K)
    for f, z in enumerate(CC.carriers(mode, kind)):
        m = CC.models(mode, kind, regime)[f]
        y, st, papr = O.ofdm_generate_cfr(z, nsym, K, N, clip, eclip, MER_INDEX)
        assert np.isfinite(y.view(np.float32)).all()
        assert np.linalg.norm(y - m.y.ravel()) / np.linalg.norm(m.y) < 2e-7
        # a decision may differ only where the magnitude lies within tau of the threshold
        assert abs(st["num_clip"] - m.num_clip) <= m.n_amb_clip, (st["num_clip"], m.num_clip, m.n_amb_clip)
        assert abs(st["num_error_clip"] - m.num_error_clip) <= m.n_amb_err, (st["num_error_clip"], m.num_error_clip, m.n_amb_err)
        # the cap: a condition on the inputs (an input that breaks it gets another seed), half of the 0.2 % the older tests allow
        assert m.n_amb_clip <= AMBIGUITY_CAP * m.num_samples and m.n_amb_err <= AMBIGUITY_CAP * m.num_samples
        assert np.allclose(papr[:, :2], m.papr_before, rtol=1e-5, atol=1e-12)
        assert np.allclose(papr[1:, 2:], m.papr_after[1:], rtol=1e-5, atol=1e-12) and not papr[0, 2:].any()
        assert st["mer_sum_iq"] == pytest.approx(m.mer_iq[MER_INDEX], rel=1e-5)
        if m.num_error_clip:
            assert st["mer_db"] == pytest.approx(10 * np.log10(m.mer_iq[MER_INDEX] / m.mer_delta[MER_INDEX]), abs=1e-3)
        else:
            assert st["mer_sum_delta"] <= (3e-6) ** 2 * st["mer_sum_iq"] and m.mer_delta[MER_INDEX] <= 1e-20 * m.mer_iq[MER_INDEX]


@pytest.mark.parametrize("inp", CC.INPUTS, ids=_ids)
def test_regimes_are_what_the_table_says(inp):
    """On the float64 model.  The shares ("about 20 % / 70 %") belong to DAB symbols -- unit carriers, blank null symbol --, the
    exact statements hold for arbitrary carriers too."""
    mode, kind = inp
    K, N, nsym = CC.geometry(mode)
    dab = kind == "bits"
    for f in range(CC.FRAMES):
        M = {r: CC.models(mode, kind, r)[f] for r in CC.REGIMES}
        live = M["base"].live
        n_live = int(live.sum()) * N
        assert int(live.sum()) == (nsym - 1 if dab else nsym)
        share = lambda r: (M[r].num_clip / n_live, M[r].num_error_clip / n_live)
        inband = np.zeros(N, bool)
        inband[1:K // 2 + 1] = inband[N - K // 2:] = True

        assert M["off_high"].num_clip == 0 and M["off_high"].num_error_clip == 0
        assert M["clip_only"].num_clip == M["base"].num_clip > 0 and M["clip_only"].num_error_clip == 0
        assert np.abs(M["clip_only"].y - M["clip_only"].t).max() < 1e-10          # CFR undoes itself
        assert share("all_clip")[0] >= 0.999
        assert M["err_zero"].num_error_clip == n_live and not M["err_zero"].eclipped[~live].any()
        assert M["light"].num_error_clip == 0 and M["light"].num_clip > 0
        assert np.array_equal(M["clip_zero"].clipped, M["clip_zero"].mag > 0)
        assert M["clip_zero"].num_clip >= (1 - AMBIGUITY_CAP) * n_live
        for k in ("clipped", "eclipped", "y"):
            assert np.array_equal(getattr(M["negative"], k), getattr(M["base"], k))
        if dab:
            assert 0.18 < share("base")[0] < 0.22 and 0.66 < share("base")[1] < 0.73
            assert 0.63 < share("heavy")[0] < 0.70 and 0.99 < share("heavy")[1] < 1.0
            assert 0.010 < share("light")[0] < 0.022
            for r in ("all_clip", "clip_zero"):                                    # in-band bins all error-clipped, out-of-band none
                assert np.array_equal(M[r].eclipped, live[:, None] & inband[None, :])
            # every sample to zero, every carrier to error_clip: the symbol again at a tenth of its size (the carriers are
            # fp32 unit vectors, 1 +- 6e-8 long: 1e-5 on samples of up to 150)
            assert np.abs(M["clip_zero"].y - 0.1 * M["clip_zero"].t).max() < 1e-5
        # the ambiguity sets are empty where the GPU tests say "exactly equal"
        for r in ("off_high", "err_zero", "all_clip"):
            assert M[r].n_amb_clip == 0 and M[r].n_amb_err == 0, r


@pytest.mark.parametrize("inp", CC.INPUTS, ids=_ids)
def test_oracle_squares_the_thresholds(inp):
    """`negative` is `base` in the reference (clip * clip, error_clip * error_clip): bytes and statistics."""
    mode, kind = inp
    K, N, nsym = CC.geometry(mode)
    z = CC.carriers(mode, kind)[0]
    (c0, e0), (c1, e1) = CC.thresholds("base", K), CC.thresholds("negative", K)
    assert (c1, e1) == (-c0, -e0)
    a, b = O.ofdm_generate_cfr(z, nsym, K, N, c0, e0, MER_INDEX), O.ofdm_generate_cfr(z, nsym, K, N, c1, e1, MER_INDEX)
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and a[1] == b[1] and np.array_equal(a[2], b[2])


def test_the_taus_come_from_existing_bars():
    assert TAU_CLIP == 2e-5 and TAU_ERR == pytest.approx(TAU_CLIP + 1e-6) and AMBIGUITY_CAP == 1e-3


def test_subnormal_powers_on_the_oracle():
    """Mode II symbols times 1e-21, both thresholds 0: |t|^2 is subnormal or underflows; the reference's arithmetic stays finite."""
    K, N, nsym = CC.geometry(2)
    z = (CC.carriers(2, "bits")[0] * np.float32(1e-21)).astype(np.complex64)
    y, st, _ = O.ofdm_generate_cfr(z, nsym, K, N, 0.0, 0.0, 1)
    assert np.isfinite(y.view(np.float32)).all() and np.abs(y).max() <= 1e-18
    assert st["num_clip"] <= nsym * N and st["num_error_clip"] <= nsym * N


def test_form_table_covers_every_cfr_form():
    names = [f.name for f in CC.FORMS]
    assert len(set(names)) == len(names) == 18
    assert {f.mode for f in CC.FORMS if f.entry == "ofdm"} == {1, 2, 3, 4}
    assert {(f.mode, f.kind) for f in CC.FORMS} <= set(CC.INPUTS)
