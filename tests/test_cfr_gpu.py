"""Crest-factor reduction on the device across its clip / error-clip range: every form of the frame kernel that runs it
(tests/cfr_cases.py::FORMS) x every regime (REGIMES), against the CPU oracle and the float64 model (tests/cfr_model.py).

What is asserted, per case and frame:
  1. rel-RMS per frame < 1e-6 against the oracle (the project's bar);
  2. the same bar per live SYMBOL (one bad symbol of 76 hides in a frame's figure); the worst one is logged (record_bound);
  3. the clip / error-clip counts differ from the model's by at most the size of the model's ambiguity set -- exactly equal where
     that set is empty; num_samples exact;
  4. papr_before / papr_after at rtol 2e-5 against the oracle; symbol 0's papr_after exactly {0, 0};
  5. MER: within 1e-2 dB of the oracle where the model clips error bins; where it clips none, the oracle's delta is exactly 0
     and the device's is what three fp32 transforms at the 1e-6 bar leave: mer_sum_delta <= (3e-6)^2 mer_sum_iq (MER >= 110 dB),
     mer_sum_iq at rtol 2e-5 of the model's;
  6. clip_only / off_high: also within the bar, per symbol, of the oracle WITHOUT crest-factor reduction;
  7. negative: the bytes and statistics of the `base` run on the same context;
  8. a second call with the same settings: the same bytes and counts (and the MER of the next two symbol indices).
The s16 forms hold 1, 2 and 6 in integers: never more than one step from FormatConverter on the oracle's frames, and that as
rarely as tests/conftest.py::int_off_by_one_limit says.  Every case asserts the kernels it launched against the rule book of
tests/test_dispatch_matrix.py.  record_bound logs every measured figure; with DABGPU_CFR_TABLE=<file> in the
environment the worst ones per form and regime are written there as a table (committed as profiles/cfr_regimes.txt)."""
import functools
import os

import numpy as np
import pytest

import oracle as O
from tests import cfr_cases as CC
from tests.conftest import int_off_by_one_limit, record_bound
from tests.golden.synth import synth_bits, synth_signal
from tests.test_dispatch_matrix import LOGN, expected_kernels, tf

pytestmark = pytest.mark.gpu

REL_RMS = 1e-6
MER_DELTA_BAR = (3e-6) ** 2          # three fp32 transforms at the 1e-6 bar between `before` and `after`
_rows = []


@pytest.fixture(scope="module", autouse=True)
def _table():
    yield
    path = os.environ.get("DABGPU_CFR_TABLE")               # (a file to write the table of measured figures to; unset: none)
    if _rows and path:
        with open(path, "w") as f:
            f.write("# form regime | worst frame rel-RMS (s16 forms: share of the components one step off) | worst symbol rel-RMS "
                    "(s16: none) | counts - model (clip, error clip), worst frame [ambiguity set sizes] | MER: worst |dB - oracle|, "
                    "or worst delta / iq where no error bin clips\n")
            f.write("\n".join(_rows) + "\n")


def rel_rms(y, ref):
    return float(np.linalg.norm(y.astype(np.complex128) - ref) / max(np.linalg.norm(ref), 1e-30))


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype.itemsize % 4 == 0 else np.uint16)


def rule_book(form, cfr=True):
    if form.entry == "ofdm":
        return [tf(LOGN[form.mode], 0, 0, 0, 0, cfr=int(cfr), bits=0)]
    k = expected_kernels(form.mode, 2 if form.gain else None, form.fir, form.overlap, cfr, False, form.fmt)
    return [s.replace("bits=1", "bits=0") for s in k] if form.entry == "symbols" else k


def context(pkg, form, frames=CC.FRAMES):
    md = pkg.Modulator(mode=form.mode, max_frames=frames, chunks_per_frame=form.chunks)
    md.trace(True)
    md.set_gain(2, 1.0, form.normalise, 4.0)
    if form.fir:
        md.set_fir_taps(None if form.fir == 45 else CC.taps_of(form.fir))
    md.set_window_overlap(form.overlap)
    md.set_output_format(form.fmt)
    return md


def run(md, form, z=None, bits=None):
    """The form's frames on the device: (frames, [statistics per frame], kernels launched)."""
    if form.entry == "ofdm":                                  # one frame per call
        z = CC.carriers(form.mode, form.kind) if z is None else z
        ys, stats = [], []
        for zf in z:
            ys.append(md.ofdm(zf))
            stats.append(md.cfr_stats(0))
        return np.stack(ys), stats, md.last_variant()
    if form.entry == "chain":
        y = md.chain(CC.bits_of(form.mode) if bits is None else bits, form.stages)
    else:
        import torch
        z = CC.carriers(form.mode, form.kind) if z is None else z
        n = len(z)
        d_out = torch.empty(n * md.out_samples_per_frame(form.stages), dtype=torch.complex64, device="cuda")
        md.symbols_dev(torch.from_numpy(np.array(z)).cuda(), n, form.stages, d_out)
        torch.cuda.synchronize()
        y = d_out.cpu().numpy().reshape(n, -1)
    return y, [md.cfr_stats(f) for f in range(len(y))], md.last_variant()


@functools.lru_cache(maxsize=2)
def oracle_without_cfr(form):
    return [CC.oracle_frame(form, z, None)[0] for z in CC.carriers(form.mode, form.kind)]


def check_mer(tag, got, idx, st, model, no_error_clip):
    """Rule 5 on one frame; returns the logged figure."""
    assert got["mer_symbol"] == idx
    if idx == 0:                                              # the reference takes no MER of symbol 0
        assert got["mer_sum_iq"] == 0.0 and got["mer_sum_delta"] == 0.0
        return 0.0
    if no_error_clip:
        assert model.num_error_clip == 0
        assert got["mer_sum_iq"] == pytest.approx(model.mer_iq[idx], rel=2e-5)
        ratio = got["mer_sum_delta"] / got["mer_sum_iq"]
        assert record_bound("cfr MER delta / iq with no error bin clipped, " + tag, ratio, MER_DELTA_BAR)
        return ratio
    mer = 10 * np.log10(got["mer_sum_iq"] / got["mer_sum_delta"])
    assert abs(mer - st["mer_db"]) < 1e-2, (mer, st["mer_db"])
    return abs(mer - st["mer_db"])


def check_samples(form, tag, y, ref, live):
    """Rules 1 and 2 (complexf), or the integer rule (s16), on one frame against `ref`; returns (frame, worst symbol) figures."""
    N = CC.geometry(form.mode)[1]
    if form.fmt:
        want, _ = O.format_convert(ref, form.fmt)
        d = np.abs(y.reshape(-1).astype(np.int32) - want.reshape(-1).astype(np.int32))
        share = float((d != 0).mean())
        assert d.max() <= 1
        assert record_bound("cfr s16 components one step from the oracle's, " + tag, share, int_off_by_one_limit(want, N, form.fmt))
        return share, float("nan")
    frame = rel_rms(y, ref)
    assert frame < REL_RMS, (tag, frame)
    per_symbol = [rel_rms(y[a:b], ref[a:b]) for s, (a, b) in enumerate(CC.segments(form)) if live[s]]
    worst = max(per_symbol)
    assert record_bound("cfr worst symbol rel-RMS, " + tag, worst, REL_RMS), (tag, int(np.argmax(per_symbol)), worst)
    return frame, worst


def check_stats(got, st, papr, model):
    """Rules 3 and 4 on one frame; returns the count differences."""
    dc, de = int(got["num_clip"]) - model.num_clip, int(got["num_error_clip"]) - model.num_error_clip
    assert abs(dc) <= model.n_amb_clip, (got["num_clip"], model.num_clip, model.n_amb_clip)
    assert abs(de) <= model.n_amb_err, (got["num_error_clip"], model.num_error_clip, model.n_amb_err)
    assert got["num_samples"] == model.num_samples
    assert np.allclose(got["papr_before"], papr[:, :2], rtol=2e-5, atol=1e-12)
    assert np.allclose(got["papr_after"], papr[:, 2:], rtol=2e-5, atol=1e-12)
    assert not got["papr_after"][0].any()
    return dc, de


def same_statistics(a, b):
    return all(a[k] == b[k] for k in ("num_clip", "num_error_clip", "num_samples")) and \
        np.array_equal(a["papr_before"], b["papr_before"]) and np.array_equal(a["papr_after"], b["papr_after"])


@pytest.mark.parametrize("regime", list(CC.REGIMES))
@pytest.mark.parametrize("form", CC.FORMS, ids=repr)
def test_cfr_form_in_regime(pkg, form, regime):
    K, N, nsym = CC.geometry(form.mode)
    clip, eclip = CC.thresholds(regime, K)
    z = CC.carriers(form.mode, form.kind)
    models = CC.models(form.mode, form.kind, regime)
    no_error_clip = regime in CC.NO_ERROR_CLIP
    tag0 = "%s %s" % (form.name, regime)
    md = context(pkg, form)
    try:
        # (negative: the first run is `base`, the second the negated thresholds -- the reference squares them)
        first = CC.thresholds("base", K) if regime == "negative" else (clip, eclip)
        md.set_cfr(True, *first)
        y, stats, kernels = run(md, form)
        assert kernels == rule_book(form), "kernels launched %s, the rule book says %s" % (kernels, rule_book(form))
        assert y.shape[0] == CC.FRAMES and np.isfinite(y.astype(np.float64) if form.fmt else y.view(np.float32)).all()
        worst = dict(frame=0.0, symbol=0.0, dc=0, de=0, mer=0.0)
        for f in range(CC.FRAMES):
            tag = "%s frame %d" % (tag0, f)
            ref, st, papr = CC.oracle_frame(form, z[f], (clip, eclip), CC.mer_indices(form, 0)[f])
            a, b = check_samples(form, tag, y[f], ref, models[f].live)
            if not form.guard and not models[f].live[0]:
                assert not y[f][:N].any()                     # a blank null symbol stays exactly zero
            if regime in ("clip_only", "off_high"):            # rule 6: the analytic property, independent of the CFR oracle
                check_samples(form, tag + ", against the chain without CFR", y[f], oracle_without_cfr(form)[f], models[f].live)
            dc, de = check_stats(stats[f], st, papr, models[f])
            m = check_mer(tag, stats[f], CC.mer_indices(form, 0)[f], st, models[f], no_error_clip)
            worst = dict(frame=max(worst["frame"], a), symbol=max(worst["symbol"], b), mer=max(worst["mer"], m),
                         dc=max(worst["dc"], dc, key=abs), de=max(worst["de"], de, key=abs))
        # rules 7 and 8: once more (negative: now with the negated thresholds)
        md.set_cfr(True, clip, eclip)
        y2, stats2, kernels2 = run(md, form)
        assert kernels2 == kernels
        assert np.array_equal(u32(y2), u32(y))
        for f in range(CC.FRAMES):
            assert same_statistics(stats2[f], stats[f])
            idx = CC.mer_indices(form, 1)[f]
            _, st, _ = O.ofdm_generate_cfr(z[f], nsym, K, N, clip, eclip, idx)
            check_mer("%s frame %d, second call" % (tag0, f), stats2[f], idx, st, models[f], no_error_clip)
        _rows.append("%-26s %-9s | %.2e | %8s | %+d %+d [%d %d] | %.2e" % (
            form.name, regime, worst["frame"], "-" if form.fmt else "%.2e" % worst["symbol"], worst["dc"], worst["de"],
            max(m.n_amb_clip for m in models), max(m.n_amb_err for m in models), worst["mer"]))
    finally:
        md.close()


# --------------------------------------------------------------------------- directed tests
def test_mer_symbol_index_wraps_through_symbol_0(pkg):
    """The MER symbol of frame f is (index + 1 + f) % nsym, the index running on from call to call (src/OfdmGenerator.cpp:198);
    when it is 0 the reference takes no MER (:250).  Mode II (nsym 77), 80 frames in one call, then 3 more."""
    form = CC.Form("wrap", 2, "chain")
    K, N, nsym = CC.geometry(2)
    cfr = CC.thresholds("base", K)
    n1, n2 = 80, 3
    bits = np.stack([synth_bits(O.tf_input_bytes(2), seed=3100 + f) for f in range(n1 + n2)])
    z = CC.carriers_of_bits(2, bits)
    md = pkg.Modulator(mode=2, max_frames=n1)
    try:
        md.trace(True)
        md.set_cfr(True, *cfr)
        for first, n in ((0, n1), (n1, n2)):
            y = md.chain(bits[first:first + n], 0)
            assert md.last_variant() == rule_book(form)
            for f in range(n):
                idx = (first + f + 1) % nsym
                got = md.cfr_stats(f)
                ref, st, papr = CC.oracle_frame(form, z[first + f], cfr, idx)
                assert rel_rms(y[f], ref) < REL_RMS
                model = CC.cfr_model(z[first + f], nsym, K, N, *cfr)
                check_stats(got, st, papr, model)
                check_mer("MER index wrap, frame %d" % (first + f), got, idx, st, model, False)
        assert (76 + 1) % nsym == 0 and (77 + 1) % nsym == 1 and (n1 + 1) % nsym == 4     # the frames the test is about
    finally:
        md.close()


def test_energy_in_symbol_0(pkg):
    """Symbol 0 with energy goes through CFR too: its clips count, its papr_before is taken, its papr_after and MER are not --
    through md.ofdm, and through symbols_dev in a call long enough (77 frames) for the MER index to reach 0."""
    K, N, nsym = CC.geometry(2)
    z = synth_signal(nsym * K, seed=21) * np.float32(1 / 40)
    cfr = (25.0, 0.1)
    model = CC.cfr_model(z, nsym, K, N, *cfr)
    in_symbol_0 = int(model.clipped[0].sum())
    assert model.live[0] and in_symbol_0 > 100 + model.n_amb_clip           # a count without symbol 0's would miss the rule
    # ---- OfdmGenerator alone
    form = CC.Form("ofdm", 2, "ofdm")
    md = context(pkg, form, 1)
    try:
        md.set_cfr(True, *cfr)
        y, stats, kernels = run(md, form, z=[z])
        assert kernels == rule_book(form)
        ref, st, papr = CC.oracle_frame(form, z, cfr, 1)
        check_samples(form, "energy in symbol 0, ofdm", y[0], ref, model.live)
        check_stats(stats[0], st, papr, model)
        assert stats[0]["papr_before"][0].all()
        check_mer("energy in symbol 0, ofdm", stats[0], 1, st, model, False)
    finally:
        md.close()
    # ---- the carriers entry with gain and FIRFilter, 77 frames: frame 76 has MER index 0
    form = CC.Form("symbols", 2, "symbols", gain=True, fir=45)
    md = context(pkg, form, nsym)
    try:
        md.set_cfr(True, *cfr)
        y, stats, kernels = run(md, form, z=[z] * nsym)
        assert kernels == rule_book(form)
        for f in (0, nsym - 2, nsym - 1):
            idx = (f + 1) % nsym
            ref, st, papr = CC.oracle_frame(form, z, cfr, idx)
            check_samples(form, "energy in symbol 0, symbols frame %d" % f, y[f], ref, model.live)
            check_stats(stats[f], st, papr, model)
            assert stats[f]["papr_before"][0].all()
            check_mer("energy in symbol 0, symbols frame %d" % f, stats[f], idx, st, model, False)
        assert stats[nsym - 1]["mer_symbol"] == 0
    finally:
        md.close()


def test_subnormal_powers(pkg):
    """Mode II symbols times 1e-21 with both thresholds 0: |x|^2 is subnormal or underflows, and a factor 0 * rsq(|x|^2) formed
    from a reciprocal square root that flushes its argument would be 0 * inf.  Subnormal arithmetic is not held to equality
    with the oracle (which gives finite output of order 1e-23): every float finite, nothing grown, counts possible."""
    form = CC.Form("ofdm", 2, "ofdm")
    K, N, nsym = CC.geometry(2)
    z = (CC.carriers(2, "bits")[0] * np.float32(1e-21)).astype(np.complex64)
    md = context(pkg, form, 1)
    try:
        md.set_cfr(True, 0.0, 0.0)
        y, stats, kernels = run(md, form, z=[z])
        assert kernels == rule_book(form)
        assert np.isfinite(y.view(np.float32)).all()
        assert np.abs(y).max() <= 1e-18
        assert stats[0]["num_samples"] == nsym * N
        assert stats[0]["num_clip"] <= nsym * N and stats[0]["num_error_clip"] <= nsym * N
        assert np.isfinite(stats[0]["papr_before"]).all() and np.isfinite(stats[0]["papr_after"]).all()
        assert np.isfinite(stats[0]["mer_sum_iq"]) and np.isfinite(stats[0]["mer_sum_delta"])
    finally:
        md.close()


def test_threshold_change_between_calls(pkg):
    """The thresholds are kernel arguments an operator moves live: base -> heavy -> base on one context is what three fresh
    contexts give, byte for byte; and CFR switched off after all_clip leaves the bytes of a context that never had it."""
    form = next(f for f in CC.FORMS if f.name == "bits_fir45-m1")
    K = CC.geometry(1)[0]

    def fresh(regime):
        md = context(pkg, form)
        try:
            md.set_cfr(regime is not None, *(CC.thresholds(regime, K) if regime else (1.0, 1.0)))
            y, _, kernels = run(md, form) if regime else (md.chain(CC.bits_of(1), form.stages), None, md.last_variant())
            assert kernels == rule_book(form, cfr=regime is not None)
            return y
        finally:
            md.close()

    want = {r: fresh(r) for r in ("base", "heavy", "all_clip", None)}
    assert not np.array_equal(u32(want["base"]), u32(want["heavy"]))
    md = context(pkg, form)
    try:
        for regime in ("base", "heavy", "base", "all_clip"):
            md.set_cfr(True, *CC.thresholds(regime, K))
            y, stats, _ = run(md, form)
            assert np.array_equal(u32(y), u32(want[regime])), regime
        md.set_cfr(False)
        y = md.chain(CC.bits_of(1), form.stages)
        assert md.last_variant() == rule_book(form, cfr=False)
        assert np.array_equal(u32(y), u32(want[None]))
    finally:
        md.close()
