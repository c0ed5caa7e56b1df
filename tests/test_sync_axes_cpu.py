"""The swept families of tests/sync_cases.py without a device.  tests/test_sync_axes_gpu.py asserts on every capture of every
family that the device's integers EQUAL the float64 model's; that can be asked only where no decision of the model is close:

* coarse start: the device adds its block powers in fp32 (relative error about B 2^-24, at most 4e-6), the model in float64.
  The chosen window's S is exactly 0, or lower than EVERY other window's, adjacent ones included, by 1e-3 of it: 250 times that
  error.
* integer offset and fine start: the runner-up |D|^2, and the runner-up |c|^2 beyond +-1 sample, are at most 0.6 of the peak
  (the fp32 transform's error is 1.1e-7).
* eps is at least 1e-3 away from +-1/2, where shift and eps trade a whole spacing.

These are conditions on the captures, never measurements of the device; a capture that misses one is changed, the condition is
not.  Then what each family states: the expected slots, starts and validity of every candidate (Cap.expect, worked out from
where the capture was cut), the shifts, shift + eps, the search range's ends, and that the model's extracted frames decode to
the chain's bits through the numpy receiver wherever Cap.receiver says the receivers behind the synchroniser are to be asked."""
import numpy as np
import pytest

from tests import sync_cases as SY
from tests.receiver import dab_demodulate
from tests.sync_model import geometry

S_WIN = 1e-3
RUNNER_UP = 0.6
EPS_EDGE = 1e-3
COUNTS = {"A_noise": {1: 38, 2: 38, 3: 22, 4: 38}, "A_clean": {1: 38, 2: 38, 3: 22, 4: 38}, "B": dict.fromkeys((1, 2, 3, 4), 29),
          "C": {1: 4, 2: 10, 3: 12, 4: 3}, "D": dict.fromkeys((2, 3, 4), 1), "E": dict.fromkeys((1, 2, 3, 4), 5),
          "F": dict.fromkeys((1, 2), 1), "G": dict.fromkeys((1, 2, 3, 4), 1)}


def test_slack_and_the_family_table():
    assert [SY.slack(m) for m in (1, 2, 3, 4)] == [32, 8, 1, 16]
    assert {f: dict((m, len(SY.family(f, m))) for m in SY.FAMILIES[f][0]) for f in SY.FAMILIES} == COUNTS
    for f, m in SY.FAMILY_MODES:
        labels = [c.label for c in SY.family(f, m)]
        assert len(set(labels)) == len(labels), (f, m)


def test_the_family_chain_is_the_chain_of_the_named_cases():
    """Mode II, cfg 2: the first three frames of the five-frame chain are the three frames m2_clean was cut from."""
    x, mode, bits, start, _ = SY.named("m2_clean")
    y, fbits = SY.family_chain(mode)
    tf = geometry(mode)["tf"]
    assert start == 0 and np.array_equal(fbits[:2], bits)
    assert np.array_equal(np.asarray(x[:2 * tf]), y[:2].reshape(-1))


@pytest.mark.parametrize("fam,mode", SY.FAMILY_MODES)
def test_every_capture_meets_the_conditions_and_what_its_family_states(fam, mode):
    g = geometry(mode)
    tf = g["tf"]
    worst = dict(win=1.0, d=0.0, c=0.0, edge=0.5)
    shifts = {}
    for c in SY.family(fam, mode):
        x = SY.family_capture(c)
        n = SY.n_samples(x)
        r = SY.family_model(c, x)
        # the conditions
        win = 1.0 if r["s_lowest"] == 0.0 else (r["s_next"] - r["s_lowest"]) / r["s_next"]
        assert win >= S_WIN, (c.label, win)
        worst["win"] = min(worst["win"], win)
        for fr, mg in zip(r["frames"], r["margins"]):
            assert mg["d_runner_up"] <= RUNNER_UP and mg["c_runner_up"] <= RUNNER_UP, (c.label, mg)
            assert 0.5 - abs(fr["eps"]) >= EPS_EDGE, (c.label, fr)
            worst.update(d=max(worst["d"], mg["d_runner_up"]), c=max(worst["c"], mg["c_runner_up"]),
                         edge=min(worst["edge"], 0.5 - abs(fr["eps"])))
        # slots, candidates, starts, validity
        assert (r["slots"], tuple((fr["start"], fr["valid"]) for fr in r["frames"])) == c.expect, (c.label, r["frames"])
        assert r["n_frames"] == len(c.expect[1]) <= r["slots"] == min(c.max_frames, n // tf)
        assert all(fr["valid"] == int(fr["start"] >= 0 and fr["start"] + tf <= n) for fr in r["frames"])
        assert all((fr["start"] - c.start + (g["N"] if c.gap else 0)) % tf == 0 for fr in r["frames"])
        assert r["extracted"].shape == (r["slots"], tf)
        # offsets
        for fr in r["frames"] if not c.gap else ():     # (N / 2 off, the cyclic prefixes are not where eps is taken from)
            assert abs(fr["shift"]) <= c.max_shift and fr["shift"] == int(np.rint(c.cfo)), (c.label, fr)
            if c.echo is None:                     # (an echo of a rotating signal pulls the estimate: up to 2.2e-3 in E)
                assert abs(fr["shift"] + fr["eps"] - c.cfo) <= 1e-3, (c.label, fr)
            shifts.setdefault(c.max_shift, set()).add(fr["shift"])
        # zeros, and the receiver behind it
        for k in range(r["slots"]):
            fr = r["frames"][k] if k < r["n_frames"] else None
            if fr is None or not fr["valid"]:
                assert not r["extracted"][k].any(), (c.label, k)
            elif c.receiver:
                bits = SY.family_frame_bits(c, fr["start"])
                assert bits is not None, (c.label, k)
                assert np.array_equal(dab_demodulate(r["extracted"][k], mode, g["CP"] // 2), bits), (c.label, k)
        if fam == "D":
            assert x.dtype == np.int16 and min(fr["quality"] for fr in r["frames"]) >= 0.98
            rms = float(np.sqrt(np.mean(x.astype(np.float64).reshape(-1, 2)[c.start + g["null"]:c.start + tf] ** 2) * 2.0))
            assert 1000.0 <= rms <= 4000.0 and np.abs(x.astype(np.int32)).max() < 32767, rms    # (fine steps, no clipping)
        if fam == "F":
            assert 0.01 <= r["null_depth"] <= 0.1, r["null_depth"]              # (the null symbol is not empty)
    print("sync axes %s mode %d: worst win of the chosen window %.3g, runner-up D %.3g c %.3g, 0.5 - |eps| %.3g"
          % (fam, mode, worst["win"], worst["d"], worst["c"], worst["edge"]))
    if fam == "B":                                 # both ends of the shift loop, for every loop length
        assert {M: (min(s), max(s)) for M, s in shifts.items()} == {M: (-M, M) for M in (0, 1, 7, 31)}
    if fam == "F":
        assert shifts == {31: {31}}
    if fam.startswith("A"):
        assert shifts == {31: {-7}}
        assert sum(c.expect[1][0][0] < 0 for c in SY.family(fam, mode)) == 1       # (the negative-start path is visited)
    if fam == "G":                                 # S is exactly 0 on a run of windows, the first of them N / 2 early
        assert r["s_lowest"] == 0.0 and r["s_next"] == 0.0 and r["coarse0"] == c.start - g["N"] // 2
    if fam == "C":
        labels = " ".join(c.label[0] for c in SY.family(fam, mode))
        assert set(labels.split()) == {1: set("cd"), 2: set("abcd"), 3: set("abcd"), 4: set("d")}[mode]
