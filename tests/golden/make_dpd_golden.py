#!/usr/bin/env python3
"""Writes tests/golden/dpd_reference.json: what the reference's own DPD engine (python/dpd: ExtractStatistic.py,
Model_Poly.py) makes of the pair tests/dpd_cases.py golden_pair() without its first 15 and last 16 samples -- per-bin counts, mean |rx| and mean phase, uncropped (taken
from the engine's lists and _plot_data, because its crop rule needs ES_n_per_bin samples in a bin and ES_n_per_bin is set
above the input's length here, so that its keep-the-first-128 rule drops nothing), and Model_Poly's coefficients at learning
rate 1 on the leading run of bins with min_count samples or more.  Needs a checkout of the reference; the tests read only the
JSON.

Model_Poly forms its design matrices as `sig ** i` on float32 arrays.  numpy evaluates that with whatever float32 power the
CPU dispatches to: the AVX-512 one is off by up to an ulp per entry, which moves the coefficients by some 1e-5 and differs from
machine to machine.  The golden is therefore generated with that dispatch switched off (NPY_DISABLE_CPU_FEATURES, numpy's own
run-time switch, set below before numpy is imported): the plain float32 power, which is the correctly rounded one -- the script
asserts that on the very entries Model_Poly uses.  The reference's code runs unchanged.   usage: tests/golden/make_dpd_golden.py /path/to/reference"""
import json
import os
import sys
import types

os.environ["NPY_DISABLE_CPU_FEATURES"] = "AVX512F AVX512CD AVX512_SKX AVX512_CLX AVX512_CNL AVX512_ICL AVX512_SPR"
import numpy as np      # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from tests import dpd_cases as DC      # noqa: E402
from tests import dpd_model as DM      # noqa: E402


def main(reference):
    sys.path.insert(0, os.path.join(reference, "python"))
    import matplotlib
    matplotlib.use("Agg")
    from dpd.ExtractStatistic import ExtractStatistic
    from dpd.Model_Poly import Poly

    p = dict(DC.GOLDEN)
    tx, rx = DC.golden_pair(p)
    c = types.SimpleNamespace(ES_n_bins=p["n_bins"], ES_n_per_bin=p["n"] + 1, MPM_tx_min=p["tx_min"])
    es = ExtractStatistic(c, p["peak"])
    # no sample on a bin edge: the reference's strict inequalities would drop it, this project's rule keeps it
    assert not np.isin(np.abs(tx), es.tx_boundaries.astype(np.float32)).any()
    # (the statistics use the samples whose 32 alignment taps lie inside rx: all but the first 15 and the last 16; the
    # reference is handed exactly those)
    used = slice(DM.CENTRE, p["n"] - (DM.TAPS - 1 - DM.CENTRE))
    _, _, _, n_per_bin = es.extract(np.array(tx[used]), np.array(rx[used]))
    tx_values, rx_values, phase_values, _ = es._plot_data
    counts = [int(v) for v in n_per_bin]
    # the model's bins (fp32 squared magnitude against the fp32 table of squared edges) are the reference's
    st = DM.stats(tx, rx, peak=p["peak"], n_bins=p["n_bins"])
    assert counts == [int(v) for v in st["count"]], "a sample changes its bin between the two rules: take another seed"
    run = next((i for i, v in enumerate(counts) if v < p["min_count"]), len(counts))
    f32 = lambda v: np.array(v[:run], dtype=np.float32)
    for v, powers in ((f32(rx_values), range(1, 6)), (f32(tx_values), range(0, 5))):
        for i in powers:
            assert np.array_equal(v ** i, (v.astype(np.float64) ** i).astype(np.float32)), "float32 power is not correctly rounded here"
    model = Poly(c, learning_rate_am=1.0, learning_rate_pm=1.0)
    model.train(f32(tx_values), f32(rx_values), f32(phase_values))
    _, am, pm = model.get_dpd_data()
    out = {"_about": "tests/golden/make_dpd_golden.py: the reference's ExtractStatistic and Model_Poly on dpd_cases.golden_pair()",
           "params": p, "numpy": np.__version__, "float32_power": "correctly rounded (AVX-512 dispatch off)", "counts": counts, "bins_fitted": run,
           "tx_centre": [float(v) for v in tx_values],
           "mean_rx": [None if np.isnan(v) else float(v) for v in rx_values],
           "mean_phase": [None if np.isnan(v) else float(v) for v in phase_values],
           "coefs_am": [float(v) for v in am], "coefs_pm": [float(v) for v in pm]}
    with open(os.path.join(HERE, "dpd_reference.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("bins fitted %d of %d, am %s, pm %s" % (run, len(counts), out["coefs_am"], out["coefs_pm"]))


if __name__ == "__main__":
    main(sys.argv[1])
