"""The resampler kernels along the axis the rest of the suite holds fixed: the RUN LENGTH, the number of consecutive hops one
workgroup walks while it carries state from hop to hop (resampler16_kernel: in0 / in1 / in2 / nxt and the halo it leaves for the
next call; resampler_kernel: Fc, G, b0, the half-window shuffle of xn, the Nyquist slot by hop parity; resampler_rational_kernel
and resampler_lane_kernel: fprev in LDS).  The launchers choose it from the call size alone (resampler_runs.h), so calls of one to
four frames only ever see runs of 1 (resampler16_kernel) or 2 (the others); Modulator.set_resampler_run_hops forces it.

Input: synth_signal / 160, 50 hops or fewer per call; reference: O.Resampler on the same samples.  Two figures per call, both
logged (record_bound):
  (a) rel-RMS of every hop's slice of the output (L / M * nin / 2 samples) against the oracle, worst hop, held to the project's
      REL_RMS = 1e-6 -- the existing bar per hop instead of per call, so that one bad hop in a run cannot hide;
  (b) max |y - ref| / |ref|_inf per call, held to four times the worst value the same kernel family has at the launch geometry
      of today (hops = 0) on the same input, over its ratios and call lengths (the convention of the spectrum and DPD bars).
      The bars are never derived from a forced geometry.

THE FIRST HOP OF A STREAM is the one hop the 1e-6 of (a) cannot be asked of.  The input has no silent hop, but a stream starts from a zero
state: out_0 = first_half(Y_0) with Y_0 the interpolation of w [0 | c_0], i.e. the half of the period where the windowed input is
zero -- what the oracle has there is the interpolator's leakage, 0.002 ... 0.06 of a regular hop's RMS, and float32 reaches it
through cancellation.  Its rel-RMS is 8e-7 ... 2.9e-5 at the launch geometry of today, on every kernel, the same at every run
length (profiles/resampler_run_geometry.txt, section 1); in absolute terms it is a hop like any other, and (b) holds it; its
rel-RMS is held to a bar of its own, four times the family's worst at hops = 0 (1.78e-5, 1.66e-5, 6.96e-5, 1.14e-4).  So
every call of the run-length walk sits behind a lead-in call of two hops (the resampler's whole state) at the same forced run
length: all 50 / 49 / 1 / 2 / 3 hops of the call are regular hops and under (a), the one-hop call shifts a halo that is not
zeros, and the lead-in itself is held to (a) on its second hop, to the first-hop bar on its first, to (b) as a whole and to
the bytes of hops = 0.  The stream-state test starts on a fresh context as it must; there the stream's first hop alone goes to
the first-hop bar instead of (a).

THE GEOMETRY THAT RAN is read back after every call (Modulator.resampler_last_launch: hops per workgroup and workgroups of the
launch): the forced value and ceil(nhops / hops) workgroups, or at hops = 0 what the launchers always chose -- no kernel's bits
depend on the run length, so the bytes alone could not tell that a forced value ever reached a launch.

Measured on MI355X at hops = 0 (profiles/resampler_run_geometry.txt), worst (b) per family and the bar:
  resampler16_kernel         3.22e-7 (x4)                  bar 1.29e-6
  resampler_kernel           2.48e-7 (Mode IV, x2 and x4)  bar 9.92e-7
  resampler_rational_kernel  7.11e-7 (Mode I, 2 500 000)   bar 2.84e-6
  resampler_lane_kernel      2.15e-7 (2 047 000)           bar 8.60e-7
At the forced run lengths: every kernel gives the bytes of hops = 0 at every run length, in one call and in the pieces of a
stream, so every figure is the one of hops = 0 -- worst (a) 4.15e-7 (Mode I, 2 500 000), worst (b) 7.11e-7.  No fault found.

With DABGPU_TABLES_DIR set to a directory, a run of the WHOLE module writes resampler_run_geometry.txt there (committed under
profiles/ by that name); a partial run writes nothing."""
import os

import numpy as np
import pytest

import oracle as O
from tests.conftest import load_pkg, record_bound
from tests.golden.synth import POLY_AM, POLY_PM, synth_signal
from tests.test_gpu_parity import REL_RMS, _chain_case_bits, bits_eq, rel_rms

pytestmark = pytest.mark.gpu

R16, PACKED, RATIONAL, LANE = "resampler16_kernel", "resampler_kernel", "resampler_rational_kernel", "resampler_lane_kernel"

# (b) at hops = 0, worst over the family's ratios and the call lengths below, and the bar: four times that
PARENT_MAXABS = {R16: 3.22e-7, PACKED: 2.48e-7, RATIONAL: 7.11e-7, LANE: 2.15e-7}
MAXABS_BAR = {k: 4.0 * v for k, v in PARENT_MAXABS.items()}
# rel-RMS of the first hop of a fresh stream at hops = 0, worst over the family's ratios, and its bar: four times that
PARENT_FIRST_HOP = {R16: 4.44e-6, PACKED: 4.16e-6, RATIONAL: 1.74e-5, LANE: 2.85e-5}
FIRST_HOP_BAR = {k: 4.0 * v for k, v in PARENT_FIRST_HOP.items()}

# Every kernel gives the same bytes at every run length: resampler16_kernel treats hops as independent work items (a carried
# input register holds what a fresh load would); the rational and the lane kernel compute F_{h-1} with the same forward() in the
# run prologue and in the loop and combine it with F_h in one place; resampler_kernel forms G in its prologue as
# fmaf(sgn * factor, v, Fc) and in the loop as fmaf(sgn, Fc, fn), fn = factor * v -- which round alike because factor = 1 / nin is
# a power of two at x2 / x4 (surveyed on MI355X before it was asserted: no hop differs at any run length).
CONFIGS = [  # id, family, mode, output rate
    ("r16-x2", R16, 1, 4096000), ("r16-x4", R16, 1, 8192000),
    ("packed-II-x2", PACKED, 2, 4096000), ("packed-II-x4", PACKED, 2, 8192000),
    ("packed-III-x2", PACKED, 3, 4096000), ("packed-III-x4", PACKED, 3, 8192000),
    ("packed-IV-x2", PACKED, 4, 4096000), ("packed-IV-x4", PACKED, 4, 8192000),
    ("rational-I-3072000", RATIONAL, 1, 3072000), ("rational-I-2400000", RATIONAL, 1, 2400000),
    ("rational-I-2500000", RATIONAL, 1, 2500000), ("rational-I-1536000", RATIONAL, 1, 1536000),
    ("rational-I-1024000", RATIONAL, 1, 1024000), ("rational-II-3072000", RATIONAL, 2, 3072000),
    ("rational-III-1536000", RATIONAL, 3, 1536000),
    ("lane-I-2049000", LANE, 1, 2049000), ("lane-I-2047000", LANE, 1, 2047000),
]
NHOPS = 50
LEAD = 2         # hops of lead-in in front of every call: the resampler's whole state
RUNS_LONG = (0, 1, 2, 3, 5, 24, 96, "nhops", "nhops+7")
RUNS_SHORT = (0, 1, 2, 3, 5)
# 50: runs of 3, 24 and 96 leave a short last run and a surplus; 49: a last run of ONE hop at 2, 3 and 24; 1 ... 3: the calls
# shorter than a run, the one-hop call with its two-copy halo shift
CALLS = ((50, RUNS_LONG), (49, RUNS_LONG), (1, RUNS_SHORT), (2, RUNS_SHORT), (3, RUNS_SHORT))
PIECES = (7, 1, 0, 13, 2, NHOPS - 23)
STREAM_CONFIGS = ["r16-x4", "r16-x2", "packed-II-x4", "rational-I-2400000", "lane-I-2049000"]
N_SPACING = {1: 2048, 2: 512, 3: 256, 4: 1024}


@pytest.fixture(scope="module")
def pkg():
    return load_pkg()


# --------------------------------------------------------------------------- shared inputs and references (computed once)
_cases = {}


def _case(mode, rate):
    """(oracle geometry, input of LEAD + NHOPS hops, the oracle's output): a stream is causal, so the reference of a shorter
    call behind the same lead-in is a prefix of this one."""
    key = (mode, rate)
    if key not in _cases:
        r = O.Resampler(2048000, rate, N_SPACING[mode])
        hin = r.fft_in // 2
        x = synth_signal((LEAD + NHOPS) * hin, seed=7100 + mode) * np.float32(1 / 160)
        ref = r.process(x)
        assert ref.size == (LEAD + NHOPS) * hin * r.L // r.M
        x.setflags(write=False)
        ref.setflags(write=False)
        _cases[key] = (dict(L=r.L, M=r.M, hin=hin, hout=hin * r.L // r.M), x, ref)
    return _cases[key]


def _figures(y, ref, nhops, first=0):
    """(a) worst per-hop rel-RMS over the hops first ... and its hop, (b) max-abs over the largest reference sample"""
    d = (y.astype(np.complex128) - ref).reshape(nhops, -1)
    r = ref.astype(np.complex128).reshape(nhops, -1)
    per_hop = np.linalg.norm(d, axis=1) / np.linalg.norm(r, axis=1)
    b = float(np.abs(d).max() / np.abs(r).max())
    if first >= nhops:
        return 0.0, -1, b
    h = first + int(np.argmax(per_hop[first:]))
    return float(per_hop[h]), h, b


def _resample(pkg, md, x, geo):
    """One traced call through dabgpu_post_process_dev (the stage entry point leaves no trace)."""
    import torch
    d_in = torch.from_numpy(np.array(x, np.complex64)).cuda()          # (a copy: the shared input is read-only)
    d_out = torch.zeros(x.size // geo["hin"] * geo["hout"], dtype=torch.complex64, device="cuda")
    md.post_process_dev(d_in, pkg.STAGE_RESAMPLE, d_out)
    return d_out.cpu().numpy()


def _launch_problem(md, family, nhops, forced):
    """None, or how the geometry of the call just made differs from what `forced` (0: the launchers' own choice) asks for."""
    hops = forced or (max(1, min(24, nhops // 1536)) if family == R16 else max(2, min(96, nhops // 512)))
    want = (hops, -(-nhops // hops))
    got = md.resampler_last_launch()
    return None if got == want else "launched %s (hops per workgroup, workgroups), expected %s" % (got, want)


def _run_value(run, nhops):
    return {"nhops": nhops, "nhops+7": nhops + 7}.get(run, run)


def _differing_hops(y, y0, nhops):
    a = np.ascontiguousarray(y).view(np.uint32).reshape(nhops, -1)
    b = np.ascontiguousarray(y0).view(np.uint32).reshape(nhops, -1)
    return [int(h) for h in np.nonzero((a != b).any(axis=1))[0]]


# --------------------------------------------------------------------------- the table the tests leave behind
_parent = {}       # config id -> worst (b) at hops = 0
_start = {}        # config id -> the first hop of a fresh stream at hops = 0: (its rel-RMS, its RMS over the next hop's)
_geometry = {}     # config id -> lines
_stream = {}       # config id -> lines
_epilogue = []     # lines


@pytest.fixture(scope="module", autouse=True)
def _tables():
    yield
    d = os.environ.get("DABGPU_TABLES_DIR")
    if not d:
        return
    ids = [c[0] for c in CONFIGS]
    # (only the whole table: a run of part of this module writes nothing)
    if sorted(_geometry) != sorted(ids) or sorted(_stream) != sorted(STREAM_CONFIGS) or len(_epilogue) < 7:
        return
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "resampler_run_geometry.txt"), "w") as f:
        f.write("# tests/test_resampler_runs_gpu.py: every resampler kernel at forced run lengths (hops per workgroup,\n"
                "# Modulator.set_resampler_run_hops; 0 = the launchers' own choice) against O.Resampler on synth_signal / 160.\n"
                "# (a) = worst per-hop rel-RMS (bar 1e-6) and the hop it is at, (b) = max |y - ref| / |ref|_inf per call.\n"
                "#\n# 1. (b) at the launch geometry of today (hops = 0), worst over the lead-in and the calls of 50, 49, 1, 2, 3 hops\n"
                "# behind it; and the first hop of a fresh stream (zero start state: nearly silent) at the same geometry -- its\n"
                "# rel-RMS against the oracle and its RMS over the next hop's\n")
        fam = {}
        for cid, family, _, _ in CONFIGS:
            f.write("%-22s %-26s (b) %.3g   first hop of the stream: rel-RMS %.3g at %.3g of a regular hop's RMS\n"
                    % (cid, family, _parent[cid], _start[cid][0], _start[cid][1]))
            fam[family] = max(fam.get(family, 0.0), _parent[cid])
        f.write("#\n# 2. worst per family, and the bar the module holds (b) to (four times the value it was derived from)\n")
        for family, v in fam.items():
            f.write("%-26s measured %.3g   bar in the module %.3g\n" % (family, v, MAXABS_BAR[family]))
        f.write("#\n# 2b. the first hop of a fresh stream, worst rel-RMS per family at hops = 0, and the bar the module holds that hop to (four times it)\n")
        for family in fam:
            v = max(_start[c[0]][0] for c in CONFIGS if c[1] == family)
            f.write("%-26s measured %.3g   bar in the module %.3g\n" % (family, v, FIRST_HOP_BAR[family]))
        f.write("#\n# 3. per call length behind a lead-in of %d hops: (a), its hop and (b) at hops = 0; then every forced run length,\n"
                "# listed by itself where its bytes differ from those of hops = 0\n" % LEAD)
        for cid in ids:
            f.write("\n".join(_geometry[cid]) + "\n")
        f.write("#\n# 4. one stream in pieces of %s hops on a fresh context, per piece ((a) without the stream's first hop)\n" % (PIECES,))
        for cid in STREAM_CONFIGS:
            f.write("\n".join(_stream[cid]) + "\n")
        f.write("#\n# 5. bit identity across run lengths: asserted for all four kernels (sections 3 and 4 list every exception: none).\n"
                "# resampler_kernel forms G in its run prologue as fmaf(sgn factor, v, Fc) and in its loop as fmaf(sgn, Fc, fn) with\n"
                "# fn = factor v; at x2 / x4 factor = 1 / nin is a power of two, fn is exact, and the two round alike.\n")
        f.write("#\n# 6. the fused epilogues through the chain (GAIN | FIR | RESAMPLE | POLY)\n")
        f.write("\n".join(_epilogue) + "\n")


# --------------------------------------------------------------------------- every kernel, every run length, one call
@pytest.mark.parametrize("cid,family,mode,rate", CONFIGS, ids=[c[0] for c in CONFIGS])
def test_every_run_length_per_hop_against_the_oracle(pkg, cid, family, mode, rate):
    """One call of 50 / 49 / 1 / 2 / 3 hops at every run length, behind a lead-in call of two hops at the same run length (see
    the module docstring): the named kernel ran, (a) < 1e-6 at every hop, (b) under the family's bar, and the bytes of
    hops = 0.  The lead-in itself: its second hop under (a), the whole of it under (b), the same bytes."""
    geo, x, ref = _case(mode, rate)
    hin, hout = geo["hin"], geo["hout"]
    problems, lines = [], []
    parent_b = 0.0
    md = pkg.Modulator(mode=mode, max_frames=1)
    try:
        md.trace(True)
        for nhops, runs in CALLS:
            xin, want = x[LEAD * hin:(LEAD + nhops) * hin], ref[LEAD * hout:(LEAD + nhops) * hout]
            y0 = lead0 = None
            same_runs, figs = [], None
            for run in runs:
                hops = _run_value(run, nhops)
                md.set_resampler(2048000, rate)                    # (a fresh stream: zero halo)
                md.set_resampler_run_hops(hops)
                tag = "%s, %d hops, run %s" % (cid, nhops, run)
                lead = _resample(pkg, md, x[:LEAD * hin], geo)
                bad = _launch_problem(md, family, LEAD, hops)
                if bad:
                    problems.append("%s, lead-in: %s" % (tag, bad))
                la, _, lb = _figures(lead, ref[:LEAD * hout], LEAD, first=1)
                l0 = rel_rms(lead[:hout], ref[:hout])
                if not record_bound("resampler runs, first hop of the stream rel-RMS, %s" % tag, l0, FIRST_HOP_BAR[family]):
                    problems.append("%s: first hop of the stream rel-RMS %.3g > %.3g" % (tag, l0, FIRST_HOP_BAR[family]))
                y = _resample(pkg, md, xin, geo)
                k = md.last_variant()
                bad = _launch_problem(md, family, nhops, hops)
                if bad:
                    problems.append("%s: %s" % (tag, bad))
                if len(k) != 1 or not k[0].startswith(family + "<"):
                    problems.append("%s: kernels %s" % (tag, k))
                a, h, b = _figures(y, want, nhops)
                if run == 0:
                    y0, lead0, figs = y, lead, (a, h, b)
                    parent_b = max(parent_b, b, lb)
                    first = _figures(lead, ref[:LEAD * hout], LEAD)
                    r2 = ref[:LEAD * hout].astype(np.complex128).reshape(LEAD, -1)
                    _start[cid] = (float(np.linalg.norm((lead.astype(np.complex128) - ref[:LEAD * hout])[:hout]) / np.linalg.norm(r2[0])),
                                   float(np.linalg.norm(r2[0]) / np.linalg.norm(r2[1])))
                    assert first[2] == lb
                if not record_bound("resampler runs (a) worst hop rel-RMS, %s" % tag, max(a, la), REL_RMS):
                    problems.append("%s: hop %d rel-RMS %.3g, second hop of the lead-in %.3g" % (tag, h, a, la))
                if not record_bound("resampler runs (b) max-abs / |ref|_inf, %s" % tag, max(b, lb), MAXABS_BAR[family]):
                    problems.append("%s: max-abs %.3g (lead-in %.3g) > %.3g" % (tag, b, lb, MAXABS_BAR[family]))
                if bits_eq(y, y0) and bits_eq(lead, lead0):
                    same_runs.append(str(run))
                else:
                    dh = _differing_hops(y, y0, nhops)
                    dmax = float(np.abs(y.astype(np.complex128) - y0).max() / np.abs(want).max())
                    lines.append("%-22s call %2d run %-8s (a) %.3g at hop %2d  (b) %.3g  differs at hops %s by up to %.3g%s"
                                 % (cid, nhops, run, a, h, b, dh, dmax, "" if bits_eq(lead, lead0) else ", and in the lead-in"))
                    problems.append("%s: bytes differ from hops = 0 at hops %s%s" % (tag, dh, "" if bits_eq(lead, lead0) else ", and in the lead-in"))
            lines.append("%-22s call %2d run 0        (a) %.3g at hop %2d  (b) %.3g  same bytes at runs %s"
                         % ((cid, nhops) + figs + (", ".join(same_runs[1:]),)))
    finally:
        md.close()
    _parent[cid] = parent_b
    _geometry[cid] = lines
    assert not problems, "\n".join(problems)


# --------------------------------------------------------------------------- stream state across calls
@pytest.mark.parametrize("cid", STREAM_CONFIGS)
def test_stream_in_pieces_at_forced_run_lengths(pkg, cid):
    """The same 50 hops as pieces of 7, 1, 0, 13, 2 and 27 hops, on a fresh context at runs of 3 and of 24 (and as launched
    today): the halo a short last run leaves (resampler16_kernel's own store; the copies behind the others), the two-copy
    shift of a one-hop call and the call of nothing, inside runs longer than a one-frame call ever has.  Per piece (a) -- the
    stream's first hop under its own bar, see the module docstring -- and (b) against the oracle fed the same pieces, the
    bytes of hops = 0, and the launch geometry read back."""
    _, family, mode, rate = next(c for c in CONFIGS if c[0] == cid)
    geo, x, _ = _case(mode, rate)
    r = O.Resampler(2048000, rate, N_SPACING[mode])
    bounds = np.cumsum((0,) + PIECES)
    assert bounds[-1] == NHOPS
    refs = [r.process(x[a * geo["hin"]:b * geo["hin"]]) for a, b in zip(bounds[:-1], bounds[1:])]
    problems, lines, base = [], [], None
    for hops in (0, 3, 24):
        md = pkg.Modulator(mode=mode, max_frames=1)
        try:
            md.trace(True)
            md.set_resampler(2048000, rate)
            md.set_resampler_run_hops(hops)
            got = []
            for i, (a, b) in enumerate(zip(bounds[:-1], bounds[1:])):
                part = x[a * geo["hin"]:b * geo["hin"]]
                tag = "%s, run %d, piece %d (%d hops)" % (cid, hops, i, b - a)
                if b == a:
                    assert md.resample(part).size == 0
                    got.append(np.zeros(0, np.complex64))
                    continue
                y = _resample(pkg, md, part, geo)
                got.append(y)
                k = md.last_variant()
                if len(k) != 1 or not k[0].startswith(family + "<"):
                    problems.append("%s: kernels %s" % (tag, k))
                bad = _launch_problem(md, family, int(b - a), hops)
                if bad:
                    problems.append("%s: %s" % (tag, bad))
                fa, h, fb = _figures(y, refs[i], int(b - a), first=1 if a == 0 else 0)
                if a == 0:
                    f0 = rel_rms(y[:geo["hout"]], refs[i][:geo["hout"]])
                    if not record_bound("resampler runs, stream, first hop rel-RMS, %s" % tag, f0, FIRST_HOP_BAR[family]):
                        problems.append("%s: first hop of the stream rel-RMS %.3g > %.3g" % (tag, f0, FIRST_HOP_BAR[family]))
                same = base is None or bits_eq(y, base[i])
                if base is None or not same:
                    lines.append("%-22s run %2d piece %d (%2d hops) (a) %.3g at hop %2d  (b) %.3g%s"
                                 % (cid, hops, i, b - a, fa, h, fb, "" if same else "  differs from run 0"))
                if not record_bound("resampler runs, stream (a), %s" % tag, fa, REL_RMS):
                    problems.append("%s: hop %d rel-RMS %.3g" % (tag, h, fa))
                if not record_bound("resampler runs, stream (b), %s" % tag, fb, MAXABS_BAR[family]):
                    problems.append("%s: max-abs %.3g > %.3g" % (tag, fb, MAXABS_BAR[family]))
                if not same:
                    problems.append("%s: bytes differ from hops = 0 at hops %s" % (tag, _differing_hops(y, base[i], int(b - a))))
            if base is None:
                base = got
            else:
                lines.append("%-22s run %2d: %s" % (cid, hops, "the bytes of run 0 in every piece" if all(
                    bits_eq(g, b0) for g, b0 in zip(got, base) if g.size) else "differs"))
        finally:
            md.close()
    _stream[cid] = lines
    assert not problems, "\n".join(problems)


# --------------------------------------------------------------------------- the fused epilogues, through the chain
EPILOGUES = [("x4-poly-complexf", 8192000, True, None), ("x4-poly-s16", 8192000, True, "s16"),
             ("x4-s16", 8192000, False, "s16"), ("x2-poly-s16", 4096000, True, "s16")]


@pytest.mark.parametrize("name,rate,poly,fmt", EPILOGUES, ids=[e[0] for e in EPILOGUES])
def test_fused_epilogues_of_the_mode1_kernel_give_the_same_bytes_at_every_run_length(pkg, name, rate, poly, fmt):
    """Mode I, one frame (96 hops) through GAIN | FIR | RESAMPLE [| POLY]: MemlessPoly and the s16 store inside
    resampler16_kernel at runs of 1, 5, 24 and 96 hops -- the bytes and the clip count of hops = 0 (which the existing tests
    hold to the oracle).  normalise as in test_chain_s16_stored_by_the_resampler (0.6: |x| < 1 for the polynomial, which then
    drives components past the s16 range); without the polynomial 2.5, the file normalisation the other s16 tests clip at.  Either
    way components clip, and the count has something to count."""
    stages = pkg.STAGE_GAIN | pkg.STAGE_FIR | pkg.STAGE_RESAMPLE | (pkg.STAGE_POLY if poly else 0)
    bits = _chain_case_bits(1, 1)
    md = pkg.Modulator(mode=1, max_frames=1)
    try:
        md.trace(True)
        md.set_gain(2, 1.0, 30000.0 / 50000.0 if poly else 2.5, 4.0)
        if poly:
            md.set_poly(POLY_AM, POLY_PM)
        md.set_output_format(fmt)
        base = None
        for hops in (0, 1, 5, 24, 96):
            md.set_resampler(2048000, rate)
            md.set_resampler_run_hops(hops)
            y = md.chain(bits, stages).copy()
            clipped = md.num_clipped() if fmt else None
            k = md.last_variant()
            want = "%s<%s, %s, %d>" % (R16, "true" if poly else "false", "true" if fmt else "false", rate // 2048000)
            assert len(k) == 2 and k[0].startswith("tf_kernel<") and k[1] == want, k
            assert _launch_problem(md, R16, 96, hops) is None, (name, hops, _launch_problem(md, R16, 96, hops))
            if base is None:
                base = (y, clipped)
                assert fmt is None or clipped > 0
                _epilogue.append("%-18s %s: %s at hops = 0; runs of 1, 5, 24, 96: the same bytes and count"
                                 % (name, want, "%d clipped components" % clipped if fmt else "complexf, nothing to clip"))
                continue
            assert y.dtype == base[0].dtype and np.array_equal(y.view(np.uint8), base[0].view(np.uint8)), (name, hops)
            assert clipped == base[1], (name, hops, clipped, base[1])
    finally:
        md.close()


def test_poly_fused_into_the_packed_kernel_at_forced_run_lengths(pkg):
    """Mode II, x4 with MemlessPoly inside resampler_kernel's store, two frames (192 hops), runs of 2, 7 and 96: per-frame
    rel-RMS against O.Chain under 1e-6."""
    stages = pkg.STAGE_GAIN | pkg.STAGE_FIR | pkg.STAGE_RESAMPLE | pkg.STAGE_POLY
    bits = _chain_case_bits(2, 2)
    ref = O.Chain(mode=2, stages=15, gain_mode=2, normalise=1.0 / 50000.0, out_rate=8192000, am=POLY_AM, pm=POLY_PM).process(bits)
    md = pkg.Modulator(mode=2, max_frames=2)
    try:
        md.trace(True)
        md.set_gain(2, 1.0, 1.0 / 50000.0, 4.0)
        md.set_poly(POLY_AM, POLY_PM)
        for hops in (2, 7, 96):
            md.set_resampler(2048000, 8192000)
            md.set_resampler_run_hops(hops)
            y = md.chain(bits, stages)
            k = md.last_variant()
            assert len(k) == 2 and k[1] == "resampler_kernel<LOGNIN, 4, true>", k
            assert _launch_problem(md, PACKED, 192, hops) is None, (hops, _launch_problem(md, PACKED, 192, hops))
            worst = max(rel_rms(y[f], ref[f]) for f in range(2))
            _epilogue.append("packed-II-x4-poly     resampler_kernel<LOGNIN = 10, 4, true>, run %2d: worst frame rel-RMS %.3g" % (hops, worst))
            assert record_bound("resampler runs, Mode II x4 poly in the store, run %d, frame rel-RMS" % hops, worst, REL_RMS)
    finally:
        md.close()


# --------------------------------------------------------------------------- the setting itself
def test_run_hops_setting_refuses_negatives_resets_and_survives_set_resampler(pkg):
    """A negative value raises and leaves the setting as it was; a forced value survives set_resampler to another ratio;
    0 gives back the launchers' own choice and the bytes of a fresh context -- each seen in the geometry of the launch."""
    geo2, x, _ = _case(2, 4096000)
    geo4, _, _ = _case(2, 8192000)
    n = LEAD + NHOPS
    md = pkg.Modulator(mode=2, max_frames=1)
    try:
        assert md.resampler_last_launch() == (0, 0)                # (nothing launched yet)
        md.set_resampler(2048000, 8192000)
        want = _resample(pkg, md, x, geo4)
        assert md.resampler_last_launch() == (2, n // 2)
    finally:
        md.close()
    md = pkg.Modulator(mode=2, max_frames=1)
    try:
        md.trace(True)
        md.set_resampler(2048000, 4096000)
        md.set_resampler_run_hops(7)
        with pytest.raises(pkg.DabGpuError, match="hops per run"):
            md.set_resampler_run_hops(-1)
        _resample(pkg, md, x, geo2)
        assert md.last_variant() == ["resampler_kernel<LOGNIN, 2, false>"]
        assert md.resampler_last_launch() == (7, -(-n // 7))       # (the refused -1 changed nothing)
        md.set_resampler(2048000, 8192000)                        # another ratio, a new stream: the 7 is still there
        assert bits_eq(_resample(pkg, md, x, geo4), want)
        assert md.last_variant() == ["resampler_kernel<LOGNIN, 4, false>"]
        assert md.resampler_last_launch() == (7, -(-n // 7))
        md.set_resampler(2048000, 8192000)
        md.set_resampler_run_hops(0)
        assert bits_eq(_resample(pkg, md, x, geo4), want)
        assert md.resampler_last_launch() == (2, n // 2)
    finally:
        md.close()


DEFAULTS = [  # family, mode, rate, stages beyond GAIN | FIR | RESAMPLE, (hops per workgroup, workgroups) at 1 and at 4 frames
    (R16, 1, 8192000, True, (1, 96), (1, 384)), (R16, 1, 4096000, False, (1, 96), (1, 384)),
    (PACKED, 2, 8192000, True, (2, 48), (2, 192)), (RATIONAL, 1, 2400000, False, (2, 48), (2, 192)),
    (LANE, 1, 2049000, False, (2, 48), (2, 192)),
]


@pytest.mark.parametrize("family,mode,rate,poly,one,four", DEFAULTS, ids=["%s-%d-%d" % d[:3] for d in DEFAULTS])
def test_default_geometry_launches_the_kernels_and_grids_it_always_did(pkg, family, mode, rate, poly, one, four):
    """hops = 0, chain calls of one and of four frames (96 and 384 hops in every mode): the kernel by name, and the geometry
    the launchers had before the run length could be forced -- single hops for resampler16_kernel (96 / 384 workgroups), runs
    of two for the others (48 / 192).  The arithmetic up to 4096 frames: tests/test_resampler_runs_cpu.py, without a launch."""
    stages = pkg.STAGE_GAIN | pkg.STAGE_FIR | pkg.STAGE_RESAMPLE | (pkg.STAGE_POLY if poly else 0)
    for n, want in ((1, one), (4, four)):
        md = pkg.Modulator(mode=mode, max_frames=n)
        try:
            md.trace(True)
            md.set_gain(2, 1.0, 1.0 / 50000.0, 4.0)
            md.set_resampler(2048000, rate)
            if poly:
                md.set_poly(POLY_AM, POLY_PM)
            md.chain(_chain_case_bits(mode, n), stages)
            k = md.last_variant()
            assert k[0].startswith("tf_kernel<") and k[1].startswith(family + "<") and len(k) == 2, (n, k)
            if family == R16:
                assert k[1] == "resampler16_kernel<%s, false, %d>" % ("true" if poly else "false", rate // 2048000), k
            assert md.resampler_last_launch() == want, (n, md.resampler_last_launch(), want)
        finally:
            md.close()
