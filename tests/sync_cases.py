"""The captures of the synchroniser's tests, shared by tests/test_sync_cpu.py (which checks on the oracle's chains and the
float64 model that every one of them is found, with every integer decision far from going the other way) and
tests/test_sync_gpu.py (which asserts equal integers on the device); and the swept families (FAMILIES, below) of
tests/test_sync_axes_cpu.py and tests/test_sync_axes_gpu.py, which hold the same two roles."""
import collections
import functools

import numpy as np

from tests import demod_cases as DC
from tests.sync_model import extract_model, extract_slots, geometry, sync_model

MAX_SHIFT = 31
NTAPS = 45
CFG2, CFG3 = 0, DC.GAIN | DC.FIR

# name -> (mode, stages, oracle keywords, start, cfo in carrier spacings, phase, noise_db or None, seed, s16)
# Every case met the conditions of tests/test_sync_cpu.py with the seed and offset it was first written with: none was changed.
CASES = {
    "m1_cfg2": (1, CFG2, {}, 1234, 3.37, 0.7, 20.0, 11, False),
    "m2_cfg2": (2, CFG2, {}, 1234, -7.31, -2.1, 20.0, 12, False),
    "m3_cfg2": (3, CFG2, {}, 333, 12.2, 1.3, 20.0, 13, False),
    "m4_cfg2": (4, CFG2, {}, 1234, -0.25, 3.0, 20.0, 14, False),
    "m1_cfg3": (1, CFG3, dict(gain_mode=2, normalise=DC.NORMALISE), 70001, -20.4, 0.4, None, 15, False),
    "m1_cfg3_tii": (1, CFG3, dict(gain_mode=2, normalise=DC.NORMALISE, tii=DC.TII), 70001, -20.4, 0.4, None, 16, False),
    "m2_clean": (2, CFG2, {}, 0, 0.0, 0.0, None, 17, False),
    "m1_s16": (1, CFG3, dict(gain_mode=2, normalise=1.0), 1234, 3.37, 0.7, 20.0, 18, True),
}
CFG3_CASES = ("m1_cfg3", "m1_cfg3_tii", "m1_s16")


def case_bits(mode, n_frames=2):
    """The coded bits of the case's chain: n_frames + 1 frames (the last one only lends its ends to the capture)."""
    import oracle as O
    return DC.case_bits(mode, n_frames + 1, O.tf_input_bytes(mode))


def capture_of(y, mode, start, cfo, phase, noise_db, seed, n_frames=2, s16=False, tail=None):
    """y: (n_frames + 1, tf) chain output.  -> the capture: the last `start` samples of the extra frame, n_frames frames, and
    a tail from the head of the extra frame (at least 2 B + N samples, and what the shortest capture the library takes needs);
    times exp(j (2 pi cfo i / N + phase)), plus complex Gaussian noise noise_db below the data symbols; complex64, or int16
    pairs through the oracle's FormatConverter."""
    g = geometry(mode)
    N, B, null, tf = g["N"], g["B"], g["null"], g["tf"]
    y = np.asarray(y).reshape(n_frames + 1, tf).astype(np.complex128)
    if tail is None:
        tail = max(2 * B + N, null - start)
    x = np.concatenate([y[n_frames][tf - start:], y[:n_frames].reshape(-1), y[n_frames][:tail]])
    i = np.arange(x.size, dtype=np.float64)
    x = x * np.exp(1j * (2.0 * np.pi * cfo * i / N + phase))
    if noise_db is not None:
        rs = np.random.RandomState(seed)
        p = float(np.mean(np.abs(y[:n_frames, null:]) ** 2))
        sigma = np.sqrt(p / 10.0 ** (noise_db / 10.0) / 2.0)
        x = x + sigma * (rs.randn(x.size) + 1j * rs.randn(x.size))
    x = x.astype(np.complex64)
    if s16:
        import oracle as O
        q, _ = O.format_convert(x, "s16")
        return np.asarray(q, np.int16)
    return x


def capture(mode, stages, start, cfo, phase, noise_db, seed, n_frames=2, s16=False, tail=None, **kw):
    """The oracle's chain on case_bits(mode, n_frames), as a capture (capture_of)."""
    import oracle as O
    y = O.Chain(mode=mode, stages=stages, **kw).process(case_bits(mode, n_frames))
    return capture_of(y, mode, start, cfo, phase, noise_db, seed, n_frames, s16, tail)


@functools.lru_cache(maxsize=None)
def named(name, tail=None):
    """-> (capture, mode, bits of the frames inside it, true start, cfo).  Computed once per process; do not write to it."""
    mode, stages, kw, start, cfo, phase, noise_db, seed, s16 = CASES[name]
    x = capture(mode, stages, start, cfo, phase, noise_db, seed, 2, s16, tail, **kw)
    x.setflags(write=False)
    return x, mode, case_bits(mode, 2)[:2], start, cfo


def n_samples(x):
    return x.size // 2 if x.dtype == np.int16 else x.size


# --------------------------------------------------------------------------- the swept families
# tests/test_sync_axes_cpu.py holds every capture below to the conditions under which the device's integers are asserted equal
# to the model's, and to what each family states; tests/test_sync_axes_gpu.py asserts them on the device.  All captures of a
# mode are cut from ONE chain of the oracle (cfg 2, five frames; a second one with TII for family F); seeds are fixed here.
#
# slack = null - NB B, the samples the null symbol is longer than the coarse window: 32 / 8 / 1 / 16 in Modes I - IV.  With the
# null symbol at s, the window at the block boundary b B lies wholly inside it when 0 <= b B - s <= slack.
Cap = collections.namedtuple("Cap", "label mode start cfo phase noise_db seed n_frames tail trim max_shift max_frames s16 echo "
                                    "tii gap receiver expect")
S16_SCALE = 80.0                                   # the chain's output has RMS 39.2 in Mode I, 13.9 in Mode III: 1100 ... 3100 steps
ECHO_PHASE = 1.1
FAMILY_FRAMES = 4                                  # the chain's frames, and one more that lends its ends


def slack(mode):
    g = geometry(mode)
    return g["null"] - g["NB"] * g["B"]


def _cap(label, mode, start, cfo, phase, noise_db, seed, n_frames=2, tail=None, trim=0, max_shift=MAX_SHIFT, max_frames=2,
         s16=False, echo=None, tii=False, gap=0, receiver=True, expect=None):
    if expect is None:                             # two whole frames where the capture was cut
        expect = (2, ((start, 1), (start + geometry(mode)["tf"], 1)))
    return Cap(label, mode, start, cfo, phase, noise_db, seed, n_frames, tail, trim, max_shift, max_frames, s16, echo, tii,
               gap, receiver, expect)


def _starts(mode, noise_db, seed):
    """A. start residues on the block grid: 0 ... 2 B, the last block of the search range, the middle of a frame."""
    g = geometry(mode)
    B, tf = g["B"], g["tf"]
    starts = list(range(0, 2 * B + 1, max(1, B // 16))) + [tf - B - 1, tf - B, tf - B + 1, tf - 1, tf // 2 + 1]
    # a start within the slack of the frame's end: the window at 0 lies inside the null symbol of the frame before, the first
    # candidate refines to start - tf < 0 and is not valid
    early = lambda s: ((s - tf, 0), (s, 1)) if tf - s <= slack(mode) else ((s, 1), (s + tf, 1))
    return [_cap("start %d" % s, mode, s, -7.31, 0.7, noise_db, seed + 1000 * mode + i, expect=(2, early(s)))
            for i, s in enumerate(starts)]


def _offsets(mode):
    """B. offset x search range: both ends of the shift loop for every loop length, eps up to 0.48 either side."""
    g = geometry(mode)
    out = []
    for M in (0, 1, 7, 31):
        v = [M, M - 0.3 if M else 0.3, M + 0.48, M - 0.48]
        for i, cfo in enumerate(sorted({round(s * c, 2) for c in v for s in (1, -1)})):
            out.append(_cap("max_shift %d, cfo %+.2f" % (M, cfo), mode, 3 * g["B"] + 5, cfo, 0.7, 20.0,
                            20000 + 1000 * mode + 10 * M + i, max_shift=M))
    return out


def _counts(mode):
    """C. frame count and buffer ends.  expect = (slots, ((start, valid), ...)): worked out by hand, not by the model."""
    g = geometry(mode)
    B, tf, null = g["B"], g["tf"], g["null"]
    seed = 30000 + 1000 * mode
    out = []
    if mode in (2, 3):
        s = 2 * B + 3
        for mf in (1, 2, 4, 6):                    # (a) four frames in the capture, whatever the context takes
            out.append(_cap("a: four frames, max_frames %d" % mf, mode, s, 5.3, 0.9, 20.0, seed + 1, 4, max_frames=mf,
                            expect=(min(mf, 4), tuple((s + k * tf, 1) for k in range(min(mf, 4))))))
        e = min(3, slack(mode))                    # (b) e samples into a frame: candidate 0 at -e, four valid ones follow
        for mf in (2, 6):                          # (e within the slack: in Mode III, at 3, the window at tf - B wins instead)
            cand = ((-e, 0),) + tuple((k * tf - e, 1) for k in range(1, 5))
            out.append(_cap("b: start tf - %d, max_frames %d" % (e, mf), mode, tf - e, 5.3, 0.9, 20.0, seed + 2, 4,
                            max_frames=mf, expect=(min(mf, 5), cand[:min(mf, 5)])))
    if mode in (1, 2, 3):                          # (c) n = 5 tf: five slots, four candidates
        out.append(_cap("c: five slots, four candidates", mode, B + 1, 5.3, 0.9, 20.0, seed + 3, 4, tail=tf - B - 1,
                        max_frames=6, expect=(5, tuple((B + 1 + k * tf, 1) for k in range(4)))))
    s = -(-null // B) * B + 1                      # (d) q B + 1 with q B >= null: the coarse start lies one sample before it
    out.append(_cap("d: frame 1 ends on the last sample", mode, s, 5.3, 0.9, 20.0, seed + 4, tail=0,
                    expect=(2, ((s, 1), (s + tf, 1)))))
    out.append(_cap("d: frame 1 ends one sample past the last", mode, s, 5.3, 0.9, 20.0, seed + 4, tail=0, trim=1,
                    expect=(2, ((s, 1), (s + tf, 0)))))
    out.append(_cap("d: the shortest capture, start 0", mode, 0, 5.3, 0.9, 20.0, seed + 5, tail=null,
                    expect=(2, ((0, 1), (tf, 1)))))
    if mode == 3:                                  # the shortest capture, 2 tf + null, with its frames as late as they fit
        out.append(_cap("d: the shortest capture, start 345", mode, 345, 5.3, 0.9, 20.0, seed + 6, tail=0,
                        expect=(2, ((345, 1), (345 + tf, 1)))))
        out.append(_cap("d: the shortest capture, start 346", mode, 346, 5.3, 0.9, 20.0, seed + 6, tail=0, trim=1,
                        expect=(2, ((346, 1), (346 + tf, 0)))))
    return out


def _s16(mode):
    """D. int16 samples outside Mode I, at an odd start."""
    return [_cap("s16", mode, 2 * geometry(mode)["B"] - 1, -3.4, 0.7, 20.0, 40000 + mode, s16=True)]


# E. which captures' frames the receivers behind the synchroniser are asked to decode: tests/test_sync_axes_cpu.py asserts
# that the numpy receiver does (early = CP / 2), the device test follows it.  The echo CP - 2 B behind the main path reaches
# past the receiver's window into the next symbol: nothing is claimed of it.
_ECHOES = (("echo 0.5 at CP / 2", 0.5, lambda CP, B: CP // 2, True),
           ("echo 0.5 at -CP / 2", 0.5, lambda CP, B: -(CP // 2), True),
           ("echo 0.5 at CP - 2 B", 0.5, lambda CP, B: CP - 2 * B, False),
           ("echo 0.7 at 3", 0.7, lambda CP, B: 3, True),
           ("echo 0.7 at -1", 0.7, lambda CP, B: -1, True))


def _echoes(mode):
    """E. one echo: the fine start has to pick the stronger path."""
    g = geometry(mode)
    return [_cap(label, mode, 3 * g["B"] + 5, -7.31, 0.7, 26.0, 50000 + 10 * mode + i, echo=(a, d(g["CP"], g["B"])), receiver=rx)
            for i, (label, a, d, rx) in enumerate(_ECHOES)]


def _tii(mode):
    """F. TII in the null symbol, the offset at the edge of the search range."""
    return [_cap("tii, cfo 30.6", mode, geometry(mode)["B"] + 7, 30.6, 0.4, None, 0, tii=True)]


def _dropout(mode):
    """G. the fine start exactly N / 2 off the coarse one.  No echo and no noise puts the two that far apart (the coarse start
    lies within a block of a null symbol), so the capture has a dropout: the N / 2 samples in front of the first null symbol,
    which starts on the block grid, are exact zeros in a clean capture.  Every window inside dropout and null symbol has S
    exactly 0 on the device as in the model (sums of exact zeros); the first of them starts N / 2 early, the impulse
    response peaks at index N / 2, and indices from N / 2 on count as negative: the candidates lie N before the frames (the
    first one before the buffer), which no receiver can use -- the point is the comparison, one index either side of which
    the starts differ by N."""
    g = geometry(mode)
    s = 20 * g["B"]
    return [_cap("dropout of N / 2 in front of the null symbol", mode, s, -7.31, 0.7, None, 0, gap=g["N"] // 2, receiver=False,
                 expect=(2, ((s - g["N"], 0), (s - g["N"] + g["tf"], 1))))]


# family -> (modes, captures of a mode)
FAMILIES = collections.OrderedDict([
    ("A_noise", ((1, 2, 3, 4), lambda mode: _starts(mode, 20.0, 10000))),
    ("A_clean", ((1, 2, 3, 4), lambda mode: _starts(mode, None, 0))),
    ("B", ((1, 2, 3, 4), _offsets)),
    ("C", ((1, 2, 3, 4), _counts)),
    ("D", ((2, 3, 4), _s16)),
    ("E", ((1, 2, 3, 4), _echoes)),
    ("F", ((1, 2), _tii)),
    ("G", ((1, 2, 3, 4), _dropout)),
])
FAMILY_MODES = [(f, m) for f, (modes, _) in FAMILIES.items() for m in modes]


def family(name, mode):
    return FAMILIES[name][1](mode)


@functools.lru_cache(maxsize=None)
def family_chain(mode, tii=False):
    """-> (the oracle's cfg 2 chain on case_bits(mode, 4): (5, tf) complex64, those bits).  Once per process; read only.
    (cfg 2 keeps nothing from frame to frame: the first three frames are the chain of the two-frame captures.)"""
    import oracle as O
    bits = case_bits(mode, FAMILY_FRAMES)
    y = O.Chain(mode=mode, stages=CFG2, **(dict(tii=DC.TII) if tii else {})).process(bits)
    y.setflags(write=False)
    bits.setflags(write=False)
    return y, bits


def family_capture(c):
    """The capture of a Cap: capture_of on the family's chain; s16 scaled before the conversion; an echo as
    x0 + a e^{j 1.1} roll(x0, d) on the clean capture x0, then the noise; `gap` samples in front of the first frame zeroed;
    `trim` samples cut off the end."""
    g = geometry(c.mode)
    y = family_chain(c.mode, c.tii)[0][:c.n_frames + 1].astype(np.complex128) * (S16_SCALE if c.s16 else 1.0)
    if c.echo is None:
        x = capture_of(y, c.mode, c.start, c.cfo, c.phase, c.noise_db, c.seed, c.n_frames, c.s16, c.tail)
    else:
        a, d = c.echo
        x0 = capture_of(y, c.mode, c.start, c.cfo, c.phase, None, 0, c.n_frames, False, c.tail).astype(np.complex128)
        rs = np.random.RandomState(c.seed)
        p = float(np.mean(np.abs(y[:c.n_frames, g["null"]:]) ** 2))
        sigma = np.sqrt(p / 10.0 ** (c.noise_db / 10.0) / 2.0)
        x = x0 + a * np.exp(1j * ECHO_PHASE) * np.roll(x0, d) + sigma * (rs.randn(x0.size) + 1j * rs.randn(x0.size))
        x = x.astype(np.complex64)
    if c.gap:
        x[c.start - c.gap:c.start] = 0
    if c.trim:
        x = x[:x.size - c.trim * (2 if c.s16 else 1)]
    return x


def family_model(c, x):
    """The model's verdict on the capture, with the slots an extraction writes and its extracted frames."""
    r = sync_model(x, c.mode, c.max_shift, c.max_frames)
    r["slots"] = extract_slots(n_samples(x), c.mode, c.max_frames)
    r["extracted"] = extract_model(x, c.mode, r["frames"], r["slots"])
    return r


def family_frame_bits(c, start):
    """The coded bits of the chain's frame that starts at sample `start` of the capture, or None where none does."""
    k, r = divmod(start - c.start, geometry(c.mode)["tf"])
    return family_chain(c.mode, c.tii)[1][k] if r == 0 and 0 <= k < c.n_frames else None
