"""The inputs of the clock's tests, shared by tests/test_clock_cpu.py (the model alone) and tests/test_clock_gpu.py (the device
against the model).  Sample counts, not frames: the resampler is under test on its own."""
from tests import clock_model as KM
from tests.channel_cases import BAR, BLOCK, signal  # noqa: F401  (the metric, the bar and the signals are the channel's)

N_STREAM = 20000

# name -> dict(ppm, lengths (of the calls; the outputs of all of them are compared), s16 (input), out, position)
KERNEL_CASES = {
    "ppm_0": dict(ppm=0.0),
    "ppm_p20": dict(ppm=20.0),
    "ppm_m20": dict(ppm=-20.0),
    "ppm_p1000": dict(ppm=1000.0),
    "ppm_m1000": dict(ppm=-1000.0),
    "ppm_1e-3": dict(ppm=1e-3),
    # a call from the reset needs 17 samples for its first output: the short calls come second as well as first
    "n1": dict(ppm=20.0, lengths=[1]),
    "n7": dict(ppm=20.0, lengths=[7]),
    "n31": dict(ppm=-1000.0, lengths=[31]),
    "n32": dict(ppm=1000.0, lengths=[32]),
    "n33": dict(ppm=20.0, lengths=[33]),
    "then_n1": dict(ppm=1000.0, lengths=[100, 1]),
    "then_n7": dict(ppm=-1000.0, lengths=[100, 7]),
    "then_n31": dict(ppm=20.0, lengths=[100, 31]),
    "then_n32": dict(ppm=-20.0, lengths=[100, 32]),
    "then_n33": dict(ppm=1000.0, lengths=[100, 33]),
    "position_2_32": dict(ppm=1000.0, lengths=[3000], position=2 ** 32 - 1000),
    "position_2_32_m": dict(ppm=-1000.0, lengths=[3000], position=2 ** 32 - 1000),
    "position_2_40": dict(ppm=1000.0, lengths=[3000], position=2 ** 40),
    "position_2_40_m": dict(ppm=-20.0, lengths=[3000], position=2 ** 40),
    "s16_input": dict(ppm=1000.0, s16=True),
    "s16_output": dict(ppm=-1000.0, s16=True, out="s16"),
}


def kernel_case(name):
    c = dict(ppm=0.0, lengths=[N_STREAM], s16=False, out="complexf", position=0)
    c.update(KERNEL_CASES[name])
    return c


# One stream, any chunking: 20 000 samples at +1000 and -1000 ppm, a slip every 1000 outputs.
STREAM_PPM = (1000.0, -1000.0)
RUN_SAMPLES = (0, 7, 2048)                         # the default; many short runs; the longest run there is


def slips(step, m_lo, m_hi):
    """the outputs m in m_lo ... m_hi - 1 at which floor(m step / 2^64) differs from that of m - 1"""
    return [m for m in range(max(m_lo, 1), m_hi) if (m * step) >> 64 != ((m - 1) * step) >> 64]


def cut_at_output(step, m):
    """the number of input samples after which output m is the first one still to come (or, where two outputs share their
    input position, the first of the two)"""
    return KM.position(m, step)[0] + 16


def splits(step, n=N_STREAM):
    """name -> the lengths of the calls"""
    sevens = [7] * (n // 7) + ([n % 7] if n % 7 else [])
    s = slips(step, 1, n - 100)
    assert len(s) >= 12
    a, b = cut_at_output(step, s[3]), cut_at_output(step, s[9])
    assert 100 < a - 1 and a + 1 < b < n
    return {"whole": [n], "one_rest": [1, n - 1], "around_16_32": [15, 16, 17, 31, 32, 33, n - 144], "sevens": sevens,
            "on_a_slip_and_beside": [a - 1, 1, 1, b - a - 1, n - b]}


# ---- the operating points of the loop (CPU test 6, GPU test 6): the inputs of tests/channel_cases.py's captures -- the end of a
# frame as lead-in, two frames, a tail, by its lead-in rule -- through the channel and then the clock at these offsets.
# name -> (capture of channel_cases, ppm, channel).  Channel "noise23": one path of gain 1 and seeded noise 23 dB below the data
# symbols; "echo": that capture's own channel (two paths, a carrier offset of 3.37 spacings, noise 20 dB below).  `early` is
# the capture's own (half the cyclic prefix in Mode II: the window drifts 4.9 samples along a frame at 100 ppm).
# Tried first: m2_p20, m2_p100, m2_m100 and m1_p20 WITHOUT a channel.  They met every condition of the CPU test (estimates
# 20.0014, 99.985, -99.981, 19.931 ppm; second pass -0.0014, 0.015, -0.019, 0.069 ppm; no bit error), but what is left after
# the correction is then sum_quadrature / sum_signal = 2e-12 ... 6e-8, set by a residual offset of a few thousandths of a ppm
# and, at the lower end, no further above fp32's own floor (2e-14, the clean chain's 137 dB) than a factor of 100: a device
# figure cannot agree with a float64 model's to 1e-3 relative there, whatever the kernels do.  With noise in front -- the level
# the offsets were first tried at in a simulation -- the figure is the noise's, which model and device share sample for sample.
# The cases were replaced, not the condition.
LOOP_CASES = {
    "m2_p20": ("m2_cfg2_echo40", 20.0, "noise23"),
    "m2_p100": ("m2_cfg2_echo40", 100.0, "noise23"),
    "m2_m100": ("m2_cfg2_echo40", -100.0, "noise23"),
    "m2_p100_echo": ("m2_cfg2_echo40", 100.0, "echo"),
    "m1_p20": ("m1_cfg3_echo300", 20.0, "noise23"),
}
LOOP_SEED = 23


def loop_case(name, channel_sigma):
    """-> (the channel's input, mode, the two frames' bits, early, ppm, (paths, sigma, seed)); channel_sigma: the package's"""
    from tests import channel_cases as CC
    cap, ppm, kind = LOOP_CASES[name]
    x, mode, bits, power = CC.capture_input(cap)
    if kind == "echo":
        channel = CC.capture_channel(cap, channel_sigma)
    else:
        channel = ([(0, 1.0 + 0.0j, 0.0)], channel_sigma(power, 23.0), LOOP_SEED)
    return x, mode, bits, CC.CAPTURES[cap][9], ppm, channel
