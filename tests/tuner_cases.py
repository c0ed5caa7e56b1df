"""The inputs of the tuner's tests, shared by tests/test_tuner_cpu.py (the host-only entries and the model alone) and
tests/test_tuner_gpu.py (the device against the model).  Sample counts, not frames, wherever the kernel alone is under test."""
import functools

import numpy as np

from tests.channel_cases import BAR, BLOCK, signal  # noqa: F401  (the metric, the bar and the signals are the channel's)

N_STREAM = 20000
SETTINGS = {"wide": 0, "channel": 1}

# the listed rates: rate -> (L, M)
LISTED = {2048000: (1, 1), 2304000: (8, 9), 2400000: (64, 75), 2500000: (512, 625), 2560000: (4, 5), 3072000: (2, 3),
          3200000: (16, 25), 4096000: (1, 2), 6144000: (1, 3), 8192000: (1, 4), 10000000: (128, 625), 16384000: (1, 8)}


def taps_per_output(rate, selectivity):
    L, M = LISTED[rate]
    D = 1 if L == M else -(-M // L)
    return (96 if selectivity else 32) * D


# refused settings: (in_rate, selectivity, offset_hz) -> words of the message
REFUSED = [((2000000, 0, 0.0), "must not be below 2048000"), ((2047999, 0, 0.0), "must not be below 2048000"),
           ((20000000, 0, 0.0), "M <= 8 L"), ((2048001, 0, 0.0), "L too large"),
           ((8192000, 0, 8192000 / 4.0), "must be below in_rate_hz / 4"), ((8192000, 0, -8192000 / 4.0), "must be below in_rate_hz / 4"),
           ((8192000, 2, 0.0), "selectivity is 0 (wide) or 1 (channel)"), ((8192000, -1, 0.0), "selectivity is 0 (wide) or 1 (channel)"),
           ((8192000, 0, float("nan")), "offset_hz must be finite"), ((8192000, 1, float("inf")), "offset_hz must be finite")]

# ---- the kernel against the model: the ratios 1/1, 4/5, 64/75, 512/625, 2/3, 1/4, 128/625, 1/8; both settings; two offsets
KERNEL_RATES = (2048000, 2560000, 2400000, 2500000, 3072000, 8192000, 10000000, 16384000)
KERNEL_OFFSETS = (0.0, 333333.3)
KERNEL_CASES = {"r%d_%s_off%d" % (rate, name, k): (rate, sel, off) for rate in KERNEL_RATES for name, sel in SETTINGS.items()
                for k, off in enumerate(KERNEL_OFFSETS)}

# ---- one stream, any chunking: 64/75 and 1/4 in the channel setting, with an offset, from a reset at an odd position
STREAM_CASES = {"r2400000": (2400000, 1, -123456.7), "r8192000": (8192000, 1, 333333.3)}
STREAM_POSITION = 12345
RUN_SAMPLES = (0, 7, 1 << 20)                      # chosen; many short runs; the most the span holds (the library clamps)


def splits(P, n=N_STREAM):
    """name -> the lengths of the calls"""
    sevens = [7] * (n // 7) + ([n % 7] if n % 7 else [])
    around = [P // 2 - 1, P // 2, P // 2 + 1, P - 1, P, P + 1]
    return {"whole": [n], "one_rest": [1, n - 1], "around_half_P_and_P": around + [n - sum(around)], "sevens": sevens}


# ---- positions and formats
POSITION_CASES = {"position_2_32": (2400000, 0, 333333.3, 2 ** 32 - 1000), "position_2_40": (8192000, 1, -777777.7, 2 ** 40),
                  "position_2_40_r10": (10000000, 0, 1234567.8, 2 ** 40)}
N_POSITION = 6000


def signal_u8(n, seed, signed=False):
    """n seeded samples as uint8 (or int8) pairs over the whole range"""
    rs = np.random.RandomState(seed)
    return rs.randint(0, 256, 2 * n).astype(np.uint8).view(np.int8 if signed else np.uint8)


def as_float_samples(x):
    """what the tuner makes of an input array on load: complex128"""
    x = np.asarray(x)
    if x.dtype == np.uint8:
        v = x.astype(np.float64) - 128.0
        return v[0::2] + 1j * v[1::2]
    if x.dtype in (np.int8, np.int16):
        v = x.astype(np.float64)
        return v[0::2] + 1j * v[1::2]
    return x.astype(np.complex128)


# ---- the operating points (CPU test 5, GPU test 5): Mode II, channel_cases' capture "m2_cfg2_echo40" (the end of a frame as
# lead-in, two frames, a tail), resampled to `rate`, interferers added at that rate, then tuner -> sync -> extract -> demod.
CAPTURE = "m2_cfg2_echo40"
TONE_DB = 40.0                                     # every tone's power above the resampled signal's data power
NEAR_TONES = (960.4e3, -1100.3e3)                  # inside the wide filter's transition band, outside the channel filter's
FAR_TONES = (1748.1e3, -3300.7e3)                  # outside the wide filter's pass band; they alias into the block without it
SECOND_BLOCK_HZ, SECOND_BLOCK_LATE = 1712000.0, 3000
# name -> (rates, setting, interferers)
OPERATING_POINTS = {
    "clean": ((8192000, 2400000, 3072000), 0, None),
    "near_tones": ((8192000, 2400000), 1, NEAR_TONES),
    "far_tones": ((8192000,), 0, FAR_TONES),
}
# what the model measured when the cases were written (the issue's table): starts, and the MER in dB, to 0.1 dB
EXPECTED_STARTS = [1736, 50888]
SECOND_BLOCK_STARTS = [1736 + SECOND_BLOCK_LATE // 4, 50888 + SECOND_BLOCK_LATE // 4]


def capture():
    """-> (native-rate capture input, mode, the two frames' bits, early)"""
    from tests import channel_cases as CC
    x, mode, bits, _ = CC.capture_input(CAPTURE)
    return x, mode, bits, CC.CAPTURES[CAPTURE][9]


@functools.lru_cache(maxsize=None)
def resampled(rate):
    """the capture with zeros behind it (4096 or more: behind the Resampler's delay of 512 samples and the tuner's P/2 the second
    frame is otherwise incomplete) through oracle.Resampler(2048000, rate, 512): complex64 at `rate`; do not write to it"""
    import oracle as O
    x = capture()[0]
    rs = O.Resampler(2048000, rate, 512)
    hop = rs.fft_in // 2
    n = -(-(x.size + 4096) // hop) * hop
    y = rs.process(np.concatenate([x, np.zeros(n - x.size, np.complex64)]))
    y.setflags(write=False)
    return y


def data_span(rate, mode):
    """the samples of the resampled capture that hold the first frame's data symbols: (first, last + 1)"""
    from tests.sync_model import geometry
    g = geometry(mode)
    L, M = LISTED[rate]
    return (EXPECTED_STARTS[0] + g["null"]) * M // L, (EXPECTED_STARTS[0] + g["tf"]) * M // L


def tone_amplitude(power):
    return float(np.sqrt(power * 10.0 ** (TONE_DB / 10.0)))


def tones(n, rate, freqs, amplitude):
    """the sum of the tones over samples 0 ... n - 1 at `rate`, complex128"""
    k = np.arange(n, dtype=np.float64)
    return sum(amplitude * np.exp(2j * np.pi * ((f / rate * k) % 1.0)) for f in freqs)


def with_tones(rate, freqs):
    """the resampled capture plus tones TONE_DB above its data power, complex64"""
    y = resampled(rate)
    a, b = data_span(rate, capture()[1])
    power = float(np.mean(np.abs(y[a:b].astype(np.complex128)) ** 2))
    return (y + tones(y.size, rate, freqs, tone_amplitude(power))).astype(np.complex64)


def second_block(y, rate=8192000):
    """y plus a copy of it SECOND_BLOCK_LATE samples late, at +SECOND_BLOCK_HZ and equal level.  The copy's lead-in is signal
    samples (y[1000:1000 + late], inside the capture's own lead-in), not zeros: leading zeros read as a null symbol."""
    late = SECOND_BLOCK_LATE
    copy = np.concatenate([y[1000:1000 + late], y[:y.size - late]]).astype(np.complex128)
    k = np.arange(y.size, dtype=np.float64)
    return (y + copy * np.exp(2j * np.pi * ((SECOND_BLOCK_HZ / rate * k) % 1.0))).astype(np.complex64)
