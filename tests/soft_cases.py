"""Inputs shared by tests/test_soft_cpu.py and tests/test_soft_gpu.py: the operating point of "soft beats hard" and seeded
soft metrics for the decoder."""
import numpy as np

from tests import decode_cases as K
from tests import decode_model as M
from tests import soft_model as S
from tests.demod_cases import NORMALISE

# The signal: Mode II, 18 transmission frames, the FIC and one 24-CU sub-channel at protection level 3-A (12 words of 64 bits
# per frame), through cfg 3 (GainControl var at 1 / 50000, FIRFilter: the window lies 44 samples early), seeded complex
# Gaussian noise on the IQ (soft_model.add_noise).  Three ETI frames come back.
OP_MODE, OP_FRAMES, OP_EARLY = 2, 18, 44
OP_SUBCHANNELS = ((0, 12, 0x22),)
OP_STEP_DB, OP_START_DB, OP_STOP_DB = 0.5, 12.0, 3.0
# Found by tests/test_soft_cpu.py's search on the numpy models (recorded in profiles/soft.txt): the highest C/N at which the hard
# path has at least one payload bit error in every returned frame, for the first noise seed at which the soft path has none at
# that level and 1 dB below.  Seeds 1 and 2 do not qualify (the soft path has 8 and 1 wrong bits 1 dB below their levels, 5.0
# and 4.5 dB); seed 3 does.
OP_SEEDS_TRIED = (1, 2, 3)
OP_SEED, OP_LEVEL_DB = 3, 5.0


def op_stream():
    """(ETI frames, the CPU front-end's coded bits, reference rows)"""
    eti, bits = K.stream(OP_FRAMES, OP_SUBCHANNELS, OP_MODE)
    return eti, bits, K.reference_rows(eti, OP_FRAMES)


def frame_errors(stats):
    """payload bit errors of every returned frame (outputs 15 ...)"""
    return [sum(u["bit_errors"] for u in stats[i]) for i in range(M.HISTORY, len(stats))]


def random_soft(shape, seed):
    """seeded int8 over the whole range, a tenth of them 0, with +127, -127 and -128 present"""
    rs = np.random.RandomState(seed)
    soft = rs.randint(-128, 128, shape).astype(np.int8)
    soft[rs.random_sample(shape) < 0.1] = 0
    flat = soft.reshape(-1)
    flat[:3] = (127, -127, -128)
    return soft


def soft_of_rows(rows, mode, fic_out, magnitude=1):
    """received rows of coded bits (decode_model.rows_of) -> the stream's softs at +-magnitude"""
    return S.soft_of_bits(K.bits_of_rows(rows, mode, fic_out), magnitude)
