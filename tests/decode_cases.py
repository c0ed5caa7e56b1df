"""Inputs shared by tests/test_decode_cpu.py and tests/test_decode_gpu.py: layouts, streams, and the two seeded error patterns."""
import importlib

import numpy as np

from tests import decode_model as M
from tests.golden.frontend_cases import ETI_CASES
from tests.golden.synth import synth_eti

MID = {1: 1, 2: 2, 3: 3, 4: 0}
MULTI = ETI_CASES["multi"]["kw"]["subchannels"]
TWELVE = ((0, 3, 0x23), (10, 6, 0x23), (30, 12, 0x23), (60, 24, 0x22), (120, 48, 0x22), (230, 21, 1), (300, 24, 1),
          (370, 30, 1), (450, 48, 2), (560, 3, 0x21), (580, 12, 0x27), (600, 72, 0x22))
# the layout shapes of tests/test_gpu_frontend_gpu.py
SHAPES = {
    "nst0": (),
    "full_cif": ((0, 432, 0x22),),
    "twelve_with_gaps": TWELVE,
    "ends_at_864": ((768, 48, 0x22),),
    "stc_order_is_not_sad_order": ((400, 48, 0x22), (0, 24, 1), (200, 3, 0x23)),
    "overlap_last_wins": ((0, 48, 0x22), (50, 24, 0x22), (90, 3, 0x23)),
}
PADDING_AND_SMALLEST = [(21, 1), (24, 1), (30, 1), (3, 0x23)]


def cpu_front_end():
    return importlib.import_module("odr-dabmod_amd.frontend").Frontend()


def stream(n, subchannels, mode, seed=1234):
    """(ETI frames from FP = 0, the CPU front-end's coded bits)"""
    eti = synth_eti(n, subchannels=subchannels, mid=MID[mode], seed=seed)
    assert eti[0, 6] >> 5 == 0
    return eti, cpu_front_end().eti_to_bits(eti, mode)


def reference_rows(eti, n):
    """row i of a whole stream's outputs: ETI frame i - 15 (zero in the lead-in)"""
    ref = np.zeros((n, 6144), np.uint8)
    ref[M.HISTORY:] = eti[:n - M.HISTORY]
    return ref


def bits_of_rows(rows, mode, fic_out):
    """the inverse of decode_model.rows_of"""
    cifs = M.CIFS[mode]
    fic = rows[:, :fic_out].reshape(-1, cifs * fic_out)
    cif = rows[:, fic_out:].reshape(-1, cifs * M.CIF)
    return np.ascontiguousarray(np.concatenate([fic, cif], axis=1))


def sparse_flips(layout, n, seed):
    """One transmitted bit flipped per 512 transmitted bits of every (ETI frame, unit), for the FIC and the sub-channels of
    code rate 1/2 or stronger; the offset inside each block of 512 is seeded and lies in the block's middle half, so two flips
    of a unit's frame are at least 256 transmitted bits apart.  A frame's bits travel in sixteen rows: the flips are placed
    on the frame's own punctured bits and carried to the rows the time interleaver sends them to (those that would land
    behind the stream's end are dropped -- the frames they belong to are never returned).
    -> (xor mask over the received rows (n, fic_out + 6912), flips[frame][unit])"""
    us, fic_out = M.units(layout)
    rs = np.random.RandomState(seed)
    own = np.zeros((n, fic_out + M.CIF), np.uint8)                 # per frame, before the time interleaver
    count = [[0] * len(us) for _ in range(n)]
    for f in range(n):
        for ui, u in enumerate(us):
            if 16 * u["in_bytes"] > u["coded_bits"]:
                continue
            blocks = u["coded_bits"] // 512
            at = 512 * np.arange(blocks) + rs.randint(128, 384, blocks)
            cols = M.unit_rows(u, fic_out)
            np.bitwise_xor.at(own[f], cols[at >> 3], (0x80 >> (at & 7)).astype(np.uint8))
            count[f][ui] = int(blocks)
    mask = np.zeros_like(own)
    mask[:, :fic_out] = own[:, :fic_out]
    p = np.arange(M.CIF)
    for b in range(8):
        for odd in (0, 1):
            d = M.DELAY[b] + odd
            cols = fic_out + p[(p & 1) == odd]
            if d < n:
                mask[d:, cols] |= own[:n - d, cols] & np.uint8(0x80 >> b)
    return mask, count


def dense_flips(shape, seed, rate=0.04):
    """every coded bit flipped with probability `rate`, seeded: an xor mask of `shape` bytes"""
    rs = np.random.RandomState(seed)
    return np.packbits(rs.random_sample(shape + (8,)) < rate, axis=-1).reshape(shape)
