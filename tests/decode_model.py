"""A numpy model of the channel decoder (odr-dabmod_amd/csrc/decode.hip; include/dabgpu.h, "the channel decoder"), from the
layout dictionary of Modulator.frontend_describe: received rows -> time de-interleaver -> depuncturing -> the K = 7 Viterbi
decoder, vectorised over the 64 states (and over the frames of a call) -> energy dispersal.

The rules that fix the bits, the same as the kernel's: Hamming metrics on the transmitted bits only; state 0 starts at metric 0,
every other state at 1 << 24; state = the last six input bits, newest at bit 0; of the two predecessors of a state the one whose
oldest bit is 0 survives unless the other's metric is strictly smaller; traceback starts at state 0 behind the tail."""
import numpy as np

CIF = 6912
HISTORY = 15
CIFS = {1: 4, 2: 1, 3: 1, 4: 2}
DELAY = (0, 8, 4, 12, 2, 10, 6, 14)                # of bit 0x80 >> b of an even byte; an odd byte: one more
TAIL_PATTERN = 0xcccccc


def _parity(x):
    return bin(x).count("1") & 1


# the encoder's window of a step is (oldest bit << 6) | new state; generators 133, 171, 145, 133 (octal) mirrored
E0 = np.array([_parity(s & 0x6d) << 3 | _parity(s & 0x4f) << 2 | _parity(s & 0x53) << 1 | _parity(s & 0x6d) for s in range(64)])
POPC4 = np.array([bin(v).count("1") for v in range(16)])
FROM0 = np.arange(64) >> 1
FROM1 = 32 + (np.arange(64) >> 1)


def prbs(n):
    """x^9 + x^5 + 1 from all ones, one byte per eight steps"""
    out, acc = np.empty(n, np.uint8), 0x1ff
    for i in range(n):
        for _ in range(8):
            acc = (acc << 1) ^ _parity(acc & 0x110)
        out[i] = acc & 0xff
    return out


def units(layout):
    """the FIC, then the sub-channels in STC order: where the payload lies in the ETI frame, where the punctured bytes lie in
    a received row (None: the FIC, at its front), and which of the mother code's bits were transmitted"""
    def kept(rules):
        parts = [np.tile(np.array([(p >> (31 - b)) & 1 for b in range(32)], bool), g) for g, p in rules]
        parts.append(np.array([(TAIL_PATTERN >> (23 - b)) & 1 for b in range(24)], bool))
        return np.concatenate(parts)
    fic_out = (sum(g * bin(p).count("1") for g, p in layout["fic_rules"]) + 12 + 7) // 8
    us = [dict(in_off=layout["fic_offset"], in_bytes=layout["fic_bytes"], out_bytes=fic_out, dst_off=None,
               kept=kept(layout["fic_rules"]))]
    for s in layout["subchannels"]:
        us.append(dict(in_off=s["offset"], in_bytes=s["framesize"], out_bytes=8 * s["cu"], dst_off=8 * s["sad"], kept=kept(s["rules"])))
    for u in us:
        assert u["kept"].size == 32 * u["in_bytes"] + 24
        u["coded_bits"] = int(u["kept"].sum())
    return us, fic_out


def rows_of(bits, mode, fic_out):
    """(n_tf, tf_input_bytes) coded bits in the chain's layout -> (n, fic_out + 6912) rows, one per ETI frame"""
    cifs = CIFS[mode]
    bits = np.ascontiguousarray(bits, np.uint8).reshape(-1, cifs * (fic_out + CIF))
    fic = bits[:, :cifs * fic_out].reshape(-1, fic_out)
    cif = bits[:, cifs * fic_out:].reshape(-1, CIF)
    return np.concatenate([fic, cif], axis=1)


def unit_rows(u, fic_out):
    """the byte columns of a received row that carry transmitted bits of the unit"""
    if u["dst_off"] is None:
        return np.arange(u["out_bytes"])
    return fic_out + u["dst_off"] + np.arange(u["out_bytes"])


def punctured(rows, t, u, fic_out):
    """the unit's punctured bytes of the frame whose FIC is in row t: rows t ... t + 15 through the time interleaver"""
    if u["dst_off"] is None:
        return rows[t, :u["out_bytes"]].copy()
    at = fic_out + u["dst_off"]
    p = np.arange(u["out_bytes"])
    out = np.zeros(u["out_bytes"], np.uint8)
    for b in range(8):
        out |= rows[t + DELAY[b] + (p & 1), at + p] & np.uint8(0x80 >> b)
    return out


def depuncture(pun, u):
    """(frames, out_bytes) -> received nibbles (frames, T) and the transmitted mask (T,), one per trellis step"""
    k = u["kept"]
    bits = np.unpackbits(pun, axis=1)[:, :u["coded_bits"]]
    full = np.zeros((pun.shape[0], k.size), np.uint8)
    full[:, k] = bits
    w = np.array([8, 4, 2, 1])
    return (full.reshape(pun.shape[0], -1, 4) * w).sum(2), (k.reshape(-1, 4) * w).sum(1)


def viterbi(recv, mask):
    """-> input bits (frames, T) and the final metric of state 0 per frame"""
    F, T = recv.shape
    metric = np.full((F, 64), 1 << 24, np.int64)
    metric[:, 0] = 0
    other = np.empty((T, F, 64), bool)
    for t in range(T):
        m = int(mask[t])
        x0 = (E0[None, :] ^ recv[:, t, None]) & m
        a0 = metric[:, FROM0] + POPC4[x0]
        a1 = metric[:, FROM1] + POPC4[x0 ^ m]
        other[t] = a1 < a0
        metric = np.where(other[t], a1, a0)
    bits = np.empty((F, T), np.uint8)
    state, f = np.zeros(F, np.int64), np.arange(F)
    for t in range(T - 1, -1, -1):
        bits[:, t] = state & 1
        state = (other[t, f, state].astype(np.int64) << 5) | (state >> 1)
    return bits, metric[:, 0].copy()


def decode_stream(layout, bits, ref_eti=None):
    """A stream from its start, all of it in one go (the kernel gives the same for every call geometry): (n_tf, tf_input_bytes)
    coded bits -> (images (n, 6144), stats[i][unit] = dict(corrected, coded_bits, bit_errors, n_bits), valid (n,)).  Output i
    is ETI frame i - 15; ref_eti row i is what it should equal."""
    us, fic_out = units(layout)
    rows = rows_of(bits, layout["mode"], fic_out)
    n = rows.shape[0]
    rows = np.concatenate([np.zeros((HISTORY, rows.shape[1]), np.uint8), rows])
    images = np.zeros((n, 6144), np.uint8)
    valid = np.arange(n) >= HISTORY
    stats = [[dict(corrected=0, coded_bits=0, bit_errors=0, n_bits=0) for _ in us] for _ in range(n)]
    outs = np.flatnonzero(valid)
    if outs.size == 0:
        return images, stats, valid
    seq = prbs(max(u["in_bytes"] for u in us))
    for ui, u in enumerate(us):
        pun = np.stack([punctured(rows, t, u, fic_out) for t in outs])
        recv, mask = depuncture(pun, u)
        dec, corrected = viterbi(recv, mask)
        payload = np.packbits(dec[:, :8 * u["in_bytes"]], axis=1) ^ seq[:u["in_bytes"]]
        images[outs, u["in_off"]:u["in_off"] + u["in_bytes"]] = payload
        for j, i in enumerate(outs):
            st = stats[i][ui]
            st["corrected"], st["coded_bits"] = int(corrected[j]), u["coded_bits"]
            if ref_eti is not None:
                want = ref_eti[i, u["in_off"]:u["in_off"] + u["in_bytes"]]
                st["bit_errors"] = int(np.unpackbits(payload[j] ^ want).sum())
                st["n_bits"] = 8 * u["in_bytes"]
    return images, stats, valid


def payload_mask(layout):
    """(6144,) bool: the FIC and MST bytes of an ETI frame, what the decoder returns"""
    us, _ = units(layout)
    m = np.zeros(6144, bool)
    for u in us:
        m[u["in_off"]:u["in_off"] + u["in_bytes"]] = True
    return m
