"""Numpy models of the soft path (include/dabgpu.h: dabgpu_demod_soft*, dabgpu_decode_soft*), independent of the device code.

demod_soft_model: float64, on the steps of tests/demod_model.py (window, FFT, occupied bins, d = z_s conj(z_{s-1})): per data
symbol P = sum |d|^2, q = 64 sqrt(2) / sqrt(P / K), soft = clamp(rint(-Re d q)), clamp(rint(-Im d q)); per block the I softs in
interleaver-undone order, then the Q softs.

decode_soft_stream: integers, vectorised over the 64 states like decode_model.viterbi, under the rules that fix the bits: a
branch with expected bits e_i costs sum max(0, (1 - 2 e_i) r_i) over its four softs r_i (0 where the bit was not transmitted),
its complement sum |r_i| minus that; state 0 starts at 0, every other state at 1 << 30; tie rule and traceback of the hard
decoder."""
import numpy as np

from tests import decode_model as M
from tests.demod_model import as_complex
from tests.receiver import MODES

SIGN = 1 - 2 * np.array([[(e >> (3 - i)) & 1 for i in range(4)] for e in M.E0], np.int64)       # (64, 4): 1 - 2 e_i
MASKS = (0x6d, 0x4f, 0x53, 0x6d)


def carrier_order(mode):
    """position of the mapper's carrier n among the occupied bins in frequency order (tests/receiver.py)"""
    N, K = MODES[mode][:2]
    idx, pi = [], 0
    for _ in range(1, N):
        pi = (13 * pi + N // 4 - 1) % N
        if (N - K) // 2 <= pi <= N - (N - K) // 2 and pi != N // 2:
            idx.append(pi - (1 + N // 2) if pi > N // 2 else pi + (K - N // 2))
    return np.array(idx)


def demod_soft_model(y, mode, early=0, exact=False):
    """One frame of native-rate samples -> (nb_symbols - 1) * 2 K int8 softs (exact=True: the float64 values before rint and
    clamp, for a test that wants to know how close a value lies to a rounding boundary)."""
    y = as_complex(y)
    N, K, nsym, null, sym = MODES[mode]
    z = np.empty((nsym, K), np.complex128)
    for s in range(nsym):
        seg = y[null + s * sym: null + (s + 1) * sym]
        X = np.fft.fft(seg[sym - N - early: sym - early])
        z[s, :K // 2] = X[1:K // 2 + 1]
        z[s, K // 2:] = X[N - K // 2:]
    d = z[1:] * np.conj(z[:-1])
    P = np.sum(np.abs(d) ** 2, axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(P > 0, 64.0 * np.sqrt(2.0) / np.sqrt(P / K), 0.0)
    v = d[:, carrier_order(mode)] * q[:, None]
    x = np.concatenate([-v.real, -v.imag], axis=1).reshape(-1)
    if exact:
        return x
    return np.clip(np.rint(x), -127, 127).astype(np.int8)


def soft_of_bits(bits, magnitude=1):
    """coded bytes -> one soft per bit: +magnitude for a 1, -magnitude for a 0"""
    b = np.unpackbits(np.ascontiguousarray(bits, np.uint8), axis=-1).astype(np.int16)
    return ((2 * b - 1) * magnitude).astype(np.int8)


def soft_rows_of(soft, mode, fic_out):
    """(n_tf, 8 tf_input_bytes) softs -> (n, 8 (fic_out + 6912)) rows, one per ETI frame (decode_model.rows_of on x 8 rows)"""
    cifs = M.CIFS[mode]
    soft = np.ascontiguousarray(soft, np.int8).reshape(-1, 8 * cifs * (fic_out + M.CIF))
    fic = soft[:, :8 * cifs * fic_out].reshape(-1, 8 * fic_out)
    cif = soft[:, 8 * cifs * fic_out:].reshape(-1, 8 * M.CIF)
    return np.concatenate([fic, cif], axis=1)


def punctured_soft(rows, t, u, fic_out):
    """the unit's punctured softs of the frame whose FIC is in row t: soft 8 p + b from row t + DELAY[b] + (p & 1)"""
    n = 8 * u["out_bytes"]
    if u["dst_off"] is None:
        return rows[t, :n].copy()
    j = np.arange(n)
    delay = np.array(M.DELAY)[j & 7] + ((j >> 3) & 1)
    return rows[t + delay, 8 * (fic_out + u["dst_off"]) + j]


def depuncture_soft(pun, u):
    """(frames, 8 out_bytes) -> (frames, T, 4) int64 softs, 0 where the pattern drops the bit"""
    k = u["kept"]
    full = np.zeros((pun.shape[0], k.size), np.int64)
    full[:, k] = pun[:, :u["coded_bits"]]
    return full.reshape(pun.shape[0], -1, 4)


def viterbi_soft(r):
    """(frames, T, 4) softs -> input bits (frames, T) and the final metric of state 0 per frame"""
    F, T, _ = r.shape
    metric = np.full((F, 64), 1 << 30, np.int64)
    metric[:, 0] = 0
    other = np.empty((T, F, 64), bool)
    dots = r @ SIGN.T                                  # (F, T, 64)
    tots = np.abs(r).sum(2)                            # (F, T)
    for t in range(T):
        c0 = (tots[:, t, None] + dots[:, t]) >> 1
        a0 = metric[:, M.FROM0] + c0
        a1 = metric[:, M.FROM1] + (tots[:, t, None] - c0)
        other[t] = a1 < a0
        metric = np.where(other[t], a1, a0)
    bits = np.empty((F, T), np.uint8)
    state, f = np.zeros(F, np.int64), np.arange(F)
    for t in range(T - 1, -1, -1):
        bits[:, t] = state & 1
        state = (other[t, f, state].astype(np.int64) << 5) | (state >> 1)
    return bits, metric[:, 0].copy()


def encode(bits):
    """(frames, T) input bits (the tail's zeros included) -> (frames, T, 4) code bits of the K = 7 mother code"""
    F, T = bits.shape
    x = np.concatenate([np.zeros((F, 6), np.int64), bits.astype(np.int64)], axis=1)
    win = sum(x[:, 6 - j:6 - j + T] << j for j in range(7))          # the oldest bit at bit 6, the new one at bit 0
    par = np.array([bin(v).count("1") & 1 for v in range(128)])
    return np.stack([par[win & m] for m in MASKS], axis=2)


def decode_soft_stream(layout, soft, ref_eti=None):
    """A stream from its start, all of it in one go: (n_tf, 8 tf_input_bytes) int8 -> (images (n, 6144), stats[i][unit] =
    dict(metric, contra_sum, soft_sum, corrected, erasures, coded_bits, bit_errors, n_bits), valid (n,)).  contra_sum is formed
    from the decoded bits encoded again, independently of the trellis: it equals metric."""
    us, fic_out = M.units(layout)
    rows = soft_rows_of(soft, layout["mode"], fic_out)
    n = rows.shape[0]
    rows = np.concatenate([np.zeros((M.HISTORY, rows.shape[1]), np.int8), rows])
    images = np.zeros((n, 6144), np.uint8)
    valid = np.arange(n) >= M.HISTORY
    keys = ("metric", "contra_sum", "soft_sum", "corrected", "erasures", "coded_bits", "bit_errors", "n_bits")
    stats = [[dict.fromkeys(keys, 0) for _ in us] for _ in range(n)]
    outs = np.flatnonzero(valid)
    if outs.size == 0:
        return images, stats, valid
    seq = M.prbs(max(u["in_bytes"] for u in us))
    for ui, u in enumerate(us):
        pun = np.stack([punctured_soft(rows, t, u, fic_out) for t in outs])
        r = depuncture_soft(pun, u)
        dec, metric = viterbi_soft(r)
        payload = np.packbits(dec[:, :8 * u["in_bytes"]], axis=1) ^ seq[:u["in_bytes"]]
        images[outs, u["in_off"]:u["in_off"] + u["in_bytes"]] = payload
        sent = u["kept"].reshape(-1, 4)[None]
        mag = np.abs(r)
        contra = sent & (r != 0) & ((r > 0) != (encode(dec) == 1))
        for j, i in enumerate(outs):
            st = stats[i][ui]
            st.update(metric=int(metric[j]), contra_sum=int(mag[j][contra[j]].sum()), soft_sum=int(mag[j].sum()),
                      corrected=int(contra[j].sum()), erasures=int((sent[0] & (r[j] == 0)).sum()), coded_bits=u["coded_bits"])
            if ref_eti is not None:
                want = ref_eti[i, u["in_off"]:u["in_off"] + u["in_bytes"]]
                st["bit_errors"] = int(np.unpackbits(payload[j] ^ want).sum())
                st["n_bits"] = 8 * u["in_bytes"]
    return images, stats, valid


def add_noise(y, mode, cn_db, seed):
    """Seeded complex Gaussian noise on every sample of (frames, tf_samples) complex IQ: its power lies cn_db below the mean
    power of the frames' samples behind the null symbol.  -> complex128"""
    y = np.asarray(y, np.complex128)
    null = MODES[mode][3]
    power = float(np.mean(np.abs(y[:, null:]) ** 2))
    sigma = np.sqrt(power / 10.0 ** (cn_db / 10.0) / 2.0)
    rs = np.random.RandomState(seed)
    return y + sigma * (rs.standard_normal(y.shape) + 1j * rs.standard_normal(y.shape))
