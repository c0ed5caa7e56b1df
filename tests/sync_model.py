"""A float64 model of the synchroniser (include/dabgpu.h, "the synchroniser"), written from the algorithm's
text, step by step, and independent of the device code: block power, coarse frame start from the null symbol, fractional
carrier offset from the cyclic prefix, integer offset and fine start from the phase reference symbol, and the extraction with
the 64-bit integer phase.  The phase reference symbol comes from the oracle's PhaseReference."""
import math

import numpy as np

from tests.receiver import MODES

RATE = 2048000.0


def geometry(mode):
    N, K, L, null, sym = MODES[mode]
    B = N // 32
    return dict(N=N, K=K, L=L, null=null, sym=sym, CP=sym - N, tf=null + L * sym, B=B, NB=null // B)


def as_complex(x):
    """complex64 samples, or int16 interleaved (re, im), as complex128."""
    x = np.asarray(x)
    if x.dtype == np.int16:
        v = x.reshape(-1, 2).astype(np.float64)
        return v[:, 0] + 1j * v[:, 1]
    return x.reshape(-1).astype(np.complex128)


def phase_reference_bins(mode):
    """P on the N bins of the transform (carrier k at bin k mod N, 0 on the unoccupied bins) and the occupied bins' mask."""
    import oracle as O
    g = geometry(mode)
    N, K = g["N"], g["K"]
    p, _ = O.phase_reference(mode)
    p = np.asarray(p, np.complex128)
    P = np.zeros(N, np.complex128)
    P[1:K // 2 + 1] = p[:K // 2]                   # positions 0 ... K/2 - 1: carriers 1 ... K/2
    P[N - K // 2:] = p[K // 2:]                    # positions K/2 ... K - 1: carriers -K/2 ... -1
    return P, P != 0


def phase_step(turns_per_sample):
    """rint(turns per sample x 2^64) as an unsigned 64-bit integer."""
    return int(np.rint(turns_per_sample * 2.0 ** 64)) % (1 << 64)


def integer_phase(n, step):
    """phi_i = 2 pi ((i step mod 2^64) >> 32) / 2^32 for i < n."""
    with np.errstate(over="ignore"):
        acc = np.arange(n, dtype=np.uint64) * np.uint64(step)
    return 2.0 * np.pi * (acc >> np.uint64(32)).astype(np.float64) / 2.0 ** 32


def _second_lowest_non_adjacent(S, b):
    far = np.ones(S.size, bool)
    far[max(b - 1, 0):b + 2] = False
    return float(S[far].min())


def _lowest_other(S, b):
    """the lowest S over every window but b, the adjacent ones included (inf where b is the only window)"""
    other = np.delete(S, b)
    return float(other.min()) if other.size else float("inf")


def sync_model(x, mode, max_shift, max_frames):
    """Steps 1 - 6 on the capture x.  -> dict: n_frames, coarse0, null_depth, frames (one dict per candidate: start, shift,
    valid, eps, cfo_hz, quality, null_depth) and margins (per candidate: d_runner_up, c_runner_up; s_second, s_next, s_lowest
    once) -- how far each integer decision was from going the other way.  s_second leaves the chosen window's neighbours out;
    s_next does not: the device adds its block powers in fp32, so the coarse decision is the model's only where the chosen
    window wins over EVERY other by far more than fp32's error."""
    g = geometry(mode)
    N, K, L, null, sym, CP, tf, B, NB = (g[k] for k in ("N", "K", "L", "null", "sym", "CP", "tf", "B", "NB"))
    x = as_complex(x)
    n = x.size
    # 1. block power
    nblk = min(n, tf + null) // B
    p = (np.abs(x[:nblk * B]) ** 2).reshape(nblk, B).sum(1)
    # 2. coarse start
    nwin = min(tf // B, nblk - NB + 1)
    S = np.lib.stride_tricks.sliding_window_view(p, NB)[:nwin].sum(1)        # (direct sums: exact zeros stay exact)
    b_star = int(np.argmin(S))
    coarse0 = b_star * B
    mean_p = float(p.mean())
    null_depth = float(S[b_star] / NB / mean_p) if mean_p > 0 else 0.0
    P, occ = phase_reference_bins(mode)
    bins = np.nonzero(occ)[0]
    pair = bins[occ[(bins + 1) % N]]                                         # bins k with k and k + 1 both occupied
    Q = np.conj(P[(pair + 1) % N] * np.conj(P[pair]))
    frames, margins = [], []
    k = 0
    while k < max_frames and coarse0 + k * tf + tf <= n:
        ck = coarse0 + k * tf
        # 3. fractional offset
        i = np.arange(2 * B, CP - 2 * B)
        a = ck + null + sym * np.arange(L)[:, None] + i[None, :]
        z = (x[a] * np.conj(x[a + N])).reshape(-1)
        gamma = complex(math.fsum(z.real), math.fsum(z.imag))                # (exactly rounded: the same on every machine)
        eps = -np.angle(gamma) / (2.0 * np.pi)
        if eps >= 0.5:
            eps -= 1.0
        # 4. integer offset
        w0 = ck + null + CP
        w = x[w0:w0 + N] * np.exp(-2j * np.pi * eps * np.arange(N) / N)
        R = np.fft.fft(w)
        ms = np.arange(-max_shift, max_shift + 1)
        D = np.array([np.sum(R[(pair + 1 + m) % N] * np.conj(R[(pair + m) % N]) * Q) for m in ms])
        D2 = np.abs(D) ** 2
        mi = int(np.argmax(D2))
        m_star = int(ms[mi])
        # 5. fine start
        C = np.zeros(N, np.complex128)
        C[bins] = R[(bins + m_star) % N] * np.conj(P[bins])
        c = N * np.fft.ifft(C)
        c2 = np.abs(c) ** 2
        l_star = int(np.argmax(c2))
        lp = l_star if l_star < N // 2 else l_star - N
        start = ck + lp
        sumC = float(np.sum(np.abs(C) ** 2))
        quality = float(c2[l_star] / (K * sumC)) if sumC > 0 else 0.0
        frames.append(dict(start=int(start), shift=m_star, valid=int(start >= 0 and start + tf <= n), eps=float(eps),
                           cfo_hz=float((m_star + eps) * RATE / N), quality=quality, null_depth=null_depth))
        far = np.ones(N, bool)
        far[[(l_star - 1) % N, l_star, (l_star + 1) % N]] = False
        margins.append(dict(d_runner_up=float(np.delete(D2, mi).max() / D2[mi]) if D2.size > 1 and D2[mi] > 0 else 0.0,
                            c_runner_up=float(c2[far].max() / c2[l_star]) if c2[l_star] > 0 else 0.0))
        k += 1
    return dict(n_frames=len(frames), coarse0=coarse0, null_depth=null_depth, frames=frames, margins=margins,
                s_lowest=float(S[b_star]), s_second=_second_lowest_non_adjacent(S, b_star), s_next=_lowest_other(S, b_star))


def extract_slots(n_samples, mode, max_frames):
    """Frames an extraction writes: min(max_frames, floor(n / tf)); those past the candidates are zeros."""
    return min(int(max_frames), int(n_samples) // geometry(mode)["tf"])


def extract_model(x, mode, frames, slots):
    """Step 7 -> (slots, tf) complex128; frames that are not valid, and slots past the candidates, are zeros."""
    g = geometry(mode)
    N, tf = g["N"], g["tf"]
    x = as_complex(x)
    out = np.zeros((slots, tf), np.complex128)
    for k, fr in enumerate(frames[:slots]):
        if not fr["valid"]:
            continue
        step = phase_step(-(fr["shift"] + fr["eps"]) / N)
        out[k] = x[fr["start"]:fr["start"] + tf] * np.exp(1j * integer_phase(tf, step))
    return out
