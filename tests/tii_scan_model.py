"""A float64 model of the TII analyser (include/dabgpu.h, "the TII analyser"), written from the definition's
text, step by step, and independent of the device code: the null symbol's transform per frame, cell energies and pair
correlations, the parity, the floor, the decision, the coarse delay from the pair carriers and the fine delay from the search
on the 1/16384-turn grid.  The phase reference symbol comes from the oracle's PhaseReference, as in tests/sync_model.py; the
cells come from the formulas of EN 300 401 14.8.1 read as carrier numbers of the standard."""
import numpy as np

from tests.sync_model import as_complex, geometry, phase_reference_bins

GRID = 16384
COMBS, BITS = 24, 8
# the 70 patterns: the 8-bit words of weight four in ascending order, b = 0 the most significant bit
PATTERNS = [w for w in range(256) if bin(w).count("1") == 4]


def exchanged(pattern):
    """The pattern a Mode II signal configured with `pattern` reads as by the standard: bits b and b + 4 exchanged."""
    w = PATTERNS[pattern]
    return PATTERNS.index(((w & 0x0f) << 4) | (w >> 4))


def first_carriers(mode, c, b):
    """The first carriers k(c, b, g) of cell (c, b), ascending; each has its pair carrier k + 1."""
    if mode == 1:
        return [base + 2 * c + 48 * b for base in (-768, -384, 1, 385)]
    return [(-192 if b < 4 else -191) + 2 * c + 48 * b]


def cell_table(mode):
    """-> int array (24, 8, G) of first carriers."""
    return np.array([[first_carriers(mode, c, b) for b in range(BITS)] for c in range(COMBS)])


def tii_scan_model(x, mode, early, old_variant=False, min_ratio=12.0, min_rel=1e-3):
    """x: n_frames whole frames (complex64, or int16 pairs).  -> dict: the head (n_used, parity, n_entries, floor, total), the
    entries (comb, pattern, mask, n_set, energy, delay_coarse, delay, runner_up), and for the conditions of
    tests/test_tii_scan_cpu.py: thr and the cell energies E (24 x 8)."""
    g = geometry(mode)
    N, null, tf = g["N"], g["null"], g["tf"]
    x = as_complex(x).reshape(-1, tf)
    n_frames = x.shape[0]
    P, _ = phase_reference_bins(mode)
    cells = cell_table(mode)                                                 # (24, 8, G)
    w0 = null - early - N
    R = np.fft.fft(x[:, w0:w0 + N], axis=1)                                  # (n_frames, N)
    k0, k1 = cells % N, (cells + 1) % N
    q = P[k1] * np.conj(P[k0]) if old_variant else np.ones(cells.shape)
    Ef = (np.abs(R[:, k0]) ** 2 + np.abs(R[:, k1]) ** 2).sum(-1)             # (n_frames, 24, 8)
    Gf = (R[:, k1] * np.conj(R[:, k0]) * np.conj(q)).sum(-1)
    total = [float(Ef[0::2].sum()), float(Ef[1::2].sum())]
    parity = 0 if total[0] >= total[1] else 1
    used = list(range(parity, n_frames, 2))
    E, G = Ef[used].sum(0), Gf[used].sum(0)
    floor = float(np.sort(E.reshape(-1), kind="stable")[95])
    thr = max(min_ratio * floor, min_rel * float(E.max()))
    on = (E >= thr) & (E > 0)
    s = N / GRID
    entries = []
    for c in range(COMBS):
        if not on[c].any():
            continue
        bs = [b for b in range(BITS) if on[c, b]]
        mask = sum(0x80 >> b for b in bs)
        tau1 = -np.angle(G[c, bs].sum()) * N / (2.0 * np.pi)
        ks, Ts = [], []
        for b in bs:
            for k in first_carriers(mode, c, b):
                ks += [k, k + 1]
                Ts += [P[k % N], P[(k + 1) % N] if old_variant else P[k % N]]
        order = np.argsort(ks)
        ks, Ts = np.array(ks)[order], np.array(Ts)[order]
        H = R[used][:, ks % N] * np.conj(Ts)[None, :]                        # (n_used, carriers)
        u = int(np.rint(tau1 / s)) + np.arange(-128, 128)
        ph = np.exp(2j * np.pi * ((ks[:, None] * u[None, :]) % GRID) / GRID)  # (carriers, 256)
        S = (np.abs(H @ ph) ** 2).sum(0)
        js = int(np.argmax(S))
        far = np.abs(np.arange(256) - js) > GRID // N
        entries.append(dict(comb=c, pattern=PATTERNS.index(mask) if len(bs) == 4 else -1, mask=mask, n_set=len(bs),
                            energy=float(E[c, bs].sum() / len(used)), delay_coarse=float(tau1 - early),
                            delay=float(u[js] * s - early), runner_up=float(S[far].max() / S[js]) if S[js] > 0 else 0.0))
    return dict(n_used=len(used), parity=parity, n_entries=len(entries), floor=floor, total=total, entries=entries, thr=thr,
                E=E, on=on, step=s)
