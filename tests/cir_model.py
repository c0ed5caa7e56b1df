"""A float64 model of the channel estimator (include/dabgpu.h, "the channel estimator"), written from the
definition's text, step by step, and independent of the device code: the phase reference symbol's transform per frame
(np.fft), the channel on the carriers, the weights, the impulse response, the profile over the frames, floor and peak, the
decision, the sixteen strongest paths and the derived figures.  The phase reference symbol comes from the oracle's
PhaseReference, as in tests/sync_model.py."""
import math

import numpy as np

from tests.sync_model import as_complex, geometry, phase_reference_bins

MAX_PATHS = 16


def carriers(mode):
    """The occupied carriers in ascending order: -K/2 ... -1, 1 ... K/2 (position i of the weights)."""
    K = geometry(mode)["K"]
    return np.concatenate([np.arange(-K // 2, 0), np.arange(1, K // 2 + 1)])


def weights(mode, window):
    K = geometry(mode)["K"]
    if not window:
        return np.ones(K)
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * (np.arange(K) + 0.5) / K)


def impulse_response(x, mode, early, window):
    """Steps 1 - 4 -> (h: (n_frames, N) complex128, H on the bins: (n_frames, N) complex128, 0 on the unoccupied ones)."""
    g = geometry(mode)
    N, null, CP, tf = g["N"], g["null"], g["CP"], g["tf"]
    x = as_complex(x).reshape(-1, tf)
    P, _ = phase_reference_bins(mode)
    ks = carriers(mode)
    bins = ks % N
    w0 = null + CP - early
    R = np.fft.fft(x[:, w0:w0 + N], axis=1)
    H = np.zeros_like(R)
    H[:, bins] = R[:, bins] * np.conj(P[bins])[None, :]
    w = weights(mode, window)
    sw = 0.0
    for wi in w:                                                             # S_w: in ascending carrier order
        sw += float(wi)
    Y = np.zeros_like(R)
    Y[:, bins] = H[:, bins] * w[None, :]
    h = N * np.fft.ifft(Y, axis=1) / sw                                      # sum_k w H e^{+j 2 pi k l / N} / S_w
    return h, H


def cir_model(x, mode, early, window=1, min_ratio=20.0, min_rel=1e-3):
    """x: n_frames whole frames (complex64, or int16 pairs).  -> dict: the head's fields, paths (index, delay, fine, power),
    pdp, resp, and for the conditions of tests/test_cir_cpu.py: maxima (the indices of every local maximum of the profile,
    whatever its level) and margin_db (the smallest |10 log10(pdp / threshold)| over them)."""
    g = geometry(mode)
    N, K, CP = g["N"], g["K"], g["CP"]
    h, H = impulse_response(x, mode, early, window)
    n_frames = h.shape[0]
    pdp, resp = np.zeros(N), np.zeros(N)
    for f in range(n_frames):                                                # the frames in order
        pdp += np.abs(h[f]) ** 2
        resp += np.abs(H[f]) ** 2
    pdp /= n_frames
    resp /= n_frames
    head = dict(n_frames=n_frames, n_peaks=0, n_paths=0, window=int(window), peak_index=0, resp_min_bin=0, resp_max_bin=0,
                floor=0.0, threshold=0.0, peak=0.0, total=0.0, path_power=0.0, mean_delay=0.0, delay_spread=0.0, first_delay=0.0,
                outside_guard=0.0, resp_mean=0.0, resp_min=0.0, resp_max=0.0)
    out = dict(head, paths=[], pdp=pdp, resp=resp, maxima=[], margin_db=float("inf"))
    peak = float(pdp.max())
    if not peak > 0.0:
        return out
    floor = float(np.sort(pdp, kind="stable")[N // 2 - 1])
    thr = max(float(np.float32(min_ratio)) * floor, float(np.float32(min_rel)) * peak)
    prev, nxt = np.roll(pdp, 1), np.roll(pdp, -1)
    local = (pdp > 0) & (pdp > prev) & (pdp >= nxt)
    is_peak = local & (pdp >= thr)
    order = sorted(np.nonzero(is_peak)[0], key=lambda l: (-pdp[l], l))[:MAX_PATHS]
    paths = []
    for l in order:
        a, b, c = float(prev[l]), float(pdp[l]), float(nxt[l])
        den = a - 2.0 * b + c
        paths.append(dict(index=int(l), delay=float((l if l < N // 2 else l - N) - early),
                          fine=0.0 if den == 0.0 else 0.5 * (a - c) / den, power=b))
    ks = carriers(mode)
    occ = np.sort(ks % N)                                                    # ascending bin order
    total = 0.0
    for v in pdp:
        total += float(v)
    rsum = 0.0
    for b in occ:
        rsum += float(resp[b])
    ro = resp[occ]
    out.update(n_peaks=int(is_peak.sum()), n_paths=len(paths), peak_index=int(np.argmax(pdp)), floor=floor, threshold=thr,
               peak=peak, total=total, resp_mean=rsum / K, resp_min=float(ro.min()), resp_max=float(ro.max()),
               resp_min_bin=int(occ[np.argmin(ro)]), resp_max_bin=int(occ[np.argmax(ro)]), paths=paths,
               maxima=[int(l) for l in np.nonzero(local)[0]])
    if thr > 0.0 and local.any():
        out["margin_db"] = float(np.min(np.abs(10.0 * np.log10(pdp[local] / thr))))
    if paths:
        pw = pwd = 0.0
        for p in paths:
            pw += p["power"]
            pwd += p["power"] * (p["delay"] + p["fine"])
        mean = pwd / pw
        first = min(p["delay"] for p in paths)
        var = outside = 0.0
        for p in paths:
            var += p["power"] * (p["delay"] + p["fine"] - mean) ** 2
            if p["delay"] - first > CP:
                outside += p["power"]
        out.update(path_power=pw, mean_delay=mean, delay_spread=math.sqrt(var / pw), first_delay=first, outside_guard=outside / pw)
    return out


HEAD_INTS = ("n_frames", "n_peaks", "n_paths", "window", "peak_index", "resp_min_bin", "resp_max_bin")
HEAD_REALS = ("floor", "threshold", "peak", "total", "path_power", "mean_delay", "delay_spread", "first_delay", "outside_guard",
              "resp_mean", "resp_min", "resp_max")
