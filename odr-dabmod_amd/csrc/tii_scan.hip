// tii_scan.hip -- the TII analyser: whole transmission frames at the native rate -> which (comb, pattern) the null symbols
// carry, how strong each comb is and when it arrives (include/dabgpu.h, "the TII analyser").  Written from ETSI EN 300 401
// 14.8 (the carrier sets A_{c,p}, read as carrier numbers of the standard); the reference has no receiver.
// Three kernels, no host round trip between them: one workgroup per frame (the null symbol's transform in float64, cell
// energies and pair correlations), one workgroup that decides (parity, floor, masks, entries, coarse delay), and one workgroup per entry
// for the fine delay.  The frame kernel leaves the K occupied bins of every frame in memory (12 KB a frame in Mode I) for the
// third kernel: that one then needs no transform, no exchange buffer and no sample format of its own, and reads 64 bins per
// frame and entry where a second transform would read 2048 samples.  Every sum and search runs in sync.hip's fixed order
// (fixed_order.h); no floating-point atomics.
#include "device_common.h"
#include "turn_phase.h"      // ld_iq, turn_phase
#include "fixed_order.h"     // group_sum, group_arg, mul_quarter, carrier_pos, twiddle64

namespace dabgpu {
namespace {

// first carrier k(c, b, g) of cell (c, b), EN 300 401 14.8.1; its pair carrier is k + 1.  Ascending in (g, b).
template <int LOGN> DEV int tii_first(int c, int b, int g)
{
    if (LOGN == 11) return (g == 0 ? -768 : g == 1 ? -384 : g == 2 ? 1 : 385) + 2 * c + 48 * b;
    return (b < 4 ? -192 : -191) + 2 * c + 48 * b;
}
template <int LOGN> struct TiiShape {
    static constexpr int G = LOGN == 11 ? 4 : 1;                        // first carriers per cell
};

// ---- 1. per frame: R = DFT_N of the null symbol's window on the cells' carriers, in float64; E_f and G_f of the 192 cells ------
// The transform is a direct sum in float64, not Fft<LOGN>: the fp32 transform was built first, and on a clean capture its own
// rounding (1e-7 of the largest bin) is as large as the unset cells themselves -- the floor came out 0.19 ... 0.54 away from the
// float64 model's, relative, where 1e-6 is asked.  One lane per cell in Mode I (lanes 192 ... 255 only help to load), three
// cells per lane in Mode II: a lane owns all the carriers of its cells (eight or six), so E_f and G_f need no exchange.
// Samples (fp32, 8 N bytes) and the N twiddles e^{-j 2 pi m / N} (float64 sincospi of an exact argument, 16 N bytes) sit in
// LDS; every lane adds its carriers' terms in sample order, two fused multiply-adds per component, the twiddle index
// (k n) mod N kept by addition.
// rows[f]: E_f[192], Re G_f[192], Im G_f[192] as float64, cell (c, b) at 8 c + b.  bins[f]: K complexf (R rounded), carrier k
// at carrier_pos.
template <int LOGN> __global__ __launch_bounds__((1 << LOGN) / 8) void tii_frame_kernel(TiiScanArgs a)
{
    constexpr int N = 1 << LOGN, T = N / 8, K = 3 * N / 4, G = TiiShape<LOGN>::G;
    constexpr int CPL = (kTiiCells + T - 1) / T, NCAR = 2 * G * CPL;    // cells and carriers per lane: 1 and 8, or 3 and 6
    static_assert(CPL * T >= kTiiCells && (LOGN == 11 || CPL * T == kTiiCells), "every cell has its lane");
    __shared__ float2 xs[N];
    __shared__ double2 W[N];
    const int t = (int)threadIdx.x;
    const int f = (int)blockIdx.x;
    if (f >= a.n_frames) return;
    const long long tf = frame_samples(a.g);
    const long long w0 = (long long)f * tf + (long long)(a.g.null_size - a.early - N);       // 0 <= early <= null - N
#pragma unroll
    for (int m = 0; m < 8; ++m) {
        const int i = t + T * m;
        xs[i] = ld_iq(a.iq, a.fmt, w0 + i);
        W[i] = twiddle64(i, N);
    }
    lds_barrier();
    if (t >= kTiiCells) return;                                         // (Mode I's last wave; no barrier follows)

    int kk[NCAR], idx[NCAR];
    double ar[NCAR], ai[NCAR];
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
        const int i = t + T * j, c = i >> 3, b = i & 7;
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const int q = 2 * (j * G + g);
            kk[q] = tii_first<LOGN>(c, b, g);
            kk[q + 1] = kk[q] + 1;
        }
    }
#pragma unroll
    for (int q = 0; q < NCAR; ++q) { idx[q] = 0; ar[q] = 0.; ai[q] = 0.; }
    for (int n = 0; n < N; ++n) {
        const float2 x = xs[n];
        const double xr = x.x, xi = x.y;
#pragma unroll
        for (int q = 0; q < NCAR; ++q) {
            const double2 w = W[idx[q]];
            ar[q] = fma(-xi, w.y, fma(xr, w.x, ar[q]));
            ai[q] = fma(xi, w.x, fma(xr, w.y, ai[q]));
            idx[q] = (idx[q] + kk[q]) & (N - 1);
        }
    }
    float2 *out = a.bins + (size_t)f * K;
    double *row = a.rows + (size_t)f * (3 * kTiiCells);
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
        double E = 0., gr = 0., gi = 0.;
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const int q = 2 * (j * G + g), k = kk[q];
            const double x0 = ar[q], y0 = ai[q], x1 = ar[q + 1], y1 = ai[q + 1];
            out[carrier_pos<K>(k)] = mk((float)x0, (float)y0);
            out[carrier_pos<K>(k + 1)] = mk((float)x1, (float)y1);
            E += (x0 * x0 + y0 * y0) + (x1 * x1 + y1 * y1);
            double zr = x1 * x0 + y1 * y0, zi = y1 * x0 - x1 * y0;      // R[k + 1] conj(R[k])
            if (a.old_variant) {                                       // times conj(q_k) = i^(phase_q[k] - phase_q[k + 1])
                const unsigned rot = ((unsigned)a.t.phase_q[carrier_pos<K>(k)] - (unsigned)a.t.phase_q[carrier_pos<K>(k + 1)]) & 3u;
                const double r = zr, s = zi;
                switch (rot) {
                case 0: break;
                case 1: zr = -s; zi = r; break;
                case 2: zr = -r; zi = -s; break;
                default: zr = s; zi = -r; break;
                }
            }
            gr += zr;
            gi += zi;
        }
        const int i = t + T * j;
        row[i] = E;
        row[kTiiCells + i] = gr;
        row[2 * kTiiCells + i] = gi;
    }
}

// ---- 2. the decision: parity, floor, threshold, masks; the entries in comb order with energy and coarse delay; the head -------
constexpr int kDecideThreads = 256;
__global__ __launch_bounds__(kDecideThreads) void tii_decide_kernel(TiiScanArgs a)
{
    constexpr int NW = kDecideThreads / 64;
    __shared__ double red_d[NW];
    __shared__ double sE[kTiiCells], sGr[kTiiCells], sGi[kTiiCells];
    __shared__ int son[kTiiCells];
    __shared__ double sfloor;
    const int t = (int)threadIdx.x;
    const bool cell = t < kTiiCells;
    const int nf = a.n_frames;

    double e[2] = {0., 0.};
    if (cell)
        for (int f = 0; f < nf; ++f) {
            const double x = a.rows[(size_t)f * (3 * kTiiCells) + t];
            if (f & 1) e[1] += x; else e[0] += x;
        }
    const double total0 = group_sum<NW, 64>(e[0], red_d, t);
    const double total1 = group_sum<NW, 64>(e[1], red_d, t);
    const int parity = total0 >= total1 ? 0 : 1;
    const int n_used = (nf - parity + 1) / 2;
    const double E = parity ? e[1] : e[0];
    if (cell) {
        double gr = 0., gi = 0.;
        for (int f = parity; f < nf; f += 2) {
            const double *row = a.rows + (size_t)f * (3 * kTiiCells);
            gr += row[kTiiCells + t];
            gi += row[2 * kTiiCells + t];
        }
        sE[t] = E; sGr[t] = gr; sGi[t] = gi;
    }
    lds_barrier();
    // the floor by rank counting (a cell's rank: the cells smaller, or equal with a lower index), and the largest E
    double mx = 0.;
    if (cell) {
        int rank = 0;
        for (int j = 0; j < kTiiCells; ++j) {
            const double o = sE[j];
            rank += (o < E || (o == E && j < t)) ? 1 : 0;
            mx = fmax(mx, o);
        }
        if (rank == kTiiCells / 2 - 1) sfloor = E;                      // the 96th smallest: exactly one cell has this rank
    }
    lds_barrier();
    const double floor = sfloor;
    const double thr = fmax((double)a.min_ratio * floor, (double)a.min_rel * mx);
    if (cell) son[t] = (E >= thr && E > 0.) ? 1 : 0;
    lds_barrier();
    if (t < kTiiCombs) {
        int mask = 0, n_set = 0;
        double en = 0., gr = 0., gi = 0.;
        for (int b = 0; b < 8; ++b)
            if (son[8 * t + b]) {
                mask |= 0x80 >> b;
                ++n_set;
                en += sE[8 * t + b];
                gr += sGr[8 * t + b];
                gi += sGi[8 * t + b];
            }
        if (n_set) {
            int slot = 0;
            for (int c = 0; c < t; ++c) {
                int any = 0;
                for (int b = 0; b < 8; ++b) any |= son[8 * c + b];
                slot += any;
            }
            int pattern = -1;
            if (n_set == 4) {                                           // index among the words of weight four, ascending
                pattern = 0;
                for (int w = 0; w < mask; ++w) pattern += __popc((unsigned)w) == 4 ? 1 : 0;
            }
            const double tau1 = -atan2(gi, gr) * ((double)a.g.N * 0.15915494309189535);      // -arg N / 2 pi
            TiiEntry r{};
            r.comb = t;
            r.pattern = pattern;
            r.mask = mask;
            r.n_set = n_set;
            r.energy = en / (double)n_used;
            r.delay_coarse = tau1 - (double)a.early;
            a.entries[slot] = r;
            a.centre[slot] = (int)rint(tau1 * ((double)kTiiGrid / (double)a.g.N));          // rint(tau1 / s), |.| <= 8192
        }
    }
    if (t == 0) {
        int n = 0;
        for (int c = 0; c < kTiiCombs; ++c) {
            int any = 0;
            for (int b = 0; b < 8; ++b) any |= son[8 * c + b];
            n += any;
        }
        TiiScanHead h{};
        h.n_used = n_used;
        h.parity = parity;
        h.n_entries = n;
        h.floor = floor;
        h.total[0] = total0;
        h.total[1] = total1;
        *a.head = h;
    }
}

// ---- 3. fine delay, one workgroup of 256 lanes per entry: lane t owns u = centre + t - 128 on the grid of N / 16384 samples ----
constexpr int kDelayThreads = 256;
template <int LOGN> __global__ __launch_bounds__(kDelayThreads) void tii_delay_kernel(TiiScanArgs a)
{
    constexpr int N = 1 << LOGN, K = 3 * N / 4, G = TiiShape<LOGN>::G, NW = kDelayThreads / 64;
    __shared__ double red_d[NW];
    __shared__ int red_i[NW];
    const int t = (int)threadIdx.x;
    const int slot = (int)blockIdx.x;
    const TiiScanHead head = *a.head;
    if (slot >= head.n_entries) return;                                 // (its slot stays zero: the API zeroes them all)
    const int comb = a.entries[slot].comb, mask = a.entries[slot].mask, centre = a.centre[slot];
    const int u = centre + t - kDelayThreads / 2;

    double S = 0.;
    for (int f = head.parity; f < a.n_frames; f += 2) {
        const float2 *bins = a.bins + (size_t)f * K;
        cf acc = mk(0.f, 0.f);
#pragma unroll
        for (int g = 0; g < G; ++g)
            for (int b = 0; b < 8; ++b) {
                if (!(mask & (0x80 >> b))) continue;                    // (uniform over the workgroup)
                const int k0 = tii_first<LOGN>(comb, b, g);
                const unsigned q0 = a.t.phase_q[carrier_pos<K>(k0)];
                const unsigned q1 = a.old_variant ? (unsigned)a.t.phase_q[carrier_pos<K>(k0 + 1)] : q0;
                // H[k] = R[k] conj(T[k]); times e^{j 2 pi ((k u) mod 16384) / 16384}: an exact integer turn
                const cf h0 = mul_quarter(bins[carrier_pos<K>(k0)], 0u - q0);
                const cf h1 = mul_quarter(bins[carrier_pos<K>(k0 + 1)], 0u - q1);
                const unsigned long long p0 = (unsigned long long)((unsigned)(k0 * u) & (unsigned)(kTiiGrid - 1));
                const unsigned long long p1 = (unsigned long long)((unsigned)((k0 + 1) * u) & (unsigned)(kTiiGrid - 1));
                acc = cfma(acc, h0, turn_phase(p0 << 50));              // 16384 = 2^14: the turn's upper bits
                acc = cfma(acc, h1, turn_phase(p1 << 50));
            }
        S += (double)acc.x * (double)acc.x + (double)acc.y * (double)acc.y;
    }
    double best = S;
    int jstar = t;
    group_arg<true, NW, 64>(best, jstar, red_d, red_i, t);
    const int dj = t > jstar ? t - jstar : jstar - t;
    double other = dj > kTiiGrid / N ? S : -1.;
    int oi = t;
    group_arg<true, NW, 64>(other, oi, red_d, red_i, t);
    if (t == 0) {
        a.entries[slot].delay = (double)(centre + jstar - kDelayThreads / 2) * ((double)N / (double)kTiiGrid) - (double)a.early;
        a.entries[slot].runner_up = best > 0. ? other / best : 0.;
    }
}

}  // namespace

hipError_t launch_tii_scan(const TiiScanArgs &a, hipStream_t s)
{
    if ((a.g.logN != 11 && a.g.logN != 9) || a.g.K != 3 * a.g.N / 4 || (a.fmt != 0 && a.fmt != 1) || a.n_frames < 2 ||
        a.early < 0 || a.early > a.g.null_size - a.g.N || !a.iq || !a.rows || !a.bins || !a.head || !a.entries || !a.centre)
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)a.n_frames);
    return by_fft_size(a.g.logN, [&](auto L) {
        if constexpr (L == 9 || L == 11) {                              // (the sizes the check above lets through)
            DABGPU_LAUNCH_T(tii_frame_kernel, (L), grid, dim3((1 << L) / 8), 0, s, a);
            DABGPU_LAUNCH(tii_decide_kernel, dim3(1), dim3(kDecideThreads), 0, s, a);
            DABGPU_LAUNCH_T(tii_delay_kernel, (L), dim3(kTiiCombs), dim3(kDelayThreads), 0, s, a);
        }
        return hipGetLastError();
    });
}

}  // namespace dabgpu
