// cir.hip -- the channel estimator: whole transmission frames at the native rate -> the impulse response their phase reference
// symbols went through, its echoes with level and delay, and the response on the carriers (include/dabgpu.h, "the channel
// estimator").  The reference has no receiver.
// Two kernels, no host round trip between them: one workgroup per frame (the phase reference symbol's transform in float64,
// the channel on the carriers, the weighted inverse transform), and one workgroup that decides (the profile over the frames,
// floor, peaks, the sixteen strongest paths, the derived figures).  Both transforms are radix-2 in float64 on one LDS buffer
// of N complex doubles, the twiddles float64 sincospi of an exact argument: the forward one decimates in frequency and leaves
// bin b at position bitrev(b), the inverse one decimates in time and takes them from there, so nothing is permuted.  The
// fp32 Fft<LOGN> of fft_planes.h would put its own rounding (1e-7 of the largest value) into a floor that lies at 1e-6 of the
// peak (profiles/tii_scan.txt has that story).  Every sum and search runs in sync.hip's fixed order (fixed_order.h); no
// floating-point atomics.
#include "device_common.h"
#include "turn_phase.h"      // ld_iq
#include "fixed_order.h"     // group_sum, group_arg, better, carrier_pos, bin_carrier, carrier_occupied, twiddle64

#include <climits>

namespace dabgpu {
namespace {

typedef double2 cd;
DEV cd mkd(double x, double y) { return make_double2(x, y); }
DEV cd cmuld(cd a, cd b) { return mkd(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
DEV cd mul_quarter_d(cd z, unsigned q)                                  // z i^q
{
    switch (q & 3u) {
    case 0: return z;
    case 1: return mkd(-z.y, z.x);
    case 2: return mkd(-z.x, -z.y);
    default: return mkd(z.y, -z.x);
    }
}

// ---- 1. per frame: R = DFT_N of the phase reference symbol's window, H = R conj(P), h = the weighted inverse transform --------
// N / 2 lanes, one butterfly per lane and stage; a stage reads and writes the two elements of its own pair, a barrier between
// stages.  X: the samples, then R at bit-reversed positions, then w H / S_w there, then h in natural order.  W[m] = e^{-j 2 pi
// m / N}, m < N / 2.  rows[f]: |h_f[l]|^2 for the N taps, then |H_f|^2 on the N bins (0 on the unoccupied ones).
template <int LOGN, int FMT> __global__ __launch_bounds__((1 << LOGN) / 2) void cir_frame_kernel(CirArgs a)
{
    constexpr int N = 1 << LOGN, T = N / 2, K = 3 * N / 4;
    static_assert(sizeof(cd) * (N + T) <= 64 * 1024, "buffer and twiddles within 64 KB of LDS");
    __shared__ cd X[N];
    __shared__ cd W[T];
    const int t = (int)threadIdx.x;
    const int f = (int)blockIdx.x;
    if (f >= a.n_frames) return;
    const long long tf = frame_samples(a.g);
    const long long w0 = (long long)f * tf + (long long)(a.g.null_size + a.g.sym_size - N - a.early);   // 0 <= early <= CP
#pragma unroll
    for (int m = 0; m < 2; ++m) {
        const int i = t + T * m;
        const cf x = ld_iq(a.iq, FMT, w0 + i);
        X[i] = mkd((double)x.x, (double)x.y);
    }
    W[t] = twiddle64(t, N);
    lds_barrier();
    // forward, decimation in frequency: spans N / 2 ... 1
#pragma unroll
    for (int sh = LOGN - 1; sh >= 0; --sh) {
        const int j = t & ((1 << sh) - 1), i0 = ((t >> sh) << (sh + 1)) + j, i1 = i0 + (1 << sh);
        const cd w = W[j << (LOGN - 1 - sh)];
        const cd u = X[i0], v = X[i1];
        X[i0] = mkd(u.x + v.x, u.y + v.y);
        X[i1] = cmuld(mkd(u.x - v.x, u.y - v.y), w);
        lds_barrier();
    }
    // position p holds bin bitrev(p): H = R conj(P) on the occupied carriers, |H|^2 out, w H / S_w back
    double *row = a.rows + (size_t)f * (2 * N);
#pragma unroll
    for (int m = 0; m < 2; ++m) {
        const int p = t + T * m;
        const int b = (int)(__brev((unsigned)p) >> (32 - LOGN));
        const int k = bin_carrier(b, N);
        cd y = mkd(0., 0.);
        double r2 = 0.;
        if (carrier_occupied(k, K)) {
            const unsigned q = a.t.phase_q[carrier_pos<K>(k)];
            const cd H = mul_quarter_d(X[p], 0u - q);
            r2 = H.x * H.x + H.y * H.y;
            const int i = k < 0 ? k + K / 2 : k + K / 2 - 1;            // position in ascending carrier order
            const double w = a.window ? 0.5 - 0.5 * cospi((double)(2 * i + 1) / (double)K) : 1.0;
            const double s = w / a.sum_w;
            y = mkd(H.x * s, H.y * s);
        }
        X[p] = y;
        row[N + b] = r2;
    }
    lds_barrier();
    // inverse, decimation in time: spans 1 ... N / 2, the twiddles conjugated
#pragma unroll
    for (int sh = 0; sh < LOGN; ++sh) {
        const int j = t & ((1 << sh) - 1), i0 = ((t >> sh) << (sh + 1)) + j, i1 = i0 + (1 << sh);
        const cd w = W[j << (LOGN - 1 - sh)];
        const cd u = X[i0], v = cmuld(X[i1], mkd(w.x, -w.y));
        X[i0] = mkd(u.x + v.x, u.y + v.y);
        X[i1] = mkd(u.x - v.x, u.y - v.y);
        lds_barrier();
    }
#pragma unroll
    for (int m = 0; m < 2; ++m) {
        const int l = t + T * m;
        const cd h = X[l];
        row[l] = h.x * h.x + h.y * h.y;
    }
}

// ---- 2. the decision: profile and response over the frames, floor, peak, threshold, peaks, paths, the derived figures ---------
// 1024 lanes; lane t owns taps (and bins) t and t + 1024.
constexpr int kDecideThreads = 1024;
constexpr int kMaxN = 2048;
__global__ __launch_bounds__(kDecideThreads) void cir_decide_kernel(CirArgs a)
{
    constexpr int T = kDecideThreads, NW = T / 64, E = kMaxN / T;
    __shared__ double sp[kMaxN], sr[kMaxN];
    __shared__ double red_d[NW];
    __shared__ int red_i[NW];
    __shared__ double s_floor, s_total, s_rsum;
    __shared__ int s_idx[kCirMaxPaths];
    __shared__ double s_pow[kCirMaxPaths], s_del[kCirMaxPaths], s_d[kCirMaxPaths];
    const int t = (int)threadIdx.x;
    const int N = a.g.N, K = a.g.K, nf = a.n_frames;

    // 5. profile and response: the frames in order
    double v[E], rv[E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int l = t + T * e;
        v[e] = -1.;
        rv[e] = 0.;
        if (l < N) {
            double s = 0., r = 0.;
            for (int f = 0; f < nf; ++f) {
                const double *row = a.rows + (size_t)f * (2 * (size_t)N);
                s += row[l];
                r += row[N + l];
            }
            v[e] = s / (double)nf;
            rv[e] = r / (double)nf;
            sp[l] = v[e];
            sr[l] = rv[e];
            a.pdp[l] = v[e];
            a.resp[l] = rv[e];
        }
    }
    if (t == 0) s_floor = 0.;
    lds_barrier();
    // total in index order, the response's sum in ascending bin order: one lane each
    if (t == 0) {
        double s = 0.;
        for (int l = 0; l < N; ++l) s += sp[l];
        s_total = s;
    } else if (t == 64) {
        double s = 0.;
        for (int b = 1; b <= K / 2; ++b) s += sr[b];
        for (int b = N - K / 2; b < N; ++b) s += sr[b];
        s_rsum = s;
    }
    // 6. the floor by counting: the value x with (taps below x) <= N/2 - 1 < (taps at or below x) is the one of rank N/2 - 1
    // by the definition's order, whichever of several equal taps holds that rank; and the peak
    double pk = -1.;
    int pki = INT_MAX;
    {
        int lt[E], le[E];
#pragma unroll
        for (int e = 0; e < E; ++e) lt[e] = le[e] = 0;
#pragma unroll 4
        for (int j = 0; j < N; ++j) {
            const double o = sp[j];
#pragma unroll
            for (int e = 0; e < E; ++e) {
                lt[e] += o < v[e] ? 1 : 0;
                le[e] += o <= v[e] ? 1 : 0;
            }
        }
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const int l = t + T * e;
            if (l >= N) continue;
            if (lt[e] <= N / 2 - 1 && N / 2 - 1 < le[e]) s_floor = v[e];  // (equal taps write the same value)
            if (better<true>(v[e], l, pk, pki)) { pk = v[e]; pki = l; }
        }
    }
    group_arg<true, NW, 64>(pk, pki, red_d, red_i, t);
    const double floor = s_floor, peak = pk;
    // what a reduction gives goes to the record at once (lane 0), not at the end: its sixteen partial results would stay in
    // registers until then.  The record and the path slots were zeroed before the launch; a zero input (peak = 0) leaves them
    // so but for n_frames and window.
    CirHead *h = a.head;
    const bool writer = t == 0 && peak > 0.;
    // 7. the decision
    const double thr = fmax((double)a.min_ratio * floor, (double)a.min_rel * peak);
    if (t == 0) {
        h->n_frames = nf;
        h->window = a.window;
    }
    if (writer) {
        h->peak_index = pki;
        h->floor = floor;
        h->threshold = thr;
        h->peak = peak;
        h->total = s_total;
        h->resp_mean = s_rsum / (double)K;
    }
    double cand[E];
    int cnt = 0;
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int l = t + T * e;
        cand[e] = -1.;
        if (l >= N) continue;
        const double b = v[e], pa = sp[(l - 1) & (N - 1)], pc = sp[(l + 1) & (N - 1)];
        if (b > 0. && b >= thr && b > pa && b >= pc) {
            cand[e] = b;
            ++cnt;
        }
    }
    {
        const int n_peaks = group_sum<NW, 64>(cnt, red_i, t);
        if (writer) h->n_peaks = n_peaks;
    }
    // the response's extremes over the occupied bins, the first bin of each
    {
        double rmin = 1.7976931348623157e308, rmax = -1.;               // (no bin: never an extreme, INT_MAX loses every tie)
        int rmin_i = INT_MAX, rmax_i = INT_MAX;
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const int b = t + T * e;
            if (b >= N || !carrier_occupied(bin_carrier(b, N), K)) continue;
            if (better<false>(rv[e], b, rmin, rmin_i)) { rmin = rv[e]; rmin_i = b; }
            if (better<true>(rv[e], b, rmax, rmax_i)) { rmax = rv[e]; rmax_i = b; }
        }
        group_arg<false, NW, 64>(rmin, rmin_i, red_d, red_i, t);
        if (writer) {
            h->resp_min_bin = rmin_i;
            h->resp_min = rmin;
        }
        group_arg<true, NW, 64>(rmax, rmax_i, red_d, red_i, t);
        if (writer) {
            h->resp_max_bin = rmax_i;
            h->resp_max = rmax;
        }
    }
    // 8. the strongest peaks in descending power, a lower index first among equals
    int n_paths = 0;
#pragma unroll 1
    for (int r = 0; r < kCirMaxPaths; ++r) {
        double bv = -1.;
        int bi = INT_MAX;
#pragma unroll
        for (int e = 0; e < E; ++e)
            if (cand[e] > 0. && better<true>(cand[e], t + T * e, bv, bi)) { bv = cand[e]; bi = t + T * e; }
        group_arg<true, NW, 64>(bv, bi, red_d, red_i, t);
        if (!(bv > 0.)) break;                                          // (uniform over the workgroup)
#pragma unroll
        for (int e = 0; e < E; ++e)
            if (t + T * e == bi) cand[e] = -1.;
        if (t == 0) s_idx[r] = bi;
        ++n_paths;
    }
    if (!writer) return;                                                // (no barrier follows)
    // 9. the paths' records and the derived figures, in the paths' order
    h->n_paths = n_paths;
    if (n_paths == 0) return;
    double pw = 0., pwd = 0., first = 0.;
    for (int r = 0; r < n_paths; ++r) {
        const int l = s_idx[r];
        const double pa = sp[(l - 1) & (N - 1)], b = sp[l], pc = sp[(l + 1) & (N - 1)];
        const double den = pa - 2. * b + pc;
        const double delay = (double)((l < N / 2 ? l : l - N) - a.early);
        const double fine = den == 0. ? 0. : 0.5 * (pa - pc) / den;
        CirPath *p = a.paths + r;
        p->index = l;
        p->delay = delay;
        p->fine = fine;
        p->power = b;
        s_pow[r] = b;
        s_del[r] = delay;
        s_d[r] = delay + fine;
        pw += b;
        pwd += b * (delay + fine);
        first = r == 0 ? delay : fmin(first, delay);
    }
    const double mean = pwd / pw;
    const double cp = (double)(a.g.sym_size - N);
    double var = 0., out = 0.;
    for (int r = 0; r < n_paths; ++r) {
        const double dd = s_d[r] - mean;
        var += s_pow[r] * dd * dd;
        if (s_del[r] - first > cp) out += s_pow[r];
    }
    h->path_power = pw;
    h->mean_delay = mean;
    h->delay_spread = sqrt(var / pw);
    h->first_delay = first;
    h->outside_guard = out / pw;
}

}  // namespace

hipError_t launch_cir(const CirArgs &a, hipStream_t s)
{
    if (a.g.logN < 8 || a.g.logN > 11 || a.g.N != (1 << a.g.logN) || a.g.N > kMaxN || a.g.K != 3 * a.g.N / 4 ||
        (a.fmt != 0 && a.fmt != 1) || a.n_frames < 1 || a.early < 0 || a.early > a.g.sym_size - a.g.N || a.g.sym_size < a.g.N ||
        (a.window != 0 && a.window != 1) || !(a.sum_w > 0.) || !a.iq || !a.rows || !a.head || !a.paths || !a.pdp || !a.resp ||
        !a.t.phase_q)
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)a.n_frames);
    return by_fft_size(a.g.logN, [&](auto L) {
        if (a.fmt == 0)
            DABGPU_LAUNCH_T(cir_frame_kernel, (L, 0), grid, dim3((1 << L) / 2), 0, s, a);
        else
            DABGPU_LAUNCH_T(cir_frame_kernel, (L, 1), grid, dim3((1 << L) / 2), 0, s, a);
        DABGPU_LAUNCH(cir_decide_kernel, dim3(1), dim3(kDecideThreads), 0, s, a);
        return hipGetLastError();
    });
}

}  // namespace dabgpu
