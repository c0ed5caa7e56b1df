// sync.hip -- the synchroniser in front of the receiver: a native-rate capture that starts at an arbitrary sample and sits a few
// carrier spacings off -> where its transmission frames start, their carrier frequency offset, and the frames themselves as
// dabgpu_demod* takes them.  Written from ETSI EN 300 401 (14.3: null symbol and phase reference symbol) and the textbook
// estimators: energy of the null symbol, cyclic-prefix correlation (fractional offset), differential correlation against the
// phase reference symbol (integer offset), its channel impulse response (fine start).  The reference has no receiver.
// Four kernels, no host round trip between them: block power, coarse start (one workgroup), one workgroup per candidate frame
// for everything else, and the extraction.  Every sum and every search runs in a FIXED order -- the lane's own terms, an xor
// butterfly inside the wave, the waves in wave order through LDS (demod_soft_kernel's rule) -- so a result repeats bit for bit
// and ties go to the first index.  No floating-point atomics.
#include "device_common.h"
#include "turn_phase.h"      // ld_iq, turn_phase, turn_step
#include "fixed_order.h"     // group_sum, group_arg, mul_quarter, carrier_pos, bin_carrier, carrier_occupied

namespace dabgpu {
namespace {

// ---- 1. block power: p[b] = sum of |x|^2 over the B samples of block b; one sample per lane, the butterfly over B lanes -----
template <int B> __global__ __launch_bounds__(256) void sync_power_kernel(SyncArgs a)
{
    const long long i = (long long)blockIdx.x * 256 + (long long)threadIdx.x;
    const bool in = i < (long long)a.nblk * B;                          // (whole groups of B lanes: nblk B is a multiple of B)
    float e = 0.f;
    if (in) {
        const cf x = ld_iq(a.iq, a.fmt, i);
        e = fmaf(x.x, x.x, x.y * x.y);
    }
    e = wave_sum_w<B>(e);
    if (in && ((int)threadIdx.x & (B - 1)) == 0) a.power[i / B] = e;
}

// ---- 2. coarse start: S[b] = p[b] + ... + p[b + NB - 1] (added afresh for every b: sums of exact zeros stay zero), the first b
// with the lowest S among the windows inside the buffer, the candidate count and the null depth.  One workgroup.
constexpr int kCoarseThreads = 1024;
__global__ __launch_bounds__(kCoarseThreads) void sync_coarse_kernel(SyncArgs a)
{
    constexpr int NW = kCoarseThreads / 64;
    __shared__ double red_d[NW];
    __shared__ int red_i[NW];
    const int t = (int)threadIdx.x;
    const int B = a.g.N / 32, NB = a.g.null_size / B;
    const long long tf = frame_samples(a.g);
    const int nwin = min((int)(tf / B), a.nblk - NB + 1);

    double total = 0.;
    for (int b = t; b < a.nblk; b += kCoarseThreads) total += (double)a.power[b];
    total = group_sum<NW, 64>(total, red_d, t);

    double best = __builtin_huge_val();
    int bb = 0x7fffffff;
    for (int b = t; b < nwin; b += kCoarseThreads) {
        double s = 0.;
        for (int j = 0; j < NB; ++j) s += (double)a.power[b + j];
        if (s < best) { best = s; bb = b; }
    }
    group_arg<false, NW, 64>(best, bb, red_d, red_i, t);
    if (t == 0) {
        SyncHead h{};
        if (nwin >= 1) {
            h.coarse0 = (long long)bb * B;
            int count = 0;
            while (count < a.slots && h.coarse0 + (long long)(count + 1) * tf <= a.n) ++count;
            h.count = count;
            const double mean = total / (double)a.nblk;
            h.null_depth = mean > 0. ? best / (double)NB / mean : 0.;
        }
        *a.head = h;
    }
}

// ---- 3 - 6. one workgroup of N/8 lanes per candidate frame ----------------------------------------------------------------
template <int LOGN> __global__ __launch_bounds__(Fft<LOGN>::T) void sync_frame_kernel(SyncArgs a)
{
    typedef Fft<LOGN> F;
    constexpr int N = F::N, T = F::T, K = 3 * N / 4, B = N / 32;
    constexpr int NW = (T + 63) / 64, WL = T < 64 ? T : 64;
    constexpr int MAXM = 2 * kSyncMaxShift + 1;
    constexpr int PAIRS = K - 2, PER = (PAIRS + T - 1) / T;             // carrier pairs k, k + 1 both occupied; per lane
    __shared__ cf xbuf[2 * F::LDS_ELEMS];
    __shared__ cf bins[N];
    __shared__ cf red_D[MAXM * NW];
    __shared__ float d2[MAXM];
    __shared__ double red_d[NW];
    __shared__ float red_f[NW];
    __shared__ int red_i[NW];

    const int t = (int)threadIdx.x;
    const int slot = (int)blockIdx.x;
    const SyncHead head = *a.head;
    if (slot >= head.count) return;                                     // (its record stays zero: the API zeroes them all)
    const int L = a.g.nb_symbols, null = a.g.null_size, sym = a.g.sym_size, CP = sym - N;
    const long long tf = frame_samples(a.g);
    const long long ck = head.coarse0 + (long long)slot * tf;           // ck + tf <= n: every read below lies inside the frame

    cf tw[F::NTW > 0 ? F::NTW : 1];
    F::template load_twiddles<false>(a.t.twiddle, t, tw);

    // 3. fractional offset: gamma = sum over the symbols' cyclic prefixes, 2 B samples left out on either side
    const int W = CP - 4 * B, terms = L * W;
    double gr = 0., gi = 0.;
    for (int j = t; j < terms; j += T) {
        const int s = j / W, i = j - s * W + 2 * B;
        const long long at = ck + null + (long long)s * sym + i;
        const cf x = ld_iq(a.iq, a.fmt, at), y = ld_iq(a.iq, a.fmt, at + N);
        gr += (double)x.x * (double)y.x + (double)x.y * (double)y.y;    // x conj(y)
        gi += (double)x.y * (double)y.x - (double)x.x * (double)y.y;
    }
    gr = group_sum<NW, WL>(gr, red_d, t);
    gi = group_sum<NW, WL>(gi, red_d, t);
    double eps = -atan2(gi, gr) * 0.15915494309189535;                 // -arg / 2 pi, in [-1/2, 1/2)
    if (eps >= 0.5) eps -= 1.0;

    // 4. integer offset: the phase reference symbol's window, derotated by eps, transformed; bins kept in LDS
    cf v[8];
    {
        const unsigned long long step = turn_step(-eps / (double)N);
        const long long w0 = ck + null + CP;
#pragma unroll
        for (int m = 0; m < 8; ++m) {
            const int i = t + T * m;
            v[m] = cmul(ld_iq(a.iq, a.fmt, w0 + i), turn_phase((unsigned long long)i * step));
        }
    }
    int par = 0;
    F::template run<-1, true, cf, false>(v, xbuf, par, tw, t);
#pragma unroll
    for (int m = 0; m < 8; ++m) bins[t + T * m] = v[m];
    // the lane's carrier pairs: first carrier and the quarter turns of conj(P[k + 1] conj(P[k]))
    int pk[PER];
    unsigned prot[PER];
    bool pon[PER];
#pragma unroll
    for (int c = 0; c < PER; ++c) {
        const int p = t + T * c;
        pon[c] = p < PAIRS;
        const int k = !pon[c] ? 1 : (p < K / 2 - 1 ? p + 1 : p - (K - 1));     // 1 ... K/2 - 1, then -K/2 ... -2
        pk[c] = k;
        prot[c] = ((unsigned)a.t.phase_q[carrier_pos<K>(k)] - (unsigned)a.t.phase_q[carrier_pos<K>(k + 1)]) & 3u;
    }
    lds_barrier();
    const int M = a.max_shift, nm = 2 * M + 1;
    for (int mi = 0; mi < nm; ++mi) {
        const int m = mi - M;
        cf acc = mk(0.f, 0.f);
#pragma unroll
        for (int c = 0; c < PER; ++c) {
            const int b0 = (pk[c] + m) & (N - 1);
            const cf r0 = bins[b0], r1 = bins[(b0 + 1) & (N - 1)];
            const cf z = mul_quarter(mk(fmaf(r1.x, r0.x, r1.y * r0.y), fmaf(r1.y, r0.x, -(r1.x * r0.y))), prot[c]);
            if (pon[c]) acc = cadd(acc, z);
        }
        acc.x = wave_sum_w<WL>(acc.x);
        acc.y = wave_sum_w<WL>(acc.y);
        if ((t & 63) == 0) red_D[mi * NW + (t >> 6)] = acc;
    }
    lds_barrier();
    for (int mi = t; mi < nm; mi += T) {
        cf D = red_D[mi * NW];
#pragma unroll
        for (int w = 1; w < NW; ++w) D = cadd(D, red_D[mi * NW + w]);
        d2[mi] = fmaf(D.x, D.x, D.y * D.y);
    }
    lds_barrier();
    int mstar = -M;
    {
        float bestd = d2[0];
        for (int mi = 1; mi < nm; ++mi)
            if (d2[mi] > bestd) { bestd = d2[mi]; mstar = mi - M; }
    }

    // 5. fine start: C = bins shifted by m*, times conj(P), on the occupied carriers; c = N IFFT(C); its first largest |c|^2
    float pc = 0.f;
#pragma unroll
    for (int m = 0; m < 8; ++m) {
        const int b = t + T * m;
        const int k = bin_carrier(b, N);
        const bool occ = carrier_occupied(k, K);
        const cf r = bins[(b + mstar) & (N - 1)];
        const unsigned q = a.t.phase_q[carrier_pos<K>(occ ? k : 1)];
        v[m] = occ ? mul_quarter(r, 0u - q) : mk(0.f, 0.f);
        if (occ) pc = fmaf(r.x, r.x, fmaf(r.y, r.y, pc));
    }
    pc = group_sum<NW, WL>(pc, red_f, t);
    F::template run<1, true, cf, false>(v, xbuf, par, tw, t);
    float peak = -1.f;
    int lstar = 0;
#pragma unroll
    for (int m = 0; m < 8; ++m) {
        const float c2 = fmaf(v[m].x, v[m].x, v[m].y * v[m].y);
        if (c2 > peak) { peak = c2; lstar = t + T * m; }
    }
    group_arg<true, NW, WL>(peak, lstar, red_f, red_i, t);

    // 6. the record
    if (t == 0) {
        SyncFrame f{};
        f.start = ck + (lstar < N / 2 ? lstar : lstar - N);
        f.shift = mstar;
        f.valid = (f.start >= 0 && f.start + tf <= a.n) ? 1 : 0;
        f.eps = eps;
        f.cfo_hz = ((double)mstar + eps) * 2048000.0 / (double)N;
        f.quality = pc > 0.f ? (double)peak / ((double)K * (double)pc) : 0.;
        f.null_depth = head.null_depth;
        a.frames[slot] = f;
    }
}

// ---- 7. extraction: out[k][i] = x[start_k + i] e^{j phi_i}, phi from the 64-bit integer step; zeros for what is not valid ----
template <int FMT> __global__ __launch_bounds__(256) void sync_extract_kernel(SyncArgs a, float2 *out)
{
    const long long tf = frame_samples(a.g);
    const long long i = (long long)blockIdx.x * 256 + (long long)threadIdx.x;
    const int slot = (int)blockIdx.y;
    if (i >= tf) return;
    cf y = mk(0.f, 0.f);
    if (slot < a.head->count) {
        const SyncFrame f = a.frames[slot];
        if (f.valid) {                                                  // start >= 0 and start + tf <= n
            const unsigned long long step = turn_step(-((double)f.shift + f.eps) / (double)a.g.N);
            y = cmul(ld_iq(a.iq, FMT, f.start + i), turn_phase((unsigned long long)i * step));
        }
    }
    out[(long long)slot * tf + i] = y;
}

bool sync_args_ok(const SyncArgs &a)
{
    const long long tf = frame_samples(a.g);
    const int B = a.g.N / 32;
    return (a.fmt == 0 || a.fmt == 1) && a.g.K == 3 * a.g.N / 4 && a.g.logN >= 8 && a.g.logN <= 11 && a.iq && a.head &&
           a.frames && a.slots >= 1 && a.n >= 2 * tf + a.g.null_size && a.max_shift >= 0 && a.max_shift <= kSyncMaxShift &&
           a.nblk == (int)(std::min<long long>(a.n, tf + a.g.null_size) / B);
}

}  // namespace

hipError_t launch_sync(const SyncArgs &a, hipStream_t s)
{
    if (!sync_args_ok(a) || !a.power) return hipErrorInvalidValue;
    const int B = a.g.N / 32;
    const dim3 pgrid((unsigned)(((long long)a.nblk * B + 255) / 256));
    return by_fft_size(a.g.logN, [&](auto L) {
        DABGPU_LAUNCH_T(sync_power_kernel, ((1 << L) / 32), pgrid, dim3(256), 0, s, a);
        DABGPU_LAUNCH(sync_coarse_kernel, dim3(1), dim3(kCoarseThreads), 0, s, a);
        DABGPU_LAUNCH_T(sync_frame_kernel, (L), dim3((unsigned)a.slots), dim3(Fft<L>::T), 0, s, a);
        return hipGetLastError();
    });
}

hipError_t launch_sync_extract(const SyncArgs &a, float2 *out, hipStream_t s)
{
    if (!sync_args_ok(a) || !out) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((frame_samples(a.g) + 255) / 256), (unsigned)a.slots);
    if (a.fmt == 0)
        DABGPU_LAUNCH(sync_extract_kernel<0>, grid, dim3(256), 0, s, a, out);
    else
        DABGPU_LAUNCH(sync_extract_kernel<1>, grid, dim3(256), 0, s, a, out);
    return hipGetLastError();
}

}  // namespace dabgpu
