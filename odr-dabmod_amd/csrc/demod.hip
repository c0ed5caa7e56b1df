// demod.hip -- the receiver beside the modulator: native-rate IQ of whole transmission frames -> the coded bits a chain call
// takes as input, plus per-frame quality figures.  The frame kernel's geometry backwards, walked as rx_symbols.h says (runs of
// symbols, the windows, a lane's six carriers against the previous symbol); here: hard decisions, the softs, the figures, and
// the frequency interleaver undone through Tables::src_carrier.  Written from ETSI EN 300 401 (14.5 - 14.7), like
// tests/receiver.py; the reference has no receiver.  No synchronisation and no channel estimate.
#include "device_common.h"
#include "fixed_order.h"     // wave_sum_w, twiddle64
#include "rx_symbols.h"
#include "dabgpu.h"

namespace dabgpu {
namespace {

// One workgroup = one run of data symbols (RxRun).  Carrier position k is bit n = src_carrier[k] of the block: I half then Q
// half, K/8 bytes each, MSB first.  The lanes OR their bits into one LDS image of the block; the first K/16
// lanes store it as dwords and count the bits that differ from the reference block.
//
// SOFT (dabgpu_demod_soft*): besides all of the above, one int8 metric per coded bit -- clamp(rint(-Re d q)), clamp(rint(-Im d
// q)) with q = 64 sqrt(2) / sqrt(P / K), P = the symbol's sum of |d|^2.  P is added in a FIXED order (the lane's six terms, an
// xor butterfly inside the wave, the waves in wave order through LDS), so the bytes repeat bit for bit and do not depend on
// the run geometry.  The softs go to an LDS image of the block by byte writes (soft n of the I half, K + n of the Q half: one
// writer each) and leave as 3 T dwords, three per lane, contiguous across the lanes.  The hard instantiations carry none of it.
//
// FORM_CSI (dabgpu_demod_csi*, the second pass; the first is demod_csi_state_kernel below): FORM_SOFT with every metric times
// the weight of its carrier POSITION (a.csi_w: K fp32 per frame, read once per run into six registers).
enum { FORM_HARD = 0, FORM_SOFT = 1, FORM_CSI = 2 };
template <int LOGN, int FORM> __device__ __forceinline__ void demod_body(const DemodArgs &a)
{
    constexpr bool SOFT = FORM == FORM_SOFT || FORM == FORM_CSI, CSI = FORM == FORM_CSI;
    typedef Fft<LOGN> F;
    typedef SixCarriers<LOGN> C;
    constexpr int N = F::N, T = F::T, K = 3 * N / 4, WORDS = K / 16;
    static_assert(WORDS <= T, "one lane per dword of the block");
    static_assert(2 * K == 12 * T, "three soft dwords per lane");
    constexpr int NW = (T + 63) / 64, WL = T < 64 ? T : 64;
    __shared__ cf xbuf[2 * F::LDS_ELEMS];
    __shared__ uint32_t blk[WORDS];
    __shared__ uint32_t sblk[SOFT ? 3 * T : 1];
    __shared__ float red_p[SOFT ? NW : 1];
    __shared__ double red_s[T], red_q[T];
    __shared__ float red_m[T];
    __shared__ unsigned red_e[T];

    const int t = (int)threadIdx.x;
    const int nblocks = a.g.nb_symbols - 1;
    const RxRun r = rx_run(a);
    if (r.idle) return;
    const int frame = r.frame, b0 = r.b0, b1 = r.b1;

    cf tw[F::NTW > 0 ? F::NTW : 1];
    F::template load_twiddles<false>(a.t.twiddle, t, tw);
    if (t < WORDS) blk[t] = 0u;            // (ordered in front of the first OR by the barriers of the first transform)

    // the lane's six carriers: where the carrier's two bits go in the LDS image (word, bit inside the word)
    int iword[6], qword[6], nsoft[SOFT ? 6 : 1];
    unsigned shift[6];
    int kpos[CSI ? 6 : 1];
#pragma unroll
    for (int c = 0; c < 6; ++c) {
        const int k = C::position(c, t);
        const int n = a.t.src_carrier[k];
        const int ib = n >> 3, qb = ib + K / 8;
        iword[c] = ib >> 2;
        qword[c] = qb >> 2;
        // (K/8 is a multiple of four bytes in every mode: the byte's place inside its word is the same in both halves)
        shift[c] = 8u * ((unsigned)ib & 3u) + (7u - ((unsigned)n & 7u));
        if constexpr (SOFT) nsoft[c] = n;
        if constexpr (CSI) kpos[c] = k;
    }
    float wgt[CSI ? 6 : 1];
    if constexpr (CSI) {
#pragma unroll
        for (int c = 0; c < 6; ++c) wgt[c] = a.csi_w[(size_t)frame * K + (size_t)kpos[c]];
    }

    const RxWindows<N> w(a, frame);
    auto load = [&](int s, cf *v) __attribute__((always_inline)) { C::load(a, w, s, t, v); };      // (a lambda: see SixCarriers::load)
    int par = 0;
    cf v[8];
    C six;
    load(b0 + 1, v);
    F::template run<-1, true, cf, false>(v, xbuf, par, tw, t);
    six.start(v, t);

    const size_t block_words = (size_t)frame * (size_t)nblocks * WORDS;
    uint32_t *soft_out = SOFT ? reinterpret_cast<uint32_t *>(a.soft_out) + (size_t)frame * (size_t)nblocks * (3 * T) : nullptr;
    double acc_s = 0., acc_q = 0.;
    float worst = 1.0f;                    // min over the lane's decisions of min(|Re d|, |Im d|)^2 / |d|^2
    unsigned errors = 0u;
    for (int b = b0; b < b1; ++b) {
        load(b + 2, v);
        F::template run<-1, true, cf, false>(v, xbuf, par, tw, t);
        float ps = 0.f, pq = 0.f;
        float sre[SOFT ? 6 : 1], sim[SOFT ? 6 : 1];
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            const cf d = six.against_previous(v, c, t);
            const float dre = d.x, dim = d.y;
            if constexpr (SOFT) { sre[c] = dre; sim[c] = dim; }
            const unsigned I = dre < 0.f ? 1u : 0u, Q = dim < 0.f ? 1u : 0u;
            if (I) atomicOr(&blk[iword[c]], 1u << shift[c]);
            if (Q) atomicOr(&blk[qword[c]], 1u << shift[c]);
            const float ar = fabsf(dre), ai = fabsf(dim);
            const float p2 = fmaf(ar, ar, ai * ai);
            const float dq = ai - ar;                       // sqrt(2) Im(d conj(c)) up to its sign
            ps += p2;
            pq = fmaf(0.5f * dq, dq, pq);
            const float lo = fminf(ar, ai);
            worst = fminf(worst, p2 > 0.f ? (lo * lo) / p2 : 0.f);
        }
        acc_s += (double)ps;
        acc_q += (double)pq;
        if constexpr (SOFT) {
            // the symbol's power: the butterfly leaves the same sum in every lane of the wave (a + b = b + a exactly)
            const float pw = wave_sum_w<WL>(ps);
            if ((t & 63) == 0) red_p[t >> 6] = pw;
        }
        lds_barrier();
        if constexpr (SOFT) {
            float P = red_p[0];
#pragma unroll
            for (int w = 1; w < NW; ++w) P += red_p[w];
            const float q = P > 0.f ? 90.50966799187809f / sqrtf(P / (float)K) : 0.f;
            int8_t *sb = reinterpret_cast<int8_t *>(sblk);
#pragma unroll
            for (int c = 0; c < 6; ++c) {
                if constexpr (CSI) {
                    sb[nsoft[c]] = (int8_t)(int)fminf(fmaxf(rintf((-sre[c] * q) * wgt[c]), -127.f), 127.f);
                    sb[K + nsoft[c]] = (int8_t)(int)fminf(fmaxf(rintf((-sim[c] * q) * wgt[c]), -127.f), 127.f);
                } else {
                    sb[nsoft[c]] = (int8_t)(int)fminf(fmaxf(rintf(-sre[c] * q), -127.f), 127.f);
                    sb[K + nsoft[c]] = (int8_t)(int)fminf(fmaxf(rintf(-sim[c] * q), -127.f), 127.f);
                }
            }
            lds_barrier();
            uint32_t *dst = soft_out + (size_t)b * (3 * T);
#pragma unroll
            for (int j = 0; j < 3; ++j) dst[t + T * j] = sblk[t + T * j];
        }
        if (t < WORDS) {
            const uint32_t w = blk[t];
            blk[t] = 0u;                   // (the next symbol's ORs come behind the barriers of its transform)
            const size_t at = block_words + (size_t)b * WORDS + (size_t)t;
            if (a.bits_out) reinterpret_cast<uint32_t *>(a.bits_out)[at] = w;
            if (a.ref_bits) errors += (unsigned)__popc(w ^ reinterpret_cast<const uint32_t *>(a.ref_bits)[at]);
        }
    }

    // the run's share of the frame's figures: the lanes' through LDS (sixteen partial sums, then one lane), one atomic each
    red_s[t] = acc_s; red_q[t] = acc_q; red_m[t] = worst; red_e[t] = errors;
    lds_barrier();
    if (t < 16) {
        double s = 0., q = 0.;
        float m = 1.0f;
        unsigned e = 0u;
        for (int i = t; i < T; i += 16) { s += red_s[i]; q += red_q[i]; m = fminf(m, red_m[i]); e += red_e[i]; }
        red_s[t] = s; red_q[t] = q; red_m[t] = m; red_e[t] = e;
    }
    lds_barrier();
    if (t == 0) {
        double s = 0., q = 0.;
        float m = 1.0f;
        unsigned e = 0u;
        for (int i = 0; i < 16; ++i) { s += red_s[i]; q += red_q[i]; m = fminf(m, red_m[i]); e += red_e[i]; }
        DemodFrameStats *st = a.stats + frame;
        atomicAdd(&st->sum_signal, s);
        atomicAdd(&st->sum_quadrature, q);
        if (e) atomicAdd(&st->bit_errors, (unsigned long long)e);
        // the smallest margin as the LARGEST complement of its bit pattern (non-negative floats order like their bits):
        // a zeroed record is then "no decision yet"
        atomicMax(&st->min_margin_inv, ~__float_as_uint(sqrtf(m)));
    }
}

template <int LOGN> __global__ __launch_bounds__(Fft<LOGN>::T) void demod_kernel(DemodArgs a) { demod_body<LOGN, FORM_HARD>(a); }
template <int LOGN> __global__ __launch_bounds__(Fft<LOGN>::T) void demod_soft_kernel(DemodArgs a) { demod_body<LOGN, FORM_SOFT>(a); }
template <int LOGN> __global__ __launch_bounds__(Fft<LOGN>::T) void demod_csi_soft_kernel(DemodArgs a) { demod_body<LOGN, FORM_CSI>(a); }

// The carrier state (dabgpu_demod_csi*, dabgpu_demod_carrier_state*: the first pass), in FLOAT64 from the samples on.  The sums
// are specified as integers and are held to the float64 model count for count (include/dabgpu.h, "the carrier state"): one
// count is 2^-16 of a metric step, an fp32 value near 64 resolves half a count, and the fp32 transform lies 1e-7 from the
// exact one -- 0.4 counts per term.  So this pass does not share demod_body's transform: a radix-2 Stockham transform on
// double2 in LDS (two buffers, the twiddles exp(-2 pi i m / N), m < N/2, in a third), one workgroup per run of symbols as
// in demod_body, lane t owning the carrier positions t, t + LANES, ...: their previous-symbol values and their two integer
// sums stay in its registers.  Per symbol: window -> LDS, log2 N stages, d = z conj(z_prev), P = sum |d|^2 through LDS,
// q = 64 sqrt(2) / sqrt(P / K), the two terms rounded to integers.  One integer atomic per lane, carrier and figure at the
// end of the run: integer addition is associative, the sums depend neither on the run geometry nor on the order of arrival.
template <int LOGN> struct State64 {
    static constexpr int N = 1 << LOGN, K = 3 * N / 4, LANES = N / 2;    // a butterfly per lane and stage: 128 ... 1024 lanes
    static constexpr int PER = (K + LANES - 1) / LANES;          // carriers per lane
    static constexpr int BF = (N / 2) / LANES;                   // butterflies per lane and stage
    static constexpr size_t LDS_BYTES = (size_t)(2 * N + N / 2) * sizeof(double2) + (size_t)LANES * sizeof(double);
};

template <int LOGN> __global__ __launch_bounds__(State64<LOGN>::LANES) void demod_csi_state_kernel(DemodArgs a)
{
    typedef State64<LOGN> S;
    constexpr int N = S::N, K = S::K, LANES = S::LANES, PER = S::PER, BF = S::BF;
    // (dynamic LDS: 88 KiB in Mode I, more than a static block may hold; S::LDS_BYTES, asked for by the launch)
    extern __shared__ double2 state64_lds[];
    double2 (*buf)[N] = reinterpret_cast<double2 (*)[N]>(state64_lds);
    double2 *wtab = state64_lds + 2 * N;
    double *red = reinterpret_cast<double *>(state64_lds + 2 * N + N / 2);

    const int t = (int)threadIdx.x;
    const RxRun r = rx_run(a);
    if (r.idle) return;
    const int frame = r.frame, b0 = r.b0, b1 = r.b1;

    for (int m = t; m < N / 2; m += LANES) wtab[m] = twiddle64(m, N);
    const RxWindows<N> w(a, frame);

    // symbol s >= 1 of the frame -> its N bins in natural order; returns the buffer that holds them
    auto transform = [&](int s) __attribute__((always_inline)) -> const double2 * {
        const long long off = w.of(s);
        lds_barrier();                                           // (the readers of the symbol before are done; wtab is written)
        for (int i = t; i < N; i += LANES) {
            const cf x = ld_iq(a.iq, a.fmt, off + i);
            buf[0][i] = make_double2((double)x.x, (double)x.y);
        }
        lds_barrier_vm();
        int cur = 0, wstep = N / 2;                              // wstep = N / (2 ns)
#pragma unroll 1
        for (int ns = 1; ns < N; ns <<= 1, wstep >>= 1) {
#pragma unroll
            for (int e = 0; e < BF; ++e) {
                const int j = t + LANES * e, k = j & (ns - 1);
                const double2 w = wtab[k * wstep];
                const double2 x0 = buf[cur][j], x1 = buf[cur][j + N / 2];
                const double pr = x1.x * w.x - x1.y * w.y, pi = x1.x * w.y + x1.y * w.x;
                const int j0 = ((j - k) << 1) + k;               // (j / ns) 2 ns + j % ns
                buf[cur ^ 1][j0] = make_double2(x0.x + pr, x0.y + pi);
                buf[cur ^ 1][j0 + ns] = make_double2(x0.x - pr, x0.y - pi);
            }
            cur ^= 1;
            lds_barrier();
        }
        return buf[cur];
    };

    int bin[PER];
    double2 prev[PER];
    long long sum_a[PER], sum_v[PER];
#pragma unroll
    for (int c = 0; c < PER; ++c) {
        const int k = t + LANES * c;
        bin[c] = position_bin<N>(k);                             // (k >= K: a bin inside the table, never used)
        if (k >= K) bin[c] = 0;
        sum_a[c] = sum_v[c] = 0;
    }
    {
        const double2 *z = transform(b0 + 1);
#pragma unroll
        for (int c = 0; c < PER; ++c) prev[c] = z[bin[c]];
    }
    for (int b = b0; b < b1; ++b) {
        const double2 *z = transform(b + 2);
        double dre[PER], dim[PER], ps = 0.0;
#pragma unroll
        for (int c = 0; c < PER; ++c) {
            const double2 x = z[bin[c]], p = prev[c];
            prev[c] = x;
            dre[c] = x.x * p.x + x.y * p.y;                      // z conj(p)
            dim[c] = x.y * p.x - x.x * p.y;
            if (t + LANES * c < K) ps += dre[c] * dre[c] + dim[c] * dim[c];
        }
        red[t] = ps;
        lds_barrier();
        for (int half = LANES / 2; half >= 1; half >>= 1) {
            if (t < half) red[t] += red[t + half];
            lds_barrier();
        }
        const double P = red[0];
        const double q = P > 0.0 ? 64.0 * sqrt(2.0) / sqrt(P / (double)K) : 0.0;
        constexpr double kScale = (double)(1 << DABGPU_CSI_FRAC_BITS);
#pragma unroll
        for (int c = 0; c < PER; ++c) {
            const double ur = fabs(dre[c] * q), ui = fabs(dim[c] * q), dq = ui - ur;
            sum_a[c] += (long long)rint(kScale * (ur + ui) / 2.0);
            sum_v[c] += (long long)rint(kScale * (dq * dq) / 2.0);
        }
        // (red is rewritten behind the barriers of the next transform)
    }
    unsigned long long *st = a.csi_sums + (size_t)frame * (size_t)(2 * K);
#pragma unroll
    for (int c = 0; c < PER; ++c) {
        const int k = t + LANES * c;
        if (k < K) {
            atomicAdd(&st[2 * k], (unsigned long long)sum_a[c]);
            atomicAdd(&st[2 * k + 1], (unsigned long long)sum_v[c]);
        }
    }
}

// The weights of a frame from its carrier state (include/dabgpu.h, "the carrier state": the rule, operation by operation):
// one workgroup per frame, one lane per carrier (a lane takes carriers t, t + 256, ...).  The totals -- over all carriers,
// then DABGPU_CSI_TRIM_PASSES times over the carriers whose V_k lies within DABGPU_CSI_TRIM_FACTOR times the mean of the set
// before -- are integer sums (any order gives the same integer); the rest is float64 per carrier.
constexpr int kCsiWeightLanes = 256;
__global__ __launch_bounds__(kCsiWeightLanes) void demod_csi_weights_kernel(const unsigned long long *sums, float *w, int K, int unit)
{
    __shared__ long long red_n[kCsiWeightLanes], red_a[kCsiWeightLanes], red_v[kCsiWeightLanes];
    const int t = (int)threadIdx.x;
    const long long *st = reinterpret_cast<const long long *>(sums) + (size_t)blockIdx.x * (size_t)(2 * K);
    float *out = w + (size_t)blockIdx.x * (size_t)K;
    long long n = K, sa = 0, sv = 0;                 // the set before: its size and totals
    for (int pass = 0; pass <= DABGPU_CSI_TRIM_PASSES; ++pass) {
        long long ln = 0, la = 0, lv = 0;
        for (int k = t; k < K; k += kCsiWeightLanes) {
            const long long V = st[2 * k + 1];
            if (pass == 0 || V * n <= (long long)DABGPU_CSI_TRIM_FACTOR * sv) { ++ln; la += st[2 * k]; lv += V; }
        }
        red_n[t] = ln; red_a[t] = la; red_v[t] = lv;
        lds_barrier();
        for (int half = kCsiWeightLanes / 2; half >= 1; half >>= 1) {
            if (t < half) { red_n[t] += red_n[t + half]; red_a[t] += red_a[t + half]; red_v[t] += red_v[t + half]; }
            lds_barrier();
        }
        n = red_n[0]; sa = red_a[0]; sv = red_v[0];
        lds_barrier();                               // (everybody has read the totals before the next pass writes)
    }
    const bool flat = unit || sa <= 0 || sv <= 0;
    const double SA = (double)sa, SV = (double)sv;
    const double floor_v = SV / (double)(64ll * n);
    for (int k = t; k < K; k += kCsiWeightLanes) {
        double r = 1.0;
        if (!flat) {
            const double A = (double)st[2 * k], V = (double)st[2 * k + 1];
            r = fmin((double)DABGPU_CSI_MAX_WEIGHT, (A * SV) / (SA * fmax(V, floor_v)));
        }
        out[k] = (float)r;
    }
}

}  // namespace

// (demod_runs: how a frame's data symbols are split into runs -- forced: symbols per run, 0 = by the batch size.  A run costs
// one transform more than its symbols, so runs stay at four symbols or more; the grid aims at four workgroups per CU.)
void demod_runs(const Geometry &g, size_t n_frames, int forced, int *runs_per_frame, int *syms_per_run)
{
    const int nblocks = g.nb_symbols - 1;
    int spr;
    if (forced > 0) {
        spr = std::min(forced, nblocks);
    } else {
        const size_t want = n_frames ? (1024 + n_frames - 1) / n_frames : 1;
        const int runs = (int)std::min<size_t>(std::max<size_t>(want, 1), (size_t)((nblocks + 3) / 4));
        spr = (nblocks + runs - 1) / runs;
    }
    *syms_per_run = spr;
    *runs_per_frame = (nblocks + spr - 1) / spr;
}

hipError_t launch_demod(const DemodArgs &a, hipStream_t s)
{
    if (a.n_frames <= 0) return hipSuccess;
    if (a.early < 0 || a.early > a.g.sym_size - a.g.N || a.runs_per_frame < 1 || a.syms_per_run < 1 ||
        (a.fmt != 0 && a.fmt != 1) || a.g.K != 3 * a.g.N / 4)
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)a.n_frames * (unsigned)a.runs_per_frame);
    return by_fft_size(a.g.logN, [&](auto L) {
        const dim3 block(Fft<L>::T);
        if (a.csi_sums) {                   // the first pass of the weighted call: the carrier state alone
            typedef State64<L> S;           // (more than 64 KiB of dynamic LDS has to be asked for)
            hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(demod_csi_state_kernel<L>),
                                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)S::LDS_BYTES);
            if (e != hipSuccess) return e;
            DABGPU_LAUNCH_T(demod_csi_state_kernel, (L), grid, dim3(S::LANES), S::LDS_BYTES, s, a);
        } else if (a.soft_out && a.csi_w) { // the second pass: weighted softs, the hard call's bits and figures
            DABGPU_LAUNCH_T(demod_csi_soft_kernel, (L), grid, block, 0, s, a);
        } else if (a.soft_out) {
            DABGPU_LAUNCH_T(demod_soft_kernel, (L), grid, block, 0, s, a);
        } else {
            DABGPU_LAUNCH_T(demod_kernel, (L), grid, block, 0, s, a);
        }
        return hipGetLastError();
    });
}

hipError_t launch_csi_weights(const unsigned long long *sums, float *w, int K, int n_frames, bool unit, hipStream_t s)
{
    if (n_frames <= 0) return hipSuccess;
    DABGPU_LAUNCH(demod_csi_weights_kernel, dim3((unsigned)n_frames), dim3(kCsiWeightLanes), 0, s, sums, w, K, unit ? 1 : 0);
    return hipGetLastError();
}

}  // namespace dabgpu
