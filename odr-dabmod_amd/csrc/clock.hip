// clock.hip -- the clock: a sampling-clock offset of at most 1000 ppm put on a sample stream or, with the opposite sign, taken
// off it (the resampler), and read from the data symbols of whole frames (the estimator, further down); include/dabgpu.h, "the
// clock".  The reference has no such stage.  Output m of the resampler is a function of its absolute index alone -- the input
// position m + floor(m step / 2^64) and the fraction behind it come from one 64 x 64-bit product, nothing accumulates -- so a
// stream cut into calls of any lengths, at any run geometry, gives the same bytes.
// The 31 samples of history the next call reads are stream_history.hip's.  A workgroup makes `run` consecutive outputs: their
// input span (run + run / 999 + 33 samples at most, the rate is that near 1) is staged in LDS as floats, then lane l
// makes outputs l, l + 256, ...: consecutive lanes read consecutive LDS words whatever the slip does, which therefore costs
// nothing -- an output's offset into the span is computed, never branched on.  The tap table stays in global memory (512 rows
// of pairs (T[p][j], T[p + 1][j] - T[p][j]), 128 KB: L2 and the vector cache hold it), one 16-byte load per two taps; the
// lanes of a wave read the same row or its neighbours.  No atomics, no scratch.
#include "device_common.h"
#include "turn_phase.h"
#include "fixed_order.h"     // wave_sum_w
#include "rx_symbols.h"      // the estimator's walk

namespace dabgpu {
namespace {

// output m: the input position i = m + floor(m step / 2^64) and F = the upper 32 bits of the low half of m step
DEV void clock_position(unsigned long long m, long long step, long long &i, uint32_t &F)
{
    const unsigned long long us = (unsigned long long)step;            // step + 2^64 when step < 0: the low half is the same,
    long long hi = (long long)__umul64hi(m, us);                       // the high half is m too large
    if (step < 0) hi -= (long long)m;
    i = (long long)m + hi;
    F = (uint32_t)((m * us) >> 32);
}

template <int IF, int OF> __global__ __launch_bounds__(256) void clock_kernel(const ClockArgs a)
{
    __shared__ float2 span[kClkSpan];
    const long long k0 = (long long)blockIdx.x * a.run;
    const int cnt = (int)min((long long)a.run, a.count - k0);
    const unsigned long long mb = a.m0 + (unsigned long long)k0;
    long long i_first, i_last;
    uint32_t F;
    clock_position(mb, a.step, i_first, F);
    clock_position(mb + (unsigned long long)(cnt - 1), a.step, i_last, F);
    // span[t] = input sample i_first - 15 + t; r: the same index counted from the call's first sample (>= -31)
    const int len = min((int)(i_last - i_first) + kClkTaps, kClkSpan);
    const long long r0 = i_first - kClkCentre - (long long)a.T;
    for (int t = threadIdx.x; t < len; t += 256) {
        const long long r = r0 + t;
        cf v = mk(0.f, 0.f);
        if (r >= 0) {
            if (r < a.n) v = load_sample<IF>(a.in, r);
        } else if (r >= -kClkHist) {
            v = a.hist[kClkHist + r];
        }
        span[t] = v;
    }
    __syncthreads();
    for (int k = threadIdx.x; k < cnt; k += 256) {
        long long i;
        clock_position(mb + (unsigned long long)k, a.step, i, F);
        const int o = min(max((int)(i - i_first), 0), len - kClkTaps);
        const float f = (float)(F & 0x7fffffu) * 1.1920928955078125e-07f;
        const float4 *row = reinterpret_cast<const float4 *>(a.tab + (size_t)(F >> 23) * kClkTaps);
        // taps 0 ... 31 in this order, one fused multiply-add per component and tap, from zero
        float re = 0.f, im = 0.f;
#pragma unroll
        for (int j = 0; j < kClkTaps; j += 2) {
            const float4 td = row[j / 2];
            const float h0 = fmaf(f, td.y, td.x), h1 = fmaf(f, td.w, td.z);
            const cf x0 = span[o + j], x1 = span[o + j + 1];
            re = fmaf(h0, x0.x, re);
            im = fmaf(h0, x0.y, im);
            re = fmaf(h1, x1.x, re);
            im = fmaf(h1, x1.y, im);
        }
        store_sample<OF>(a.out, k0 + k, re, im);
    }
}

// ---- the estimator.  demod.hip's walk (rx_symbols.h): one workgroup per run of data symbols, a lane's six carriers against
// the previous symbol.  Per block, float64 sums of the fp32 terms in one order: the lane's carriers in their order, an xor
// butterfly inside the wave (a + b = b + a exactly: every lane ends with the same sum), the waves in wave order through LDS.
// A block's sums do not depend on the run it is in.
template <int LOGN> __global__ __launch_bounds__(Fft<LOGN>::T) void sco_kernel(ScoArgs a)
{
    typedef Fft<LOGN> F;
    typedef SixCarriers<LOGN> C;
    constexpr int N = F::N, T = F::T;
    constexpr int NW = (T + 63) / 64, WL = T < 64 ? T : 64;
    __shared__ cf xbuf[2 * F::LDS_ELEMS];
    __shared__ double red[NW][kScoSums];

    const int t = (int)threadIdx.x;
    const int nblocks = a.g.nb_symbols - 1;
    const RxRun r = rx_run(a);
    if (r.idle) return;
    const int frame = r.frame, b0 = r.b0, b1 = r.b1;

    cf tw[F::NTW > 0 ? F::NTW : 1];
    F::template load_twiddles<false>(a.t.twiddle, t, tw);

    const RxWindows<N> w(a, frame);
    auto load = [&](int s, cf *v) __attribute__((always_inline)) { C::load(a, w, s, t, v); };      // (a lambda: see SixCarriers::load)
    int par = 0;
    cf v[8];
    C six;
    load(b0 + 1, v);
    F::template run<-1, true, cf, false>(v, xbuf, par, tw, t);
    six.start(v, t);

    for (int b = b0; b < b1; ++b) {
        load(b + 2, v);
        F::template run<-1, true, cf, false>(v, xbuf, par, tw, t);
        double sum[kScoSums] = {0., 0., 0., 0., 0.};
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            const cf d = six.against_previous(v, c, t);                 // demod's product
            const float dre = d.x, dim = d.y;
            // e = d conj(c), c the decided point (sgn Re d + j sgn Im d) / sqrt 2, a negative sign where demod decides a 1
            const float er = (fabsf(dre) + fabsf(dim)) * kSqrtHalf;
            const float ei = ((dre < 0.f ? -dim : dim) - (dim < 0.f ? -dre : dre)) * kSqrtHalf;
            const float mag = sqrtf(fmaf(er, er, ei * ei));
            sum[C::upper(c) ? 0 : 2] += (double)er;
            sum[C::upper(c) ? 1 : 3] += (double)ei;
            sum[4] += (double)mag;
        }
#pragma unroll
        for (int i = 0; i < kScoSums; ++i) sum[i] = wave_sum_w<WL>(sum[i]);
        if ((t & 63) == 0) {
#pragma unroll
            for (int i = 0; i < kScoSums; ++i) red[t >> 6][i] = sum[i];
        }
        lds_barrier();
        if (t < kScoSums) {                // (the next block's writes to red come behind the barriers of its transform)
            double s = red[0][t];
            for (int w = 1; w < NW; ++w) s += red[w][t];
            a.rows[((size_t)frame * (size_t)nblocks + (size_t)b) * kScoSums + t] = s;
        }
    }
}

// a frame's sums: its blocks in index order, one lane per (frame, sum)
__global__ __launch_bounds__(64) void sco_frames_kernel(const double *__restrict__ rows, double *__restrict__ frames, int n, int nblocks)
{
    const int i = (int)(blockIdx.x * 64 + threadIdx.x);
    if (i >= n * kScoSums) return;
    const int frame = i / kScoSums, k = i - frame * kScoSums;
    double s = 0.;
    for (int b = 0; b < nblocks; ++b) s += rows[((size_t)frame * (size_t)nblocks + (size_t)b) * kScoSums + k];
    frames[i] = s;
}

}  // namespace

hipError_t launch_sco(const ScoArgs &a, hipStream_t s)
{
    if (a.n_frames <= 0 || !a.iq || !a.rows || !a.frames || a.early < 0 || a.early > a.g.sym_size - a.g.N || a.runs_per_frame < 1 ||
        a.syms_per_run < 1 || (a.fmt != 0 && a.fmt != 1) || a.g.K != 3 * a.g.N / 4 ||
        (long long)a.runs_per_frame * a.syms_per_run < a.g.nb_symbols - 1)
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)a.n_frames * (unsigned)a.runs_per_frame);
    hipError_t e = by_fft_size(a.g.logN, [&](auto L) {
        DABGPU_LAUNCH_T(sco_kernel, (L), grid, dim3(Fft<L>::T), 0, s, a);
        return hipGetLastError();
    });
    if (e != hipSuccess) return e;
    DABGPU_LAUNCH(sco_frames_kernel, dim3((unsigned)((a.n_frames * kScoSums + 63) / 64)), dim3(64), 0, s, a.rows, a.frames, a.n_frames,
                  a.g.nb_symbols - 1);
    return hipGetLastError();
}

// outputs per workgroup: forced (1 ... kClkMaxRun), or 1024
int clock_run(size_t count, int forced)
{
    (void)count;
    if (forced > 0) return std::min(forced, kClkMaxRun);
    return 1024;
}

hipError_t launch_clock(const ClockArgs &a, hipStream_t s)
{
    if (!a.in || !a.out || !a.hist || !a.tab || a.n < 1 || a.count < 1 || (a.in_fmt != 0 && a.in_fmt != 1) ||
        (a.out_fmt != 0 && a.out_fmt != 1) || a.run < 1 || a.run > kClkMaxRun)
        return hipErrorInvalidValue;
    // what the kernel relies on: |step| <= 2^64 / 1000 (a run's span fits), and every output's 32 taps lie in
    // [T - 31, T + n - 1]
    if (a.step > 18446744073709552LL || a.step < -18446744073709552LL) return hipErrorInvalidValue;
    const unsigned __int128 w = ((unsigned __int128)1 << 64) + (__int128)a.step;
    const auto pos = [&](unsigned long long m) { return (long long)(((unsigned __int128)m * w) >> 64); };
    const __int128 lo = (__int128)pos(a.m0) - kClkCentre, hi = (__int128)pos(a.m0 + (unsigned long long)(a.count - 1)) + 16;
    if (lo < (__int128)a.T - kClkHist || hi > (__int128)a.T + a.n - 1) return hipErrorInvalidValue;
    const long long blocks = (a.count + a.run - 1) / a.run;
    if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    const dim3 grid((unsigned)blocks), block(256);
    if (a.in_fmt == 0 && a.out_fmt == 0) DABGPU_LAUNCH((clock_kernel<0, 0>), grid, block, 0, s, a);
    else if (a.in_fmt == 0) DABGPU_LAUNCH((clock_kernel<0, 1>), grid, block, 0, s, a);
    else if (a.out_fmt == 0) DABGPU_LAUNCH((clock_kernel<1, 0>), grid, block, 0, s, a);
    else DABGPU_LAUNCH((clock_kernel<1, 1>), grid, block, 0, s, a);
    return hipGetLastError();
}

}  // namespace dabgpu
