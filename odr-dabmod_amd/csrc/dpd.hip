// dpd.hip -- what a predistortion estimator needs from a block of transmitted samples (tx) and the matching capture of the
// amplifier's feedback path (rx), formed on the device:
//   dpd_xspectrum_kernel<FMT_TX>  Welch cross-spectrum of the two buffers: spectrum_kernel's segments, runs and walk (welch.h),
//                                 rectangular window, Fft<11>::run<-1>, float64 sums per lane, one row per workgroup; and
//                                 dpd_xspectrum_reduce_kernel, welch.h's row sum.  Only the four cross products are this
//                                 file's own.  Integer lag, sub-sample delay, gain and coherence follow on the host.
//   dpd_stats_kernel<FMT_TX>      the aligned amplitude-bin statistics: one lane per tx sample, the rx window of a tile
//                                 through LDS (each rx sample is read from memory once per tile), a 32-tap fractional-delay
//                                 filter and a complex gain on rx, the bin from |tx|^2, six figures per bin.
// No floating-point atomics anywhere.  The statistics are sums of INTEGERS (every term is rounded once, then added with
// integer atomics, LDS first, one global 64-bit add per bin and figure and workgroup): the same bits for every repetition and
// every tile size.  tx is complexf or s16 pairs (the chain writes both), rx is complexf.
#include "device_common.h"
#include "turn_phase.h"     // load_sample

namespace dabgpu {
namespace {

typedef Fft<11> SF;
static_assert(SF::N == SPECTRUM_NFFT && SF::T == kWelchLanes, "2048 points on 256 lanes");

// One workgroup = one run of consecutive segments (welch_run); run segment s is segment a.seg_first + s of the buffers, walked
// by two WelchWalkers: tx, and rx at a.rx_offset.  After the two transforms lane t holds bins t + 256 m (FFT order) of TX and
// RX: S += TX conj(RX), P_tx += |TX|^2, P_rx += |RX|^2, products in fp32, sums in float64.
template <int FMT> __global__ __launch_bounds__(SF::T) void dpd_xspectrum_kernel(DpdXspecArgs a)
{
    constexpr int T = SF::T;
    __shared__ cf xbuf[2 * SF::LDS_ELEMS];

    const int t = (int)threadIdx.x;
    const WelchRun run = welch_run(blockIdx.x, a.segs_per_run, a.n_segments);
    if (run.idle) return;

    cf tw[SF::NTW];
    SF::template load_twiddles<false>(a.twiddle, t, tw);

    // (launch_dpd_xspectrum has made sure that every segment of the range lies inside both buffers)
    auto xt = welch_walker<cf>([tx = a.tx](long long i) { return load_sample<FMT>(tx, i); });
    auto xr = welch_walker<cf>([rx = a.rx](long long i) { return rx[i]; });
    xt.start((a.seg_first + run.s0) * kWelchHop, t);
    xr.start((a.seg_first + run.s0) * kWelchHop + a.rx_offset, t);

    double sre[8], sim[8], ptx[8], prx[8];
#pragma unroll
    for (int m = 0; m < 8; ++m) sre[m] = sim[m] = ptx[m] = prx[m] = 0.;
    int par = 0;
    for (long long s = run.s0; s < run.s1; ++s) {
        xt.advance(s + 1 < run.s1);
        xr.advance(s + 1 < run.s1);
        cf u[8], v[8];
#pragma unroll
        for (int m = 0; m < 8; ++m) u[m] = xt.raw[m];
        SF::template run<-1, true, cf, false>(u, xbuf, par, tw, t);
#pragma unroll
        for (int m = 0; m < 8; ++m) v[m] = xr.raw[m];
        SF::template run<-1, true, cf, false>(v, xbuf, par, tw, t);
#pragma unroll
        for (int m = 0; m < 8; ++m) {
            sre[m] += (double)fmaf(u[m].x, v[m].x, u[m].y * v[m].y);
            sim[m] += (double)fmaf(u[m].y, v[m].x, -(u[m].x * v[m].y));
            ptx[m] += (double)fmaf(u[m].x, u[m].x, u[m].y * u[m].y);
            prx[m] += (double)fmaf(v[m].x, v[m].x, v[m].y * v[m].y);
        }
    }

    double *row = a.rows + (size_t)blockIdx.x * (4 * SPECTRUM_NFFT) + t;
#pragma unroll
    for (int m = 0; m < 8; ++m) {
        row[T * m] = sre[m];
        row[SPECTRUM_NFFT + T * m] = sim[m];
        row[2 * SPECTRUM_NFFT + T * m] = ptx[m];
        row[3 * SPECTRUM_NFFT + T * m] = prx[m];
    }
}

// (always stored: a cross-spectrum call starts over)
__global__ __launch_bounds__(64) void dpd_xspectrum_reduce_kernel(DpdXspecArgs a)
{
    welch_row_sum<4 * SPECTRUM_NFFT>(a.rows, a.n_runs, a.n_segments, a.acc, false, (int)(blockIdx.x * blockDim.x + threadIdx.x));
}

// dpd_stats_kernel: workgroup w owns the tx samples (a.tile_first + w) tile ... + tile - 1; lane t takes samples t + 256 k of
// the tile.  The rx window of the tile -- rx[base + lag - 15 ... base + lag + tile + 15] -- goes through LDS once (entries
// outside the buffer are zero and never used: a sample is used only when all 32 taps lie inside rx, a.i_first <= i <
// a.i_end).  Every figure of a sample is rounded ONCE to an integer (amplitudes in units of peak 2^-24, |r|^2 in units of
// peak^2 2^-24, phases in units of 2^-24 rad, phase^2 in units of 2^-24 rad^2; |r| clamped at 16 peak, so no term passes
// 2^32) and added with integer atomics: the result does not depend on the order.
template <int FMT> __global__ __launch_bounds__(256) void dpd_stats_kernel(DpdStatsArgs a)
{
    constexpr int NSUM = DPD_MAX_BINS * DPD_FIGURES;
    __shared__ cf win[DPD_TILE_MAX + DPD_TAPS];
    __shared__ unsigned long long bins[NSUM + 2];
    __shared__ float edge[DPD_MAX_BINS + 1];

    const int t = (int)threadIdx.x;
    const long long base = (a.tile_first + (long long)blockIdx.x) * a.tile;
    const long long w0 = base + a.lag - DPD_TAP_CENTRE;
    for (int k = t; k < a.tile + DPD_TAPS - 1; k += 256) {
        const long long p = w0 + k;
        win[k] = (p >= 0 && p < a.n) ? a.rx[p] : mk(0.f, 0.f);
    }
    for (int k = t; k < NSUM + 2; k += 256) bins[k] = 0ull;
    for (int k = t; k <= a.n_bins; k += 256) edge[k] = a.edge2[k];
    lds_barrier();

    const double ua = 16777216.0 / (double)a.peak;
    const double ua2 = ua / (double)a.peak;
    const float rmax = 16.f * a.peak;
    unsigned used = 0, over = 0;
    for (int j = t; j < a.tile; j += 256) {
        const long long i = base + j;
        if (i < a.i_first || i >= a.i_end) continue;
        const cf x = load_sample<FMT>(a.tx, (size_t)i);
        float sr = 0.f, si = 0.f;
#pragma unroll
        for (int q = 0; q < DPD_TAPS; ++q) {
            const cf c = win[j + q];
            sr = fmaf(a.h[q], c.x, sr);
            si = fmaf(a.h[q], c.y, si);
        }
        const float rr = fmaf(a.g_re, sr, -(a.g_im * si)), ri = fmaf(a.g_re, si, a.g_im * sr);
        ++used;
        // (no contraction: the bin of a sample is a function of its two fp32 components alone, and r = t gives phase 0)
        const float a2 = __fadd_rn(__fmul_rn(x.x, x.x), __fmul_rn(x.y, x.y));
        int lo = 0, hi = a.n_bins + 1;                     // edge2[lo] <= a2 < edge2[hi] (edge2[0] = 0 holds for every a2)
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (edge[mid] <= a2) lo = mid; else hi = mid;
        }
        if (lo >= a.n_bins) {
            ++over;
            continue;
        }
        const float at = sqrtf(a2);
        const float ar = fminf(sqrtf(__fadd_rn(__fmul_rn(rr, rr), __fmul_rn(ri, ri))), rmax);
        const float pre = __fadd_rn(__fmul_rn(rr, x.x), __fmul_rn(ri, x.y));
        const float pim = __fsub_rn(__fmul_rn(ri, x.x), __fmul_rn(rr, x.y));
        const float phi = atan2f(pim, pre);
        unsigned long long *b = bins + lo * DPD_FIGURES;
        atomicAdd(b + 0, 1ull);
        atomicAdd(b + 1, (unsigned long long)__double2ll_rn((double)at * ua));
        atomicAdd(b + 2, (unsigned long long)__double2ll_rn((double)ar * ua));
        atomicAdd(b + 3, (unsigned long long)__double2ll_rn((double)phi * 16777216.0));        // (signed: two's complement)
        atomicAdd(b + 4, (unsigned long long)__double2ll_rn((double)ar * (double)ar * ua2));
        atomicAdd(b + 5, (unsigned long long)__double2ll_rn((double)phi * (double)phi * 16777216.0));
    }
    if (over) atomicAdd(bins + NSUM, (unsigned long long)over);
    if (used) atomicAdd(bins + NSUM + 1, (unsigned long long)used);
    lds_barrier();
    for (int k = t; k < a.n_bins * DPD_FIGURES; k += 256)
        if (bins[k]) atomicAdd(a.sums + k, bins[k]);
    if (t < 2 && bins[NSUM + t]) atomicAdd(a.sums + NSUM + t, bins[NSUM + t]);
}

}  // namespace

hipError_t launch_dpd_xspectrum(const DpdXspecArgs &a, size_t n_samples, hipStream_t s)
{
    long long first, count;
    dpd_segments(n_samples, a.rx_offset, &first, &count);
    if (first != a.seg_first || count != a.n_segments || check_welch(a, kDpdMaxRuns) != hipSuccess) return hipErrorInvalidValue;
    if (a.n_segments > 0) {
        if (!a.tx || !a.rx) return hipErrorInvalidValue;
        const dim3 grid((unsigned)a.n_runs), block(SF::T);
        switch (a.fmt) {
        case 0: DABGPU_LAUNCH(dpd_xspectrum_kernel<0>, grid, block, 0, s, a); break;
        case 1: DABGPU_LAUNCH(dpd_xspectrum_kernel<1>, grid, block, 0, s, a); break;
        default: return hipErrorInvalidValue;
        }
    }
    DABGPU_LAUNCH(dpd_xspectrum_reduce_kernel, dim3(4 * SPECTRUM_NFFT / 64), dim3(64), 0, s, a);
    return hipGetLastError();
}

void dpd_used_range(long long n, long long lag, long long *i_first, long long *i_end)
{
    // rx[i + lag - 15] ... rx[i + lag + 16] inside [0, n)
    *i_first = std::max<long long>(0, DPD_TAP_CENTRE - lag);
    *i_end = std::min<long long>(n, n - (DPD_TAPS - 1 - DPD_TAP_CENTRE) - lag);
    if (*i_end < *i_first) *i_end = *i_first;
}

hipError_t launch_dpd_stats(DpdStatsArgs a, hipStream_t s)
{
    if (a.n < 0 || a.tile < 256 || a.tile > DPD_TILE_MAX || a.tile % 256 || a.n_bins < 1 || a.n_bins > DPD_MAX_BINS ||
        !(a.peak > 0.f) || !a.sums || !a.edge2)
        return hipErrorInvalidValue;
    dpd_used_range(a.n, a.lag, &a.i_first, &a.i_end);
    if (a.i_first >= a.i_end) return hipSuccess;
    if (!a.tx || !a.rx) return hipErrorInvalidValue;
    a.tile_first = a.i_first / a.tile;
    const long long tiles = (a.i_end + a.tile - 1) / a.tile - a.tile_first;
    if (tiles > 0x7fffffffll) return hipErrorInvalidValue;
    const dim3 grid((unsigned)tiles), block(256);
    switch (a.fmt) {
    case 0: DABGPU_LAUNCH(dpd_stats_kernel<0>, grid, block, 0, s, a); break;
    case 1: DABGPU_LAUNCH(dpd_stats_kernel<1>, grid, block, 0, s, a); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace dabgpu
