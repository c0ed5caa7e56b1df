// spectrum.hip -- the spectrum monitor: a Welch averaged periodogram of any sample buffer the library writes or is handed.
// Segments of 2048 samples at a hop of 1024 in every transmission mode, a window from a table, the forward transform the
// receiver runs (Fft<11>::run<-1>, 256 lanes, eight points per lane), |X|^2 in fp32, float64 sums.  No symbol timing, no
// native rate, no particular sample format: complexf, s16, u8 (byte - 128) and s8.  Two kernels: spectrum_kernel<FMT> leaves
// one row of 2048 partial sums per workgroup, spectrum_reduce_kernel adds the rows in workgroup order.  No floating-point
// atomics: the result is a function of input, window and run geometry alone.  Segments, runs, the walk over a run's samples
// and the row sum are welch.h's, shared with dpd.hip; the window multiply and |X|^2 are this file's own.
#include "device_common.h"
#include "turn_phase.h"     // load_sample

namespace dabgpu {
namespace {

typedef Fft<11> SF;
static_assert(SF::N == SPECTRUM_NFFT && SF::T == kWelchLanes, "2048 points on 256 lanes");

// One workgroup = one run of consecutive segments (welch_run), walked by one WelchWalker: lane t holds the raw samples
// x[t + 256 m] of the current segment in raw[m].  The windowed copy goes through the transform; afterwards lane t holds bins
// t + 256 m (FFT order, bin 0 = DC), whose |X|^2 go to eight float64 accumulators.
template <int FMT> __global__ __launch_bounds__(SF::T) void spectrum_kernel(SpectrumArgs a)
{
    constexpr int T = SF::T;
    __shared__ cf xbuf[2 * SF::LDS_ELEMS];

    const int t = (int)threadIdx.x;
    const WelchRun run = welch_run(blockIdx.x, a.segs_per_run, a.n_segments);
    if (run.idle) return;

    cf tw[SF::NTW];
    SF::template load_twiddles<false>(a.twiddle, t, tw);
    float w[8];
#pragma unroll
    for (int m = 0; m < 8; ++m) w[m] = a.window[t + T * m];

    auto x = welch_walker<cf>([iq = a.iq](long long i) { return load_sample<FMT>(iq, i); });
    x.start(run.s0 * kWelchHop, t);

    double acc[8];
#pragma unroll
    for (int m = 0; m < 8; ++m) acc[m] = 0.;
    int par = 0;
    for (long long s = run.s0; s < run.s1; ++s) {
        cf v[8];
        x.advance(s + 1 < run.s1);
#pragma unroll
        for (int m = 0; m < 8; ++m) v[m] = mk(x.raw[m].x * w[m], x.raw[m].y * w[m]);
        SF::template run<-1, true, cf, false>(v, xbuf, par, tw, t);
#pragma unroll
        for (int m = 0; m < 8; ++m) acc[m] += (double)fmaf(v[m].x, v[m].x, v[m].y * v[m].y);
    }

    double *row = a.rows + (size_t)blockIdx.x * SPECTRUM_NFFT + t;
#pragma unroll
    for (int m = 0; m < 8; ++m) row[T * m] = acc[m];
}

__global__ __launch_bounds__(64) void spectrum_reduce_kernel(SpectrumArgs a)
{
    welch_row_sum<SPECTRUM_NFFT>(a.rows, a.n_runs, a.n_segments, a.acc, a.accumulate != 0, (int)(blockIdx.x * blockDim.x + threadIdx.x));
}

}  // namespace

hipError_t check_welch(const WelchArgs &a, int max_runs)
{
    if (a.n_segments < 0 || a.n_runs < 0 || a.segs_per_run < 1 || a.n_runs > max_runs || (long long)a.n_runs * a.segs_per_run < a.n_segments ||
        (a.n_segments > 0 && a.n_runs < 1) || !a.acc || !a.rows || (a.n_segments > 0 && !a.twiddle))
        return hipErrorInvalidValue;
    return hipSuccess;
}

hipError_t launch_spectrum(const SpectrumArgs &a, hipStream_t s)
{
    if (check_welch(a, kSpectrumMaxRuns) != hipSuccess) return hipErrorInvalidValue;
    if (a.n_segments > 0) {
        if (!a.iq || !a.window) return hipErrorInvalidValue;
        const dim3 grid((unsigned)a.n_runs), block(SF::T);
        switch (a.fmt) {
        case 0: DABGPU_LAUNCH(spectrum_kernel<0>, grid, block, 0, s, a); break;
        case 1: DABGPU_LAUNCH(spectrum_kernel<1>, grid, block, 0, s, a); break;
        case 2: DABGPU_LAUNCH(spectrum_kernel<2>, grid, block, 0, s, a); break;
        case 3: DABGPU_LAUNCH(spectrum_kernel<3>, grid, block, 0, s, a); break;
        default: return hipErrorInvalidValue;
        }
    }
    DABGPU_LAUNCH(spectrum_reduce_kernel, dim3(SPECTRUM_NFFT / 64), dim3(64), 0, s, a);
    return hipGetLastError();
}

}  // namespace dabgpu
