// spectrum.hip -- the spectrum monitor: a Welch averaged periodogram of any sample buffer the library writes or is handed.
// Segments of 2048 samples at a hop of 1024 in every transmission mode, a window from a table, the forward transform the
// receiver runs (Fft<11>::run<-1>, 256 lanes, eight points per lane), |X|^2 in fp32, float64 sums.  No symbol timing, no
// native rate, no particular sample format: complexf, s16, u8 (byte - 128) and s8.  Two kernels: spectrum_kernel<FMT> leaves
// one row of 2048 partial sums per workgroup, spectrum_reduce_kernel adds the rows in workgroup order.  No floating-point
// atomics: the result is a function of input, window and run geometry alone.
#include "device_common.h"
#include "turn_phase.h"     // load_sample

namespace dabgpu {
namespace {

typedef Fft<11> SF;
static_assert(SF::N == SPECTRUM_NFFT && SF::T == 256, "2048 points on 256 lanes");

// One workgroup = one RUN of consecutive segments (a.segs_per_run of them; the last run may be shorter).  Segment i is
// samples 1024 i ... 1024 i + 2047; lane t holds the raw samples x[t + 256 m] of the current segment in raw[m].  The next
// segment's first half is this one's second half: raw[4..7] move to raw[0..3] and four samples per lane are loaded (one segment
// ahead, into nxt), so every sample is read from memory once per run.  The windowed copy goes through the transform; afterwards lane t holds bins
// t + 256 m (FFT order, bin 0 = DC), whose |X|^2 go to eight float64 accumulators.
template <int FMT> __global__ __launch_bounds__(SF::T) void spectrum_kernel(SpectrumArgs a)
{
    constexpr int T = SF::T, HOP = SPECTRUM_NFFT / 2;
    __shared__ cf xbuf[2 * SF::LDS_ELEMS];

    const int t = (int)threadIdx.x;
    const long long s0 = (long long)blockIdx.x * a.segs_per_run;
    const long long s1 = s0 + a.segs_per_run < a.n_segments ? s0 + a.segs_per_run : a.n_segments;
    if (s0 >= s1) return;

    cf tw[SF::NTW];
    SF::template load_twiddles<false>(a.twiddle, t, tw);
    float w[8];
#pragma unroll
    for (int m = 0; m < 8; ++m) w[m] = a.window[t + T * m];

    cf raw[8], nxt[4];
    const size_t first = (size_t)s0 * HOP + (size_t)t;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        raw[4 + m] = load_sample<FMT>(a.iq, first + T * m);                                // the first half of segment s0
        nxt[m] = load_sample<FMT>(a.iq, first + HOP + T * m);                              // ... and its second half
    }

    double acc[8];
#pragma unroll
    for (int m = 0; m < 8; ++m) acc[m] = 0.;
    int par = 0;
    for (long long s = s0; s < s1; ++s) {
        cf v[8];
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            raw[m] = raw[4 + m];
            raw[4 + m] = nxt[m];
        }
        // the second half of the NEXT segment, requested ahead of this one's transform, which hides its latency
        // (s + 1 < s1 is the same for every lane; the last segment of the input ends at (n_segments + 1) HOP)
        if (s + 1 < s1) {
            const size_t half = (size_t)(s + 2) * HOP + (size_t)t;
#pragma unroll
            for (int m = 0; m < 4; ++m) nxt[m] = load_sample<FMT>(a.iq, half + T * m);
        }
#pragma unroll
        for (int m = 0; m < 8; ++m) v[m] = mk(raw[m].x * w[m], raw[m].y * w[m]);
        SF::template run<-1, true, cf, false>(v, xbuf, par, tw, t);
#pragma unroll
        for (int m = 0; m < 8; ++m) acc[m] += (double)fmaf(v[m].x, v[m].x, v[m].y * v[m].y);
    }

    double *row = a.rows + (size_t)blockIdx.x * SPECTRUM_NFFT + t;
#pragma unroll
    for (int m = 0; m < 8; ++m) row[T * m] = acc[m];
}

// One lane per bin: the rows in workgroup order, then into the context's sums (stored, or added when accumulating).  Lane 0
// keeps the segment count behind the 2048 sums.
__global__ __launch_bounds__(64) void spectrum_reduce_kernel(SpectrumArgs a)
{
    const int k = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (k >= SPECTRUM_NFFT) return;
    const double *row = a.rows + k;
    double s = 0.;
    int r = 0;
    for (; r + 8 <= a.n_runs; r += 8) {
        double x[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) x[j] = row[(size_t)(r + j) * SPECTRUM_NFFT];
#pragma unroll
        for (int j = 0; j < 8; ++j) s += x[j];
    }
    for (; r < a.n_runs; ++r) s += row[(size_t)r * SPECTRUM_NFFT];
    a.acc[k] = a.accumulate ? a.acc[k] + s : s;
    if (k == 0) {
        unsigned long long *count = reinterpret_cast<unsigned long long *>(a.acc + SPECTRUM_NFFT);
        *count = (a.accumulate ? *count : 0ull) + (unsigned long long)a.n_segments;
    }
}

}  // namespace

// (spectrum_runs: how the segments are split into runs -- forced: segments per run, 0 = by the input size.  About 1024
// workgroups per launch and four segments or more per run: a run reads half a segment more than its share.  Never more
// than kSpectrumMaxRuns rows of scratch, whatever is forced.)
void spectrum_runs(long long n_segments, int forced, int *n_runs, int *segs_per_run)
{
    long long spr;
    if (n_segments <= 0) {
        *n_runs = 0;
        *segs_per_run = 1;
        return;
    }
    if (forced > 0) {
        spr = std::min<long long>(forced, n_segments);
    } else {
        const long long runs = std::max<long long>(1, std::min<long long>(1024, (n_segments + 3) / 4));
        spr = (n_segments + runs - 1) / runs;
    }
    spr = std::max(spr, (n_segments + kSpectrumMaxRuns - 1) / kSpectrumMaxRuns);
    spr = std::min<long long>(spr, 0x7fffffff);
    *segs_per_run = (int)spr;
    *n_runs = (int)((n_segments + spr - 1) / spr);
}

hipError_t launch_spectrum(const SpectrumArgs &a, hipStream_t s)
{
    if (a.n_segments < 0 || a.n_runs < 0 || a.segs_per_run < 1 || a.n_runs > kSpectrumMaxRuns ||
        (long long)a.n_runs * a.segs_per_run < a.n_segments || (a.n_segments > 0 && a.n_runs < 1) || !a.acc)
        return hipErrorInvalidValue;
    if (a.n_segments > 0) {
        if (!a.iq || !a.rows || !a.twiddle || !a.window) return hipErrorInvalidValue;
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
