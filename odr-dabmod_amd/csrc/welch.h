// welch.h -- the rule the two Welch measurements share (spectrum.hip: the spectrum monitor; dpd.hip: the DPD cross-spectrum),
// once: segments of SPECTRUM_NFFT samples at a hop of half that, which of them a sample pair can use, how they are split into
// runs, the run a workgroup takes, how a lane walks its run's samples, and how the workgroups' rows of float64 partial sums
// become the sums.  Plain C++ for host and device: the kernels run these per lane, a host compiler builds them alone
// (tools/welch_check.cpp walks every run with a bounds-checking loader).
#pragma once
#include <stddef.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define WELCH_HD __host__ __device__ __forceinline__
#define WELCH_UNROLL _Pragma("unroll")
#else
#define WELCH_HD inline
#define WELCH_UNROLL
#endif

namespace dabgpu {

// kWelchLanes lanes per workgroup, lane t holds samples (and, after the transform, bins) t + 256 m, m = 0 ... 7.  Rows of
// scratch per launch: at most kSpectrumMaxRuns of 2048 sums (16 KiB each), kDpdMaxRuns of 4 x 2048 (64 KiB: 256 MiB).
enum { SPECTRUM_NFFT = 2048, kWelchHop = SPECTRUM_NFFT / 2, kWelchLanes = 256, kSpectrumMaxRuns = 1 << 16, kDpdMaxRuns = 4096 };

// segment i is samples 1024 i ... 1024 i + 2047: floor((n - 2048) / 1024) + 1 of them, or none
WELCH_HD long long welch_n_segments(size_t n) { return n >= (size_t)SPECTRUM_NFFT ? (long long)((n - SPECTRUM_NFFT) / kWelchHop) + 1 : 0; }

// the range of segments of an n-sample pair whose rx range (shifted by rx_offset) lies inside the buffer
WELCH_HD void dpd_segments(size_t n, long long rx_offset, long long *first, long long *count)
{
    const long long HOP = kWelchHop, n_seg = welch_n_segments(n);
    const long long lo = rx_offset < 0 ? (-rx_offset + HOP - 1) / HOP : 0;        // 1024 i + rx_offset >= 0
    const long long room = (long long)n - SPECTRUM_NFFT - rx_offset;              // 1024 i <= room
    const long long hi = room < 0 ? 0 : n_seg < room / HOP + 1 ? n_seg : room / HOP + 1;
    *first = lo < hi ? lo : 0;
    *count = lo < hi ? hi - lo : 0;
}

// How the segments are split into runs -- forced: segments per run, 0 = by the input size.  About 1024 workgroups per launch
// and four segments or more per run: a run reads half a segment more than its share.  Never more than max_runs rows of
// scratch, whatever is forced.
WELCH_HD void spectrum_runs(long long n_segments, int forced, int max_runs, int *n_runs, int *segs_per_run)
{
    *n_runs = 0;
    *segs_per_run = 1;
    if (n_segments <= 0) return;
    const long long runs = (n_segments + 3) / 4 < 1024 ? (n_segments + 3) / 4 : 1024, least = (n_segments + max_runs - 1) / max_runs;
    long long spr = forced <= 0 ? (n_segments + runs - 1) / runs : forced < n_segments ? forced : n_segments;
    spr = spr > least ? spr : least;
    spr = spr < 0x7fffffff ? spr : 0x7fffffff;
    *segs_per_run = (int)spr;
    *n_runs = (int)((n_segments + spr - 1) / spr);
}

// the run of workgroup wg: run segments s0 ... s1 - 1 (the last run may be shorter; a workgroup behind it is idle)
struct WelchRun { long long s0, s1; bool idle; };
WELCH_HD WelchRun welch_run(long long wg, int segs_per_run, long long n_segments)
{
    const long long s0 = wg * segs_per_run, s1 = s0 + segs_per_run < n_segments ? s0 + segs_per_run : n_segments;
    return {s0, s1, s0 >= s1};
}

// A lane's walk over the samples of one run: S load(long long sample_index) is the buffer.  After the k-th advance() raw[m] is
// sample first_sample + 1024 (k - 1) + t + 256 m, the current segment.  The second half of a segment is the first half of the
// next: raw[4..7] move to raw[0..3], and the half behind them (nxt) was requested one segment ahead -- when advance was told
// there is a next segment (`more`, the same for every lane) -- in front of the current segment's transform, which hides its
// latency.  Every sample of the run is loaded once, none outside it.
template <typename S, typename Load> struct WelchWalker {
    Load load;
    long long first;    // the lane's first sample of the run
    long long k;        // advances so far (the next half is formed from it, not carried: the compiler's loop is then the one the
    S raw[8], nxt[4];   //   spectrum kernel had with the walk written out)

    WELCH_HD void start(long long first_sample, int t)
    {
        first = first_sample + t;
        k = 0;
        WELCH_UNROLL for (int m = 0; m < 4; ++m) {
            raw[4 + m] = load(first + kWelchLanes * m);                 // the first half of the run's first segment
            nxt[m] = load(first + kWelchHop + kWelchLanes * m);         // ... and its second half
        }
    }
    WELCH_HD void advance(bool more)
    {
        WELCH_UNROLL for (int m = 0; m < 4; ++m) {
            raw[m] = raw[4 + m];
            raw[4 + m] = nxt[m];
        }
        ++k;
        if (!more) return;
        const long long half = first + (k + 1) * kWelchHop;
        WELCH_UNROLL for (int m = 0; m < 4; ++m) nxt[m] = load(half + kWelchLanes * m);
    }
};
template <typename S, typename Load> WELCH_HD WelchWalker<S, Load> welch_walker(Load load) { return WelchWalker<S, Load>{load}; }

// Entry k of the sums (one lane each): entry k of the n_runs rows of WIDTH partial sums in workgroup order, eight loads per
// step, then into acc (stored, or added when accumulating).  The lane of entry 0 keeps the segment count behind the WIDTH
// sums, as one unsigned long long.  (The row pointer is stepped, not formed from r: the loads then go out in the order the
// chain of additions needs them; profiles/welch_refactor.txt, part 3.)
template <int WIDTH> WELCH_HD void welch_row_sum(const double *rows, int n_runs, long long n_segments, double *acc, bool accumulate, int k)
{
    if (k >= WIDTH) return;
    const double *row = rows + k;
    double s = 0.;
    int r = 0;
    for (; r + 8 <= n_runs; r += 8, row += 8 * (size_t)WIDTH) {
        double x[8];
        WELCH_UNROLL for (int j = 0; j < 8; ++j) x[j] = row[(size_t)j * WIDTH];
        WELCH_UNROLL for (int j = 0; j < 8; ++j) s += x[j];
    }
    for (; r < n_runs; ++r, row += WIDTH) s += *row;
    acc[k] = accumulate ? acc[k] + s : s;
    if (k != 0) return;
    unsigned long long *count = reinterpret_cast<unsigned long long *>(acc + WIDTH);
    *count = (accumulate ? *count : 0ull) + (unsigned long long)n_segments;
}

}  // namespace dabgpu
