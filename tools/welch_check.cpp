// welch_check.cpp -- the rule the two Welch measurements share (odr-dabmod_amd/csrc/welch.h) on the host alone: the walk of a
// lane over every run's samples through a recording, bounds-checking loader; the run split against the two-step rule it
// replaced, written out here; the segment range of a sample pair against brute force.  No HIP library is linked.
//   c++ -std=c++17 -Iodr-dabmod_amd/csrc tools/welch_check.cpp                                      (tests/test_welch_host.py)
#include "welch.h"

#include <algorithm>
#include <cstdio>
#include <vector>

namespace {
int g_failed = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            if (++g_failed <= 20) std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
        }                                                                  \
    } while (0)

using namespace dabgpu;

// (a) Every run of n_segments segments from segment seg_first on, shifted by offset, as lane t walks it.  The buffer is the
// run's own range [1024 (seg_first + s0) + offset, 1024 (seg_first + s1 + 1) + offset), one counter per sample: a load outside
// it fails (and would be the sanitizer's, were the test left out), a sample of the lane loaded twice or never fails.
struct Sample { long long index; };
int check_walks()
{
    int walks = 0;
    for (long long n_segments = 1; n_segments <= 9; ++n_segments)
        for (int spr = 1; spr <= n_segments; ++spr)
            for (long long seg_first : {0ll, 3ll})
                for (long long offset : {0ll, 7ll, -300ll, 1000ll})
                    for (int t : {0, 1, 255}) {
                        const int n_runs = (int)((n_segments + spr - 1) / spr);
                        CHECK(welch_run(n_runs, spr, n_segments).idle);
                        for (int wg = 0; wg < n_runs; ++wg, ++walks) {
                            const WelchRun run = welch_run(wg, spr, n_segments);
                            CHECK(!run.idle && run.s0 == (long long)wg * spr && run.s1 > run.s0 && run.s1 <= n_segments);
                            CHECK(run.s1 - run.s0 == spr || (wg == n_runs - 1 && run.s1 == n_segments));
                            const long long lo = (seg_first + run.s0) * kWelchHop + offset, hi = (seg_first + run.s1 + 1) * kWelchHop + offset;
                            std::vector<int> loads((size_t)(hi - lo), 0);
                            auto x = welch_walker<Sample>([&](long long i) {
                                CHECK(i >= lo && i < hi);
                                if (i >= lo && i < hi) ++loads[(size_t)(i - lo)];
                                return Sample{i};
                            });
                            x.start(lo, t);
                            for (long long s = run.s0; s < run.s1; ++s) {
                                x.advance(s + 1 < run.s1);
                                for (int m = 0; m < 8; ++m)
                                    CHECK(x.raw[m].index == (seg_first + s) * kWelchHop + offset + t + kWelchLanes * m);
                            }
                            for (long long i = lo; i < hi; ++i) CHECK(loads[(size_t)(i - lo)] == ((i - lo) % kWelchLanes == t ? 1 : 0));
                        }
                    }
    return walks;
}

// (b) the split this header's spectrum_runs replaced: one cap of 65536 rows inside the rule, and a second split by the caller
// whose cap is 4096
void two_step_runs(long long n_segments, int forced, int max_runs, int *n_runs, int *segs_per_run)
{
    const long long first_cap = 1 << 16;
    if (n_segments <= 0) {
        *n_runs = 0;
        *segs_per_run = 1;
    } else {
        long long spr;
        if (forced > 0) {
            spr = std::min<long long>(forced, n_segments);
        } else {
            const long long runs = std::max<long long>(1, std::min<long long>(1024, (n_segments + 3) / 4));
            spr = (n_segments + runs - 1) / runs;
        }
        spr = std::max(spr, (n_segments + first_cap - 1) / first_cap);
        spr = std::min<long long>(spr, 0x7fffffff);
        *segs_per_run = (int)spr;
        *n_runs = (int)((n_segments + spr - 1) / spr);
    }
    if (max_runs < first_cap && *n_runs > max_runs) {
        *segs_per_run = (int)((n_segments + max_runs - 1) / max_runs);
        *n_runs = (int)((n_segments + *segs_per_run - 1) / *segs_per_run);
    }
}
int check_splits()
{
    int splits = 0;
    for (long long n_segments = 0; n_segments <= 300000; ++n_segments)         // (both caps: 4096 and 65536 runs of one segment)
        for (int forced : {0, 1, 3, 4096, 0x7fffffff})
            for (int max_runs : {(int)kSpectrumMaxRuns, (int)kDpdMaxRuns}) {
                int n_runs = -1, spr = -1, want_runs = -1, want_spr = -1;
                spectrum_runs(n_segments, forced, max_runs, &n_runs, &spr);
                two_step_runs(n_segments, forced, max_runs, &want_runs, &want_spr);
                CHECK(n_runs == want_runs && spr == want_spr);
                CHECK(spr >= 1 && (long long)n_runs * spr >= n_segments && n_runs <= max_runs);
                CHECK(n_runs == 0 ? n_segments == 0 : (long long)(n_runs - 1) * spr < n_segments);
                ++splits;
            }
    return splits;
}

// (c) segment i of an n-sample pair counts iff it lies inside tx and, shifted by the offset, inside rx; those that count form
// one range
int check_pairs()
{
    int pairs = 0;
    for (long long n = 0; n <= 6200; ++n) {
        CHECK(welch_n_segments((size_t)n) == (n < 2048 ? 0 : (n - 2048) / 1024 + 1));
        for (long long offset = -3000; offset <= 3000; ++offset, ++pairs) {
            long long want_first = 0, want_count = 0;
            bool one_range = true;
            for (long long i = 0; 1024 * i + 2048 <= n; ++i) {
                if (1024 * i + offset < 0 || 1024 * i + offset + 2048 > n) continue;
                if (!want_count) want_first = i;
                else if (i != want_first + want_count) one_range = false;
                ++want_count;
            }
            long long first = -1, count = -1;
            dpd_segments((size_t)n, offset, &first, &count);
            CHECK(one_range && first == want_first && count == want_count);
        }
    }
    return pairs;
}
}  // namespace

int main()
{
    const int walks = check_walks(), splits = check_splits(), pairs = check_pairs();
    if (g_failed) {
        std::fprintf(stderr, "welch_check: %d checks failed\n", g_failed);
        return 1;
    }
    std::printf("welch ok: %d runs walked, %d splits, %d sample pairs\n", walks, splits, pairs);
    return 0;
}
