// resampler_runs.h -- how a resampler launch cuts its hops into runs, one workgroup per run.  Host arithmetic only: no HIP,
// nothing of the library, so that a test can compile it by itself.
#pragma once
#include <algorithm>
#include <cstddef>

namespace dabgpu {

// Hops per run.  forced > 0 (dabgpu_debug_resampler_run_hops) is taken as it is -- a value above nhops gives one workgroup;
// 0: from the call size alone.
//   hop_independent (resampler16_kernel, Mode I x2 / x4): no run prologue, so short streams are cut into single hops and long
//     ones into runs of 24 (four runs per Mode-I frame);
//   otherwise (resampler_kernel, resampler_rational_kernel, resampler_lane_kernel): every run starts with a forward transform
//     of the hop before it, so long streams get runs of 96 hops (one Mode-I frame) and short ones are cut finer so that the
//     launch still covers the chip (>= 512 workgroups when there are that many pairs of hops).
inline int resampler_run_hops(size_t nhops, bool hop_independent, int forced)
{
    if (forced > 0) return forced;
    return hop_independent ? (int)std::max<size_t>(1, std::min<size_t>(24, nhops / 1536))
                           : (int)std::max<size_t>(2, std::min<size_t>(96, nhops / 512));
}

inline unsigned resampler_run_grid(size_t nhops, int hops_per_run)
{
    return (unsigned)((nhops + (size_t)hops_per_run - 1) / (size_t)hops_per_run);
}

}  // namespace dabgpu
