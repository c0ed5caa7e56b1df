// stream_history.hip -- the history a streamed stage (channel.hip, clock.hip, tuner.hip) leaves for its next call: the call's
// last H input samples, as floats, into the other of the stage's two history buffers.  One lane per sample.
#include "device_common.h"
#include "turn_phase.h"

namespace dabgpu {
namespace {

template <int IF> __global__ __launch_bounds__(256)
void stream_history_kernel(const void *in, long long n, int H, const float2 *__restrict__ cur, float2 *__restrict__ next)
{
    const int j = (int)(blockIdx.x * 256 + threadIdx.x);
    if (j >= H) return;
    const long long r = n - H + j;                                      // (n >= 1: r < 0 reads cur[n + j], n + j < H)
    next[j] = r >= 0 ? load_sample<IF>(in, r) : cur[H + r];
}

}  // namespace

hipError_t launch_stream_history(const void *in, int in_fmt, long long n, int H, const float2 *cur, float2 *next, hipStream_t s)
{
    if (!in || !cur || !next || cur == next || n < 1 || in_fmt < 0 || in_fmt > 3 || H < 1 || H > kStreamMaxHist) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((H + 255) / 256)), block(256);
    switch (in_fmt) {
    case 0: DABGPU_LAUNCH(stream_history_kernel<0>, grid, block, 0, s, in, n, H, cur, next); break;
    case 1: DABGPU_LAUNCH(stream_history_kernel<1>, grid, block, 0, s, in, n, H, cur, next); break;
    case 2: DABGPU_LAUNCH(stream_history_kernel<2>, grid, block, 0, s, in, n, H, cur, next); break;
    default: DABGPU_LAUNCH(stream_history_kernel<3>, grid, block, 0, s, in, n, H, cur, next); break;
    }
    return hipGetLastError();
}

}  // namespace dabgpu
