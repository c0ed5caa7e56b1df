// channel.hip -- the channel emulator between the modulator's IQ and the receiver: at most 64 paths, each an integer delay, a
// complex gain and a Doppler rotation of its own, and seeded Gaussian noise (include/dabgpu.h, "the channel").  The reference
// has no such stage.  Every output sample is a function of its absolute index a = position + i alone -- the phase is the
// integer phase of sync.hip's extraction (nothing accumulates), the noise is Philox4x32-10 on the counter a >> 1 -- so a stream
// cut into calls of any lengths, at any run geometry, gives the same bytes.  No atomics, no LDS.
// A lane makes kChLane consecutive samples; the shifted reads x[a - d] go straight to memory, contiguous per path and eight-byte
// aligned only.  The 2047 samples of history the next call reads are stream_history.hip's.  The path table travels in the
// kernel arguments: uniform loads, and a new configuration is ordered behind the calls queued before it with nothing to copy.
#include "device_common.h"
#include "turn_phase.h"

namespace dabgpu {
namespace {

// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC11): counter (c0, c1, 0, 0)
DEV void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t k0, uint32_t k1, uint32_t w[4])
{
    uint32_t x0 = c0, x1 = c1, x2 = 0u, x3 = 0u;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t h0 = __umulhi(0xD2511F53u, x0), l0 = 0xD2511F53u * x0;
        const uint32_t h1 = __umulhi(0xCD9E8D57u, x2), l1 = 0xCD9E8D57u * x2;
        x0 = h1 ^ x1 ^ k0;
        x1 = l1;
        x2 = h0 ^ x3 ^ k1;
        x3 = l0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    w[0] = x0; w[1] = x1; w[2] = x2; w[3] = x3;
}

// one complex unit Gaussian from two words: Box-Muller, u = ((wa >> 9) + 1/2) 2^-23 (exact, never 0 or 1), the angle reduced
// exactly as every rotation here
DEV cf gauss_pair(uint32_t wa, uint32_t wb)
{
    const float u = ((float)(wa >> 9) + 0.5f) * 1.1920928955078125e-07f;
    const float r = sqrtf(-2.0f * logf(u));
    const cf e = turn_phase((unsigned long long)wb << 32);
    return mk(r * e.x, r * e.y);
}

// sample j of the call, j >= -kChMaxDelay: the input, or the history in front of it
template <int IF> DEV cf ld_x(const ChannelArgs &a, long long j)
{
    if (j >= 0) return load_sample<IF>(a.in, j);
    return a.hist[kChMaxDelay + j];
}

template <int IF, int OF> __global__ __launch_bounds__(256) void channel_kernel(const ChannelArgs a)
{
    const long long begin = (long long)blockIdx.x * a.run;
    const long long end = min(a.n, begin + (long long)a.run);
    for (long long i0 = begin + (long long)threadIdx.x * kChLane; i0 < end; i0 += kChTile) {
        bool on[kChLane];
        cf s0[kChLane], s1[kChLane];
#pragma unroll
        for (int k = 0; k < kChLane; ++k) {
            on[k] = i0 + k < end;
            s0[k] = mk(0.f, 0.f);
            s1[k] = mk(0.f, 0.f);
        }
        // the paths that do not rotate, in their given order
        for (int p = 0; p < a.n_static; ++p) {
            const long long j0 = i0 - (long long)a.path[p].delay;
            const cf g = mk(a.path[p].gr, a.path[p].gi);
#pragma unroll
            for (int k = 0; k < kChLane; ++k) {
                const cf x = on[k] ? ld_x<IF>(a, j0 + k) : mk(0.f, 0.f);
                s0[k] = cadd(s0[k], cmul(g, x));
            }
        }
        // the paths that do, in theirs: (g e^{j 2 pi theta}) x
        for (int p = a.n_static; p < a.n_paths; ++p) {
            const long long j0 = i0 - (long long)a.path[p].delay;
            const cf g = mk(a.path[p].gr, a.path[p].gi);
            const unsigned long long step = a.path[p].step;
#pragma unroll
            for (int k = 0; k < kChLane; ++k) {
                const cf x = on[k] ? ld_x<IF>(a, j0 + k) : mk(0.f, 0.f);
                const cf w = cmul(g, turn_phase((a.position + (unsigned long long)(i0 + k)) * step));
                s1[k] = cadd(s1[k], cmul(w, x));
            }
        }
        cf y[kChLane];
#pragma unroll
        for (int k = 0; k < kChLane; ++k) y[k] = cadd(s0[k], s1[k]);
        if (a.sigma > 0.f) {
            // one Philox block serves samples 2 c and 2 c + 1: a run that starts at an odd sample takes half a block at either end
            const unsigned long long a0 = a.position + (unsigned long long)i0;
            const unsigned long long c = a0 >> 1;
            const bool odd = (a0 & 1u) != 0u;
            uint32_t w0[4], w1[4], w2[4] = {0u, 0u, 0u, 0u};
            philox4x32_10((uint32_t)c, (uint32_t)(c >> 32), a.seed_lo, a.seed_hi, w0);
            philox4x32_10((uint32_t)(c + 1), (uint32_t)((c + 1) >> 32), a.seed_lo, a.seed_hi, w1);
            if (odd) philox4x32_10((uint32_t)(c + 2), (uint32_t)((c + 2) >> 32), a.seed_lo, a.seed_hi, w2);
            const cf n0 = gauss_pair(odd ? w0[2] : w0[0], odd ? w0[3] : w0[1]);
            const cf n1 = gauss_pair(odd ? w1[0] : w0[2], odd ? w1[1] : w0[3]);
            const cf n2 = gauss_pair(odd ? w1[2] : w1[0], odd ? w1[3] : w1[1]);
            const cf n3 = gauss_pair(odd ? w2[0] : w1[2], odd ? w2[1] : w1[3]);
            const cf nz[kChLane] = {n0, n1, n2, n3};
#pragma unroll
            for (int k = 0; k < kChLane; ++k) y[k] = mk(fmaf(a.sigma, nz[k].x, y[k].x), fmaf(a.sigma, nz[k].y, y[k].y));
        }
        if (OF == 0) {
            float2 *out = reinterpret_cast<float2 *>(a.out) + i0;
            if (on[kChLane - 1] && ((uintptr_t)out & 15u) == 0) {     // (the same values either way: only the store's width differs)
                reinterpret_cast<float4 *>(out)[0] = make_float4(y[0].x, y[0].y, y[1].x, y[1].y);
                reinterpret_cast<float4 *>(out)[1] = make_float4(y[2].x, y[2].y, y[3].x, y[3].y);
            } else {
#pragma unroll
                for (int k = 0; k < kChLane; ++k)
                    if (on[k]) out[k] = y[k];
            }
        } else {
            uint32_t *out = reinterpret_cast<uint32_t *>(a.out) + i0;
            unsigned unused = 0;
            uint32_t v[kChLane];
#pragma unroll
            for (int k = 0; k < kChLane; ++k) v[k] = s16_pair<unsigned &>(y[k].x, y[k].y, unused);
            if (on[kChLane - 1] && ((uintptr_t)out & 15u) == 0) {
                reinterpret_cast<uint4 *>(out)[0] = make_uint4(v[0], v[1], v[2], v[3]);
            } else {
#pragma unroll
                for (int k = 0; k < kChLane; ++k)
                    if (on[k]) out[k] = v[k];
            }
        }
    }
}

constexpr int kChMaxRun = 8 * kChTile;

}  // namespace

// samples per workgroup: forced (rounded up to whole lanes), or passes of kChTile so that a large call still has thousands
// of workgroups
int channel_run(size_t n, int forced)
{
    if (forced > 0) return (int)std::min<long long>(((long long)forced + kChLane - 1) / kChLane * kChLane, 1 << 30);
    const size_t passes = std::min<size_t>(std::max<size_t>(n / ((size_t)kChTile * 4096), 1), kChMaxRun / kChTile);
    return (int)passes * kChTile;
}

hipError_t launch_channel(const ChannelArgs &a, hipStream_t s)
{
    if (!a.in || !a.out || !a.hist || a.n < 1 || (a.in_fmt != 0 && a.in_fmt != 1) || (a.out_fmt != 0 && a.out_fmt != 1) ||
        a.n_static < 0 || a.n_static > a.n_paths || a.n_paths > kChMaxPaths || a.run < kChLane || a.run % kChLane || !(a.sigma >= 0.f))
        return hipErrorInvalidValue;
    for (int p = 0; p < a.n_paths; ++p)
        if (a.path[p].delay > (uint32_t)kChMaxDelay || (a.path[p].step == 0) != (p < a.n_static)) return hipErrorInvalidValue;
    const long long blocks = (a.n + a.run - 1) / a.run;
    if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    const dim3 grid((unsigned)blocks), block(256);
    if (a.in_fmt == 0 && a.out_fmt == 0) DABGPU_LAUNCH((channel_kernel<0, 0>), grid, block, 0, s, a);
    else if (a.in_fmt == 0) DABGPU_LAUNCH((channel_kernel<0, 1>), grid, block, 0, s, a);
    else if (a.out_fmt == 0) DABGPU_LAUNCH((channel_kernel<1, 0>), grid, block, 0, s, a);
    else DABGPU_LAUNCH((channel_kernel<1, 1>), grid, block, 0, s, a);
    return hipGetLastError();
}

}  // namespace dabgpu
