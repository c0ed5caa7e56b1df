// tuner.hip -- the tuner: a mixer, a channel filter and a rational decimator L / M that take a capture at any accepted rate
// and offset down to the native 2.048 MS/s; include/dabgpu.h, "the tuner".  The reference has no such stage.  Output m is a
// function of its absolute index alone -- q = m M, the input position q div L and the tap row q mod L are integers, the mixer's
// phase is the input index times a 64-bit step, nothing accumulates -- so a stream cut into calls of any lengths, at any run
// geometry, gives the same bytes.
// A workgroup makes `run` consecutive outputs: their input span ((run - 1) M / L + P samples) is loaded once in either of four
// formats, mixed once and staged in LDS as floats, then every lane makes several outputs at a time, each one serial fma chain
// per component over its P taps in tap order.  Two kernels, because what a wave's lanes share differs:
//   L = 1 (1/1, 1/2, 1/3, 1/4, 1/8): ONE tap row, the same for every output.  It is read through uniform loads (one address per wave),
//     four taps each.  Consecutive outputs lie M samples apart; read from a span in input order that is a stride of 8 M bytes for
//     ds_read_b64, at 1/4 a 4-way bank conflict in a 32-lane half.  The span is therefore staged split by residue: input t of
//     the span at [t mod M][t div M].  Tap j of output k is then at [j mod M][k + j div M]: the lanes of a wave, k consecutive,
//     read consecutive eight-byte words of one residue row -- no conflict at any M.  Four outputs per lane.
//   L > 1: consecutive outputs use different rows (row p + M mod L follows row p); the table (at most 512 x 192 floats) stays
//     in global memory, one 16-byte load per four taps and output; the span is staged in input order and output k reads it
//     from floor((p0 + k M) / L) on: 32 consecutive lanes cover 32 M / L consecutive samples, a conflict of degree ceil(M / L)
//     at most (2 at 64/75).  Two outputs per lane.
// The P - 1 samples of history the next call reads are stream_history.hip's.  No atomics, no scratch.
#include "device_common.h"
#include "turn_phase.h"

namespace dabgpu {
namespace {

// input sample r of the call (r < 0: the history, zero in front of it; r >= n is asked for by no output), mixed by the phase
// of its absolute index T + r.  step = 0: the sample's bits.
template <int IF> DEV cf tuner_sample(const TunerArgs &a, long long r)
{
    const int H = a.P - 1;
    cf v = mk(0.f, 0.f);
    if (r >= 0) {
        if (r < a.n) v = load_sample<IF>(a.in, r);
    } else if (r >= -(long long)H) {
        v = a.hist[H + r];
    }
    if (a.step != 0) {
        const cf w = turn_phase((a.T + (unsigned long long)r) * a.step);
        v = mk(fmaf(v.x, w.x, -__fmul_rn(v.y, w.y)), fmaf(v.x, w.y, __fmul_rn(v.y, w.x)));
    }
    return v;
}

constexpr int kDecOut = 4, kRatOut = 2;   // outputs a lane makes at a time

template <int IF, int OF> __global__ __launch_bounds__(256) void tuner_dec_kernel(const TunerArgs a)
{
    __shared__ float2 span[kTunSpan];
    const int M = a.M, P = a.P;
    const long long k0 = (long long)blockIdx.x * a.run;
    const int cnt = (int)min((long long)a.run, a.count - k0);
    const unsigned long long mb = a.m0 + (unsigned long long)k0;
    const long long i_first = (long long)(mb * (unsigned long long)M);
    // input t of the span = input sample i_first - (P/2 - 1) + t, at span[(t mod M) S + t div M]; M S <= kTunSpan (tuner_run_max)
    const int len = (cnt - 1) * M + P;
    const int S = ((len + M - 1) / M) | 1;
    const long long r0 = i_first - (P / 2 - 1) - (long long)a.T;
    for (int t = threadIdx.x; t < len; t += 256) {
        const int d = t / M, res = t - d * M;
        span[res * S + d] = tuner_sample<IF>(a, r0 + t);
    }
    __syncthreads();
    // the one tap row: every lane loads the same sixteen bytes (one address per wave: a broadcast, no gather).  Through the
    // constant address space the compiler reads it with scalar loads instead; measured a few per cent slower
    const float4 *tab = reinterpret_cast<const float4 *>(a.tab);
    for (int kb = 0; kb < cnt; kb += 256 * kDecOut) {
        int k[kDecOut];
        float re[kDecOut], im[kDecOut];
#pragma unroll
        for (int u = 0; u < kDecOut; ++u) {
            k[u] = min(kb + (int)threadIdx.x + 256 * u, cnt - 1);
            re[u] = 0.f;
            im[u] = 0.f;
        }
        // taps 0 ... P - 1 in this order, one fused multiply-add per component and tap, from zero; tap j = d M + res
        int res = 0, row = 0, d = 0;
        for (int j4 = 0; j4 < P / 4; ++j4) {
            const float4 h4 = tab[j4];
            const float h[4] = {h4.x, h4.y, h4.z, h4.w};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
#pragma unroll
                for (int u = 0; u < kDecOut; ++u) {
                    const cf x = span[row + d + k[u]];
                    re[u] = fmaf(h[i], x.x, re[u]);
                    im[u] = fmaf(h[i], x.y, im[u]);
                }
                ++res;
                row += S;
                if (res == M) {
                    res = 0;
                    row = 0;
                    ++d;
                }
            }
        }
#pragma unroll
        for (int u = 0; u < kDecOut; ++u) {
            const int ku = kb + (int)threadIdx.x + 256 * u;
            if (ku < cnt) store_sample<OF>(a.out, k0 + ku, re[u], im[u]);
        }
    }
}

template <int IF, int OF> __global__ __launch_bounds__(256) void tuner_rat_kernel(const TunerArgs a)
{
    __shared__ float2 span[kTunSpan];
    const unsigned L = (unsigned)a.L, M = (unsigned)a.M;
    const int P = a.P;
    const long long k0 = (long long)blockIdx.x * a.run;
    const int cnt = (int)min((long long)a.run, a.count - k0);
    const unsigned long long qb = (a.m0 + (unsigned long long)k0) * (unsigned long long)M;
    const long long i_first = (long long)(qb / L);
    const unsigned p_first = (unsigned)(qb - (unsigned long long)i_first * L);
    // span[t] = input sample i_first - (P/2 - 1) + t; output k of the run starts at t = (p_first + k M) div L
    const int len = min((int)((p_first + (unsigned)(cnt - 1) * M) / L) + P, kTunSpan);
    const long long r0 = i_first - (P / 2 - 1) - (long long)a.T;
    for (int t = threadIdx.x; t < len; t += 256) span[t] = tuner_sample<IF>(a, r0 + t);
    __syncthreads();
    for (int kb = 0; kb < cnt; kb += 256 * kRatOut) {
        int o[kRatOut];
        const float4 *row[kRatOut];
        float re[kRatOut], im[kRatOut];
#pragma unroll
        for (int u = 0; u < kRatOut; ++u) {
            const unsigned q = p_first + (unsigned)min(kb + (int)threadIdx.x + 256 * u, cnt - 1) * M;
            const unsigned i = q / L;
            o[u] = min((int)i, len - P);
            row[u] = reinterpret_cast<const float4 *>(a.tab + (size_t)(q - i * L) * (size_t)P);
            re[u] = 0.f;
            im[u] = 0.f;
        }
        // taps 0 ... P - 1 in this order, one fused multiply-add per component and tap, from zero
        for (int j = 0; j < P; j += 4) {
#pragma unroll
            for (int u = 0; u < kRatOut; ++u) {
                const float4 h4 = row[u][j / 4];
                const float h[4] = {h4.x, h4.y, h4.z, h4.w};
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const cf x = span[o[u] + j + i];
                    re[u] = fmaf(h[i], x.x, re[u]);
                    im[u] = fmaf(h[i], x.y, im[u]);
                }
            }
        }
#pragma unroll
        for (int u = 0; u < kRatOut; ++u) {
            const int ku = kb + (int)threadIdx.x + 256 * u;
            if (ku < cnt) store_sample<OF>(a.out, k0 + ku, re[u], im[u]);
        }
    }
}

template <int IF, int OF> void launch_one(const TunerArgs &a, dim3 grid, hipStream_t s)
{
    if (a.L == 1) DABGPU_LAUNCH((tuner_dec_kernel<IF, OF>), grid, dim3(256), 0, s, a);
    else DABGPU_LAUNCH((tuner_rat_kernel<IF, OF>), grid, dim3(256), 0, s, a);
}
template <int IF> void launch_in(const TunerArgs &a, dim3 grid, hipStream_t s)
{
    if (a.out_fmt == 0) launch_one<IF, 0>(a, grid, s);
    else launch_one<IF, 1>(a, grid, s);
}

}  // namespace

// outputs per workgroup at most: the span of `run` outputs, (run - 1) M / L + 1 + P samples at most in input order and
// M (run + P / M + 1) split by residue, fits kTunSpan
int tuner_run_max(int L, int M, int P)
{
    const int D = (M + L - 1) / L;
    const long long r = (long long)(kTunSpan - P - 2 * D) * L / M;
    return (int)std::max<long long>(1, std::min<long long>(r, kTunMaxRun));
}

// outputs per workgroup: forced (1 ... tuner_run_max), or the largest multiple of 256 up to 1024 that fits
int tuner_run(int L, int M, int P, int forced)
{
    const int mx = tuner_run_max(L, M, P);
    if (forced > 0) return std::min(forced, mx);
    return mx >= 256 ? std::min(1024, mx / 256 * 256) : mx;
}

hipError_t launch_tuner(const TunerArgs &a, hipStream_t s)
{
    if (!a.in || !a.out || !a.hist || !a.tab || a.n < 1 || a.count < 1 || a.in_fmt < 0 || a.in_fmt > 3 ||
        (a.out_fmt != 0 && a.out_fmt != 1))
        return hipErrorInvalidValue;
    // what the kernels rely on: the ratio's and the tap count's ranges, a run whose span fits, and every output's P taps in
    // [T - (P - 1), T + n - 1]
    if (a.L < 1 || a.L > kTunMaxL || a.M < a.L || a.M > 8 * a.L) return hipErrorInvalidValue;
    const int D = (a.M + a.L - 1) / a.L;
    if ((a.P != 32 * D && a.P != 96 * D) || a.P > kTunMaxTaps || (a.L == 1 && a.P % a.M)) return hipErrorInvalidValue;
    if (a.run < 1 || a.run > tuner_run_max(a.L, a.M, a.P)) return hipErrorInvalidValue;
    if (a.T > (1ULL << 50) || a.n > (1LL << 40) || a.m0 > (1ULL << 60)) return hipErrorInvalidValue;
    const auto pos = [&](unsigned long long m) { return (__int128)m * a.M / a.L; };
    const __int128 lo = pos(a.m0) - (a.P / 2 - 1), hi = pos(a.m0 + (unsigned long long)(a.count - 1)) + a.P / 2;
    if (lo < (__int128)a.T - (a.P - 1) || hi > (__int128)a.T + a.n - 1) return hipErrorInvalidValue;
    const long long blocks = (a.count + a.run - 1) / a.run;
    if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    const dim3 grid((unsigned)blocks);
    switch (a.in_fmt) {
    case 0: launch_in<0>(a, grid, s); break;
    case 1: launch_in<1>(a, grid, s); break;
    case 2: launch_in<2>(a, grid, s); break;
    default: launch_in<3>(a, grid, s); break;
    }
    return hipGetLastError();
}

}  // namespace dabgpu
