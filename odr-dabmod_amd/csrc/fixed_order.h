// fixed_order.h -- what the kernels that must repeat bit for bit share (sync.hip, tii_scan.hip, cir.hip; through rx_symbols.h
// demod.hip and the estimator of clock.hip): workgroup sums and searches in a FIXED order -- the lane's own terms, an xor
// butterfly inside the wave, the waves in wave order through LDS; ties go to the first index -- the phase reference symbol's
// quarter turns, which bins carry a carrier, and the float64 twiddle.  Anonymous namespace, as device_common.h.
#pragma once
#include "device_common.h"

namespace dabgpu {
namespace {

DEV cf mul_quarter(cf z, unsigned q)                                    // z i^q
{
    switch (q & 3u) {
    case 0: return z;
    case 1: return mk(-z.y, z.x);
    case 2: return mk(-z.x, -z.y);
    default: return mk(z.y, -z.x);
    }
}

// ---- workgroup reductions in a fixed order: butterfly over the WL lanes of a wave, then the NW waves in wave order ----------
template <int WL, typename V> DEV V wave_sum_w(V x)
{
#pragma unroll
    for (int off = WL / 2; off >= 1; off >>= 1) x += __shfl_xor(x, off, WL);
    return x;
}
template <int NW, int WL, typename V> DEV V group_sum(V x, V *red, int t)
{
    x = wave_sum_w<WL>(x);
    if ((t & 63) == 0) red[t >> 6] = x;
    lds_barrier();
    V s = red[0];
#pragma unroll
    for (int w = 1; w < NW; ++w) s += red[w];
    lds_barrier();
    return s;
}
// the first index of the extreme value: MAX (largest) or the smallest; (v, i) pairs, a lower index wins a tie
template <bool MAX, typename V> DEV bool better(V v, int i, V v0, int i0)
{
    return (MAX ? v > v0 : v < v0) || (v == v0 && i < i0);
}
template <bool MAX, int NW, int WL, typename V> DEV void group_arg(V &v, int &i, V *red_v, int *red_i, int t)
{
#pragma unroll
    for (int off = WL / 2; off >= 1; off >>= 1) {
        const V ov = __shfl_xor(v, off, WL);
        const int oi = __shfl_xor(i, off, WL);
        if (better<MAX>(ov, oi, v, i)) { v = ov; i = oi; }
    }
    if ((t & 63) == 0) { red_v[t >> 6] = v; red_i[t >> 6] = i; }
    lds_barrier();
    v = red_v[0]; i = red_i[0];
#pragma unroll
    for (int w = 1; w < NW; ++w)
        if (better<MAX>(red_v[w], red_i[w], v, i)) { v = red_v[w]; i = red_i[w]; }
    lds_barrier();
}

// position of carrier k (k = 1 ... K/2, -K/2 ... -1) in Tables::phase_q: the frame kernel's order, positive carriers first
template <int K> DEV int carrier_pos(int k) { return k > 0 ? k - 1 : k + K; }
// carrier of bin b of an N-point transform, and whether it is occupied (k = -K/2 ... -1, 1 ... K/2)
DEV int bin_carrier(int b, int N) { return b <= N / 2 ? b : b - N; }
DEV bool carrier_occupied(int k, int K) { return k != 0 && k >= -K / 2 && k <= K / 2; }
// e^{-j 2 pi m / N} in float64 (sincospi of an exact argument): the twiddle of the float64 transforms
DEV double2 twiddle64(int m, int N)
{
    double sn, cs;
    sincospi(-2.0 * (double)m / (double)N, &sn, &cs);
    return make_double2(cs, sn);
}

}  // namespace
}  // namespace dabgpu
