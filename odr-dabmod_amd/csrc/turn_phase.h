// turn_phase.h -- what the kernels that take or make a sample stream share (sync.hip, channel.hip, clock.hip, tuner.hip,
// spectrum.hip, dpd.hip ...): the load of one sample in any input format, the store of one output sample, and the rotation by
// an integer phase.  Anonymous namespace, as device_common.h.
#pragma once
#include "device_common.h"

namespace dabgpu {
namespace {

// one sample of format FMT (0 = complexf, 1 = s16 pair, 2 = u8 pair: byte - 128, 3 = s8 pair) as fp32
template <int FMT> DEV cf load_sample(const void *base, long long i)
{
    if (FMT == 0) return reinterpret_cast<const float2 *>(base)[i];
    if (FMT == 1) {
        const uint32_t w = reinterpret_cast<const uint32_t *>(base)[i];                    // re in the low half
        return mk((float)(short)(w & 0xffffu), (float)(short)(w >> 16));
    }
    const unsigned w = reinterpret_cast<const uint16_t *>(base)[i];                         // re in the low byte
    if (FMT == 2) return mk((float)((int)(w & 0xffu) - 128), (float)((int)(w >> 8) - 128));
    return mk((float)(signed char)(w & 0xffu), (float)(signed char)(w >> 8));
}
// the same for the capture stages, whose format (complexf or s16) is a kernel argument
DEV cf ld_iq(const void *iq, int fmt, long long i)
{
    if (fmt == 0) return load_sample<0>(iq, i);
    return load_sample<1>(iq, i);
}

// one output sample as an s16 pair: format_kernel's conversion (format_one: saturating, toward zero), without the clip count.
// The counter format_one wants is thrown away: a copy of this function's, or (Count = unsigned &, channel_kernel) one the
// caller's unrolled stores share -- either way the instructions these kernels had with the conversion written out.
template <typename Count = unsigned> DEV uint32_t s16_pair(float re, float im, Count unused = 0)
{
    const int qr = format_one<1>(re, unused), qi = format_one<1>(im, unused);
    return (unsigned)(qr & 0xffff) | ((unsigned)qi << 16);
}
// output sample `at` in format OF (0 = complexf, 1 = s16 pair)
template <int OF> DEV void store_sample(void *out, long long at, float re, float im)
{
    if (OF == 0) reinterpret_cast<float2 *>(out)[at] = mk(re, im);
    else reinterpret_cast<uint32_t *>(out)[at] = s16_pair(re, im);
}

// exp(2 pi j f), f = the upper 32 bits of a 64-bit turn accumulator / 2^32.  Range reduction in integers: the nearest quarter
// turn comes off exactly, what is left (|.| <= 1/8 turn, 30 bits) is rounded to fp32 once (2^-27 half turns: 2.4e-8 rad).
DEV cf turn_phase(unsigned long long acc)
{
    const uint32_t hi = (uint32_t)(acc >> 32);
    const uint32_t q = (hi + 0x20000000u) >> 30;
    const int r = (int)(hi - (q << 30));
    float s, c;
    sincospif((float)r * 4.656612873077393e-10f, &s, &c);               // r 2^-31 half turns
    switch (q & 3u) {
    case 0: return mk(c, s);
    case 1: return mk(-s, c);
    case 2: return mk(-c, -s);
    default: return mk(s, -c);
    }
}
// rint(turns per sample 2^64) as the accumulator's step (|turns| < 1/4: fits the signed conversion)
DEV unsigned long long turn_step(double turns) { return (unsigned long long)(long long)rint(turns * 18446744073709551616.0); }

}  // namespace
}  // namespace dabgpu
