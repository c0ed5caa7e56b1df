// turn_phase.h -- what the kernels that take a sample stream and rotate it share (sync.hip, channel.hip): the load of one
// sample in either input format and the rotation by an integer phase.  Anonymous namespace, as device_common.h.
#pragma once
#include "device_common.h"

namespace dabgpu {
namespace {

DEV cf ld_iq(const void *iq, int fmt, long long i)
{
    if (fmt == 0) return reinterpret_cast<const float2 *>(iq)[i];
    const uint32_t w = reinterpret_cast<const uint32_t *>(iq)[i];       // s16 pair: re in the low half
    return mk((float)(short)(w & 0xffffu), (float)(short)(w >> 16));
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
