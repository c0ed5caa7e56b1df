// frontend.hip -- the front-end on the device: raw ETI(NI) frames -> the chain's coded bits.
// Two launches per call, for any number of ETI frames:
//   fe_encode_kernel    one workgroup per (ETI frame, unit); a unit is the FIC or one sub-channel.  Energy dispersal
//                       (PrbsGenerator, src/PrbsGenerator.cpp:112-123), the K = 7 mother code (ConvEncoder,
//                       src/ConvEncoder.cpp:95-139) and puncturing (PuncturingEncoder, src/PuncturingEncoder.cpp:152-196).
//                       The seed form of the launch (FeArgs::unit0 = 1, FeArgs::row0 below kFeHistory) runs the sub-channel
//                       units alone and leaves them in history rows row0 ...: the state in front of a frame, from the frames
//                       before it, with no FIC, no assembly and no shift behind it.
//   fe_assemble_kernel  one lane per output dword: the 16-frame time interleaver (src/TimeInterleaver.cpp:66-93), the CIF over
//                       its padding (FrameMultiplexer, src/FrameMultiplexer.cpp:58-92) and the BlockPartitioner layout
//                       (src/BlockPartitioner.cpp:111-117).
// Integer work on independent bits: the same bytes as the CPU classes of host/Frontend.cpp.
#include "dabgpu_internal.h"

namespace dabgpu {

namespace {

constexpr int kFeThreads = 256;
constexpr int kFeRowWords = kFeCifBytes / 4;

// The 32 code bits of one input byte: they depend on the byte and on the six bits before it.  The reference's register is
// seven bits wide, the new bit enters at bit 6, and the generators 133, 171, 145, 133 (octal) read it as the masks 0x5b, 0x79,
// 0x65, 0x5b.  Here the last 14 input bits sit in `s` oldest first (MSB), so the window of step k is the register mirrored,
// and so are the masks: 0x6d, 0x4f, 0x53, 0x6d.
__device__ __forceinline__ uint32_t mother_code(uint32_t prev, uint32_t byte)
{
    const uint32_t s = ((prev & 0x3fu) << 8) | byte;
    uint32_t w = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const uint32_t win = (s >> (7 - k)) & 0x7fu;
        w = (w << 4) | ((__popc(win & 0x6du) & 1u) << 3) | ((__popc(win & 0x4fu) & 1u) << 2) | ((__popc(win & 0x53u) & 1u) << 1) |
            (__popc(win & 0x6du) & 1u);
    }
    return w;
}

// the bits of w that the pattern keeps, in order, MSB first, right-aligned
__device__ __forceinline__ uint32_t keep_bits(uint32_t w, uint32_t pattern)
{
    uint32_t acc = 0;
#pragma unroll
    for (int b = 31; b >= 0; --b)
        if ((pattern >> b) & 1u) acc = (acc << 1) | ((w >> b) & 1u);
    return acc;
}

__global__ __launch_bounds__(kFeThreads) void fe_encode_kernel(FeArgs a)
{
    // the dispersed payload as bytes; the unit's output as a bit stream in words whose MSB is the first bit
    __shared__ uint8_t s_in[6144];
    __shared__ uint32_t s_out[kFeRowWords + 1];
    // (unit0 = 1: the FIC, unit 0, is left out -- the seed form)
    const int per_frame = a.n_units - a.unit0, f = blockIdx.x / per_frame;
    const FeUnit &u = a.units[a.unit0 + blockIdx.x % per_frame];
    const uint32_t in_bytes = u.in_bytes, out_words = u.out_bytes / 4;
    const uint8_t *src = a.eti + (size_t)f * 6144 + u.in_off;
    for (uint32_t i = threadIdx.x; i < in_bytes; i += kFeThreads) s_in[i] = src[i] ^ a.prbs[i];
    for (uint32_t d = threadIdx.x; d <= out_words; d += kFeThreads) s_out[d] = 0;
    __syncthreads();
    // one lane per 4-byte group of the mother code's output = per input byte; group in_bytes is the flush: six zero bits,
    // 24 code bits under the tail rule (the last segment: its pattern is left-aligned in 32 bits)
    for (uint32_t i = threadIdx.x; i <= in_bytes; i += kFeThreads) {
        const uint32_t byte = i < in_bytes ? s_in[i] : 0u, prev = i ? s_in[i - 1] : 0u;
        const uint32_t w = mother_code(prev, byte);
        uint32_t r = 0;
        while (r < u.nseg && i >= u.g0[r + 1]) ++r;
        const uint32_t pattern = u.pat[r], kept = __popc(pattern);
        if (!kept) continue;
        const uint32_t at = u.base[r] + (i - u.g0[r]) * kept;
        const unsigned long long v = (unsigned long long)keep_bits(w, pattern) << (64 - kept - (at & 31u));
        const uint32_t hi = (uint32_t)(v >> 32), lo = (uint32_t)v;
        if (hi) atomicOr(&s_out[at >> 5], hi);
        if (lo) atomicOr(&s_out[(at >> 5) + 1], lo);
    }
    __syncthreads();
    // (what lies behind the last kept bit is the zero padding up to 8 x CU)
    if (u.owner < 0) {
        uint32_t *dst = (uint32_t *)(a.fic + (size_t)f * a.fic_out);
        for (uint32_t d = threadIdx.x; d < out_words; d += kFeThreads) dst[d] = __builtin_bswap32(s_out[d]);
    } else {
        // row row0 + f of the history (15 + f in a call that produces output), at the sub-channel's place in the CIF; a
        // capacity unit that a later sub-channel of the STC list covers as well is that one's (the reference's memcpy order:
        // the last one wins)
        uint32_t *dst = (uint32_t *)(a.hist + (size_t)(a.row0 + f) * kFeCifBytes + u.dst_off);
        const int16_t *own = a.owner + (u.dst_off >> 3);
        for (uint32_t d = threadIdx.x; d < out_words; d += kFeThreads)
            if (own[d >> 1] == u.owner) dst[d] = __builtin_bswap32(s_out[d]);
    }
}

// Bit 0x80 >> b of an even byte comes from the frame delayed by {0,8,4,12,2,10,6,14}[b], of an odd byte by
// {1,9,5,13,3,11,7,15}[b]: as the mask a delay has on a little-endian dword of two (even, odd) byte pairs.
__device__ __forceinline__ uint32_t delay_mask(int d)
{
    // b = the 3-bit reversal of d >> 1
    const int h = d >> 1, b = ((h & 1) << 2) | (h & 2) | (h >> 2);
    const uint32_t m = 0x80u >> b;
    return (d & 1) ? m * 0x01000100u : m * 0x00010001u;
}

__global__ __launch_bounds__(kFeThreads) void fe_assemble_kernel(FeArgs a, size_t total)
{
    const size_t idx = (size_t)blockIdx.x * kFeThreads + threadIdx.x;
    if (idx >= total) return;
    const uint32_t fic_words = (uint32_t)(a.cifs * a.fic_out) / 4, tf_words = fic_words + (uint32_t)a.cifs * kFeRowWords;
    const size_t tf = idx / tf_words;
    const uint32_t w = (uint32_t)(idx % tf_words);
    uint32_t v;
    if (w < fic_words) {
        v = ((const uint32_t *)a.fic)[tf * fic_words + w];
    } else {
        const uint32_t j = w - fic_words, cif = j / kFeRowWords, jj = j % kFeRowWords;
        if (a.owner[jj >> 1] < 0) {
            v = ((const uint32_t *)a.prbs)[jj];
        } else {
            // row of this CIF's own frame; a sub-channel starts on an even byte, so the CIF's byte parity is its parity
            const uint32_t *row = (const uint32_t *)a.hist + ((size_t)kFeHistory + tf * a.cifs + cif) * kFeRowWords + jj;
            v = 0;
#pragma unroll
            for (int d = 0; d < 16; ++d) v |= row[-(ptrdiff_t)d * kFeRowWords] & delay_mask(d);
        }
    }
    ((uint32_t *)a.out)[idx] = v;
}

}  // namespace

hipError_t launch_fe_encode(const FeArgs &a, hipStream_t s)
{
    // (the rows a launch may write: the history and the call's own in the ordinary form, the history alone in the seed form)
    if (a.unit0 < 0 || a.unit0 > 1 || a.row0 < 0 || (a.unit0 ? a.row0 + a.n_eti > kFeHistory : a.row0 != kFeHistory))
        return hipErrorInvalidValue;
    if (a.n_eti <= 0 || a.n_units - a.unit0 <= 0) return hipSuccess;
    DABGPU_LAUNCH(fe_encode_kernel, dim3((unsigned)a.n_eti * (unsigned)(a.n_units - a.unit0)), dim3(kFeThreads), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_fe_assemble(const FeArgs &a, hipStream_t s)
{
    if (a.n_eti <= 0) return hipSuccess;
    const size_t total = (size_t)a.n_eti * (size_t)(a.fic_out + kFeCifBytes) / 4;
    DABGPU_LAUNCH(fe_assemble_kernel, dim3((unsigned)((total + kFeThreads - 1) / kFeThreads)), dim3(kFeThreads), 0, s, a, total);
    return hipGetLastError();
}

}  // namespace dabgpu
