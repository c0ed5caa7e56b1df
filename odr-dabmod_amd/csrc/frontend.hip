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
// Integer work on independent bits: the same bytes as the CPU classes of host/Frontend.cpp.  The code itself -- mother_code,
// keep_bits, the segment lookup, delay_mask, the frame's words as rows -- is conv_code.h's, shared with decode.hip.
#include "dabgpu_internal.h"

namespace dabgpu {

namespace {

constexpr int kFeThreads = 256;
constexpr int kFeRowWords = kFeCifBytes / 4;

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
        const FeSegment g = fe_segment(u, i);
        if (!g.kept) continue;
        const unsigned long long v = (unsigned long long)keep_bits(w, g.pattern) << (64 - g.kept - (g.at & 31u));
        const uint32_t hi = (uint32_t)(v >> 32), lo = (uint32_t)v;
        if (hi) atomicOr(&s_out[g.at >> 5], hi);
        if (lo) atomicOr(&s_out[(g.at >> 5) + 1], lo);
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

__global__ __launch_bounds__(kFeThreads) void fe_assemble_kernel(FeArgs a, size_t total)
{
    const size_t idx = (size_t)blockIdx.x * kFeThreads + threadIdx.x;
    if (idx >= total) return;
    const uint32_t fic_row = (uint32_t)a.fic_out / 4, tf_words = (uint32_t)a.cifs * (fic_row + kFeRowWords);
    const size_t tf = idx / tf_words;
    // the word's ETI frame of the call and its place there: in the frame's FIC, or behind it in its CIF.  (The FIC branch pays
    // a division for its row that it could do without: the FICs lie in frame order, word w of them at tf * fic_words + w.)
    const RowWord r = tf_row_word((uint32_t)(idx % tf_words), (uint32_t)a.cifs, fic_row, kFeRowWords);
    const size_t frame = tf * a.cifs + r.k;
    uint32_t v;
    if (r.at < fic_row) {
        v = ((const uint32_t *)a.fic)[frame * fic_row + r.at];
    } else {
        const uint32_t jj = r.at - fic_row;
        if (a.owner[jj >> 1] < 0) {
            v = ((const uint32_t *)a.prbs)[jj];
        } else {
            // row of this CIF's own frame; a sub-channel starts on an even byte, so the CIF's byte parity is its parity
            const uint32_t *row = (const uint32_t *)a.hist + ((size_t)kFeHistory + frame) * kFeRowWords + jj;
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
