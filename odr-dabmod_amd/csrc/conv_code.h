// conv_code.h -- the channel coding that frontend.hip runs forwards and decode.hip backwards, once: the K = 7 mother code, the
// puncturing tables of one unit (FeUnit) with their lookup, the time interleaver's delay per bit, and the layout of a
// transmission frame's words as rows of one ETI frame each.  Plain C++ for host and device: the kernels run these per lane, a
// host compiler builds them alone (tools/conv_code_check.cpp holds them to the CPU classes of host/Frontend.cpp).
// EN 300 401 11.1 (mother code), 11.2 (puncturing), 12 (time interleaving); ConvEncoder, PuncturingEncoder, TimeInterleaver,
// BlockPartitioner of the reference (src/ConvEncoder.cpp:95-139, src/PuncturingEncoder.cpp:152-196, src/TimeInterleaver.cpp:66-93,
// src/BlockPartitioner.cpp:111-117).
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define CONV_HD __host__ __device__ __forceinline__
#define CONV_UNROLL _Pragma("unroll")
#else
#define CONV_HD inline
#define CONV_UNROLL
#endif

namespace dabgpu {

// One FeUnit per FIC / sub-channel: where its payload lies in the ETI frame, where its punctured bytes go, and the flattened
// puncturing segments -- segment r covers the 4-byte groups g0[r] ... g0[r + 1] - 1 of the mother code's output with pattern
// pat[r], its first kept bit at bit base[r] of the unit's output; entry nseg is the 24-bit tail.
constexpr int kFeCifBytes = 864 * 8;      // one CIF; also the length of the dispersal table
constexpr int kFeHistory = 15;            // frames the time interleaver looks back
struct FeUnit {
    uint32_t in_off, in_bytes;            // payload inside the 6144-byte frame
    uint32_t out_bytes;                   // punctured and padded: the FIC's 288 / 384, or 8 x CU
    uint32_t dst_off;                     // byte offset inside the CIF row (8 x SAD); 0 for the FIC
    int32_t owner;                        // sub-channel index in STC order; -1: the FIC
    uint32_t nseg;
    uint32_t g0[6], base[6], pat[6];      // (4 rules + the tail + the end)
};

// The four code bits of one step.  The reference's register is seven bits wide, the new bit enters at bit 6, and the
// generators 133, 171, 145, 133 (octal) read it as the masks 0x5b, 0x79, 0x65, 0x5b.  Here a window holds the last seven input
// bits oldest first (MSB), the register mirrored, and so are the masks.
constexpr uint32_t kConvGen[4] = {0x6d, 0x4f, 0x53, 0x6d};
CONV_HD uint32_t code_nibble(uint32_t win)
{
    return ((uint32_t)(__builtin_popcount(win & kConvGen[0]) & 1) << 3) | ((uint32_t)(__builtin_popcount(win & kConvGen[1]) & 1) << 2) |
           ((uint32_t)(__builtin_popcount(win & kConvGen[2]) & 1) << 1) | (uint32_t)(__builtin_popcount(win & kConvGen[3]) & 1);
}

// The 32 code bits of one input byte: they depend on the byte and on the six bits before it (the last 14 input bits in `s`,
// oldest first; the window of step k is seven of them).
CONV_HD uint32_t mother_code(uint32_t prev, uint32_t byte)
{
    const uint32_t s = ((prev & 0x3fu) << 8) | byte;
    uint32_t w = 0;
    CONV_UNROLL for (int k = 0; k < 8; ++k) w = (w << 4) | code_nibble((s >> (7 - k)) & 0x7fu);
    return w;
}

// The decoder's side of the same step.  State = the last six input bits, newest at bit 0; the step into state s with oldest
// bit o has the window (o << 6) | s.  This is the nibble expected on the branch with o = 0; every generator reads the oldest
// bit, so the branch with o = 1 expects the complement.
CONV_HD uint32_t branch_nibble(uint32_t state) { return code_nibble(state); }

// the bits of w that the pattern keeps, in order, MSB first, right-aligned
CONV_HD uint32_t keep_bits(uint32_t w, uint32_t pattern)
{
    uint32_t acc = 0;
    CONV_UNROLL for (int b = 31; b >= 0; --b)
        if ((pattern >> b) & 1u) acc = (acc << 1) | ((w >> b) & 1u);
    return acc;
}
// its inverse: the `kept` bits of acc (right-aligned, first bit highest) at the places the pattern keeps, MSB first
CONV_HD uint32_t spread_bits(uint32_t acc, uint32_t pattern, uint32_t kept)
{
    uint32_t w = 0, n = kept;
    CONV_UNROLL for (int b = 31; b >= 0; --b)
        if ((pattern >> b) & 1u) w |= ((acc >> --n) & 1u) << b;
    return w;
}

// 4-byte group i of the unit's mother-code output (group in_bytes is the tail): the pattern it is punctured with, how many
// bits that keeps, and where the first of them lies in the unit's punctured bit stream
struct FeSegment { uint32_t pattern, kept, at; };
CONV_HD FeSegment fe_segment(const FeUnit &u, uint32_t i)
{
    uint32_t r = 0;
    while (r < u.nseg && i >= u.g0[r + 1]) ++r;
    const uint32_t pattern = u.pat[r], kept = (uint32_t)__builtin_popcount(pattern);
    return {pattern, kept, u.base[r] + (i - u.g0[r]) * kept};
}

// Bit 0x80 >> b of an even byte comes from the frame delayed by {0,8,4,12,2,10,6,14}[b], of an odd byte by
// {1,9,5,13,3,11,7,15}[b]: as the mask a delay has on a little-endian dword of two (even, odd) byte pairs.
CONV_HD uint32_t delay_mask(int d)
{
    // b = the 3-bit reversal of d >> 1
    const int h = d >> 1, b = ((h & 1) << 2) | (h & 2) | (h >> 2);
    const uint32_t m = 0x80u >> b;
    return (d & 1) ? m * 0x01000100u : m * 0x00010001u;
}

// Word w of a transmission frame (the FICs of its `cifs` ETI frames, then their CIFs) as word `at` of row k, a row being one
// ETI frame's FIC (fic_row words) followed by its CIF (cif_row words)
struct RowWord { uint32_t k, at; };
CONV_HD RowWord tf_row_word(uint32_t w, uint32_t cifs, uint32_t fic_row, uint32_t cif_row)
{
    const uint32_t fic_words = cifs * fic_row;
    if (w < fic_words) return {w / fic_row, w % fic_row};
    return {(w - fic_words) / cif_row, fic_row + (w - fic_words) % cif_row};
}

}  // namespace dabgpu
