// carriers.hip -- the integer front of the chain as ONE kernel beside the frame kernel: coded bits -> the carriers of a
// transmission frame, i.e. the sub-graph cifMap -> cifFreq -> cifDiff (+ cifRef) -> cifSig (+ NullSymbol / TII) [-> cifCicEq] of
// src/DabModulator.cpp:385-399.  What dabgpu_carriers_process returns and what a chain call runs first when the CIC
// equaliser is on (the from-carriers chain does the rest).
#include "device_common.h"

namespace dabgpu {
namespace {

// cos / sin of p * 45 degrees as {-1, 0, +1} codes, (codes >> 2p) & 3 = value + 1 (the frame kernel's unit vectors, tf_kernel.h)
constexpr unsigned kUnitCodes = 0x901Au;
constexpr int kCarBitWords = 7200;   // coded bits of one transmission frame in dwords: 75 x 384 B (Mode I), the largest
constexpr int kCarSyms = 160;        // >= nb_symbols (153 in Mode III)

// exp(i p pi / 4) without its modulus: components 0 / +-1 (the magnitude table carries sqrt(1/2) on the diagonal states)
DEV cf unit_eighth(unsigned p)
{
    const float cx = (float)((int)((kUnitCodes >> (2u * (p & 7u))) & 3u) - 1);
    const float cy = (float)((int)((kUnitCodes >> (2u * ((p + 6u) & 7u))) & 3u) - 1);
    return mk(cx, cy);
}

// One lane per carrier POSITION k (the frequency interleaver's output order = the order of the output), walking the
// frame's symbols with the carrier's differential phase in a register; the 64 lanes of a wave are 64 adjacent carriers, so
// every store instruction writes 512 contiguous bytes.  A workgroup stages the frame's coded bits (at most 28.8 kB) in LDS
// once; the symbol loop then has no global load in it -- nothing that waits for the stores in flight.
//
// A carrier of symbol s >= 1 is mag[s - 1] * u8[phase]: the 3-bit phase (in eighths) is 2 q + (s - 1), q the running sum of
// quarter turns -- the phase reference's, plus (I, Q) = 00 -> 0, 10 -> 1, 11 -> 2, 01 -> 3 per data block (every QPSK point
// also turns by one eighth: the s - 1) --, and mag the modulus the reference's fp32 product chain leaves after s - 1
// multiplications (Tables::mag, formed on the host with the reference's operations).  Bit for bit the
// reference's QpskSymbolMapper -> FrequencyInterleaver -> DifferentialModulator.
// Symbol 0 is the null symbol: zeros, or on a frame that carries TII what tii_kernel forms from the phase reference symbol.
// cic != nullptr: every carrier times cic[k], a second fp32 multiplication as in CicEqualizer::process (out[i] = in[i] * myFilter[j]).
__global__ __launch_bounds__(256) void carriers_from_bits_kernel(CarrierArgs a)
{
#pragma clang fp contract(off)
    __shared__ uint32_t bits_l[kCarBitWords];
    __shared__ float mag_l[kCarSyms];
    const int K = a.g.K, nsym = a.g.nb_symbols + 1;
    const int blocks_per_frame = (K + 255) / 256;
    const int frame = (int)blockIdx.x / blocks_per_frame;
    const int k = ((int)blockIdx.x - frame * blocks_per_frame) * 256 + (int)threadIdx.x;
    if (frame >= a.n_frames) return;
    const int block_bytes = K / 4;                                   // one data block: K/8 bytes of I bits, K/8 of Q bits
    const int words = (a.g.nb_symbols - 1) * block_bytes / 4;        // <= kCarBitWords
    const uint32_t *src = reinterpret_cast<const uint32_t *>(a.bits + (size_t)frame * (size_t)(a.g.nb_symbols - 1) * (size_t)block_bytes);
    for (int i = threadIdx.x; i < words; i += 256) bits_l[i] = src[i];
    for (int i = threadIdx.x; i < a.g.nb_symbols; i += 256) mag_l[i] = a.t.mag[i];
    __syncthreads();
    if (k >= K) return;

    const float f = a.cic ? a.cic[k] : 1.0f;
    const bool eq = a.cic != nullptr;
    auto put = [&](int s, cf y) __attribute__((always_inline)) {
        if (eq) y = mk(y.x * f, y.y * f);
        a.out[((size_t)frame * (size_t)nsym + (size_t)s) * (size_t)K + (size_t)k] = y;
    };

    unsigned q = (unsigned)a.t.phase_q[k] & 3u;
    // symbol 0: TII on every other frame of the stream (TII::m_insert, src/TII.cpp:226-242; gather form of :172-211)
    cf y0 = mk(0.f, 0.f);
    if (a.acp != nullptr && (((frame & 1) == 0) == (a.tii_insert0 != 0))) {
        if (a.acp[k]) y0 = unit_eighth(2u * q);
        else if (k > 0 && a.acp[k - 1]) y0 = unit_eighth(2u * (a.tii_old_variant ? q : ((unsigned)a.t.phase_q[k - 1] & 3u)));
    }
    put(0, y0);
    // symbol 1: the phase reference
    {
        const cf u = unit_eighth(2u * q);
        const float mg = mag_l[0];
        put(1, mk(u.x * mg, u.y * mg));
    }
    // the carrier's bit in a data block: bit n of the I half, bit n of the Q half (MSB first), n its index before interleaving
    const int n = a.t.src_carrier[k];
    const uint8_t *ib = reinterpret_cast<const uint8_t *>(bits_l) + (n >> 3);
    const int qoff = K >> 3;
    const unsigned sh = 7u - ((unsigned)n & 7u);
    for (int s = 2; s < nsym; ++s) {
        const uint8_t *blk = ib + (s - 2) * block_bytes;
        const unsigned I = ((unsigned)blk[0] >> sh) & 1u, Q = ((unsigned)blk[qoff] >> sh) & 1u;
        q = (q + ((I ^ Q) | (Q << 1))) & 3u;
        const cf u = unit_eighth(2u * q + (unsigned)(s - 1));
        const float mg = mag_l[s - 1];
        put(s, mk(u.x * mg, u.y * mg));
    }
}

}  // namespace

hipError_t launch_carriers_from_bits(const CarrierArgs &a, hipStream_t s)
{
    if (a.n_frames <= 0) return hipSuccess;
    if ((a.g.nb_symbols - 1) * (a.g.K / 4) > 4 * kCarBitWords || a.g.nb_symbols > kCarSyms) return hipErrorInvalidValue;
    const unsigned blocks = (unsigned)a.n_frames * (unsigned)((a.g.K + 255) / 256);
    DABGPU_LAUNCH(carriers_from_bits_kernel, dim3(blocks), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace dabgpu
