// decode.hip -- the channel decoder on the device: the chain's coded bits -> the ETI payload.  frontend.hip backwards, from the
// tables dabgpu_frontend_configure uploads (FeUnit, the dispersal sequence) and the code of conv_code.h.  The reference has no
// receiver: nothing here replaces a class of its flowgraph.  Two launches per call, for either metric width:
//   dec_rows_kernel    one lane per input dword: the transmission frame layout (the FICs of its ETI frames, then their CIFs)
//                      into rows of one ETI frame each, punctured FIC | CIF, behind the fifteen rows of history.
//   dec_decode_kernel  one wave per (output ETI frame, unit).  The time interleaver undone (delay_mask forward in time: 16 rows
//                      OR-ed per dword), depuncturing into one byte per trellis step (received nibble | transmitted mask << 4),
//                      the K = 7 Viterbi decoder with lane = state, traceback, energy dispersal.
// Hard decisions, Hamming metrics in uint32, no normalisation.  The rules a CPU model has to follow to give the same bits
// (tests/decode_model.py): state 0 starts at 0, every other state at 1 << 24; of the two predecessors of a state the one whose
// oldest bit is 0 survives unless the other's metric is strictly smaller; traceback starts at state 0 behind the tail.
// Predecessor metrics come through ds_bpermute (two per step): DESIGN.md 4.10 says why.
//
// The soft decoder (dabgpu_decode_soft*): the same two launches on int8 metrics, one per coded bit (soft > 0: the bit is more
// likely 1; 0 says nothing; -128 counts with magnitude 128), eight bytes where the hard decoder has one.
//   dec_soft_rows_kernel    one lane per dword of softs, the same index rule on rows eight times as long.
//   dec_soft_decode_kernel  one wave per (output, unit), lane = state.  The unit's PUNCTURED softs are staged in LDS (at most
//                           864 CU x 64 = 55 296 B; the depunctured ones, four bytes per step, would not fit), the time
//                           interleaver undone by a byte gather over sixteen rows.  Depuncturing happens per 64-step chunk:
//                           lane k forms the four softs of step 64 c + k (0 where the pattern drops the bit) in one dword and
//                           their magnitudes' sum, and the step loop reads both by v_readlane.
// Metric: with e_i the branch's expected bit and r_i the soft, cost = sum max(0, (1 - 2 e_i) r_i) = (sum |r_i| + sum (1 - 2 e_i)
// r_i) / 2 -- one signed 4 x int8 dot product per state and the step's scalar total; the complementary branch costs total - cost.
// State 0 starts at 0, every other state at 1 << 30; uint32 without normalisation (at most 512 per step, fewer than 48 294
// steps).  Behind the traceback the decoded bits are encoded again, one lane per 4-byte group, against the softs in LDS: the
// contradicting bits, their magnitudes (= the final metric), the erasures.
// The trellis walk is written once (dec_forward, dec_traceback, dec_disperse): the two kernels differ in what a lane prepares
// per 64-step chunk and in the two branch costs of a step.
#include "dabgpu_internal.h"

namespace dabgpu {

namespace {

constexpr int kDecRowWords = kFeCifBytes / 4;

// the dwords of `bytes` coded bytes at WIDTH metric bytes per coded byte: 1 (hard, the bits packed) or 8 (soft, one per bit)
template <int WIDTH> __device__ __forceinline__ uint32_t metric_words(uint32_t bytes) { return WIDTH == 1 ? bytes / 4 : (WIDTH / 4) * bytes; }

template <int WIDTH, typename Args> __device__ __forceinline__ void dec_rows_body(const Args &a, size_t total)
{
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const uint32_t fic_row = metric_words<WIDTH>((uint32_t)a.fic_out), cif_row = metric_words<WIDTH>(kFeCifBytes);
    const uint32_t tf_words = (uint32_t)a.cifs * fic_row + (uint32_t)a.cifs * cif_row, row_words = fic_row + cif_row;
    const size_t tf = idx / tf_words;
    const RowWord r = tf_row_word((uint32_t)(idx % tf_words), (uint32_t)a.cifs, fic_row, cif_row);
    ((uint32_t *)a.rows)[((size_t)kFeHistory + tf * a.cifs + r.k) * row_words + r.at] = ((const uint32_t *)a.in)[idx];
}
__global__ __launch_bounds__(256) void dec_rows_kernel(DecArgs a, size_t total) { dec_rows_body<1>(a, total); }
__global__ __launch_bounds__(256) void dec_soft_rows_kernel(DecSoftArgs a, size_t total) { dec_rows_body<8>(a, total); }

// ---- What the two decode kernels share.  One wave per (output f, unit), lane = state.
// the lead-in: an output before the start of the stream (f < a.first_valid) is not decoded, its record is zero.  (The test
// and the return stay in the kernel: behind a function, the store would stand in front of every read of the unit.)
template <typename Stats> __device__ __forceinline__ void dec_no_output(Stats *st) { if (threadIdx.x == 0) *st = Stats{}; }

// The forward pass over T steps, 64 at a time; returns the final metric of state 0.  State = the last six input bits, newest
// at bit 0, so the predecessors of a state are lane >> 1 with oldest bit 0 and 32 + (lane >> 1) with oldest bit 1.
//   prepare(c)      what this lane holds of chunk c (of step 64 c + lane), read by v_readlane in the step loop
//   costs(held, k)  the costs of the two branches into this lane's state at step k of the chunk, oldest bit 0 and 1
// `start`: the metric of every state but 0.  Lane k keeps the survivor word of step k; 64 of them leave in one coalesced store.
struct DecCosts { uint32_t c0, c1; };
template <typename Prepare, typename Costs>
__device__ __forceinline__ uint32_t dec_forward(unsigned long long *surv, uint32_t T, uint32_t start, Prepare prepare, Costs costs)
{
    const int lane = threadIdx.x;
    const int from0 = (lane >> 1) * 4, from1 = (32 + (lane >> 1)) * 4;
    uint32_t metric = lane ? start : 0u;
    const uint32_t chunks = (T + 63) / 64;
    for (uint32_t c = 0; c < chunks; ++c) {
        const auto held = prepare(c);
        const int nk = (int)min(64u, T - c * 64);
        unsigned long long mine = 0;
        for (int k = 0; k < nk; ++k) {
            const DecCosts b = costs(held, k);
            const uint32_t a0 = (uint32_t)__builtin_amdgcn_ds_bpermute(from0, (int)metric) + b.c0;
            const uint32_t a1 = (uint32_t)__builtin_amdgcn_ds_bpermute(from1, (int)metric) + b.c1;
            const bool other = a1 < a0;
            metric = other ? a1 : a0;
            const unsigned long long word = __ballot(other);
            if (lane == k) mine = word;                  // (lane k keeps step k's word)
        }
        surv[c * 64 + lane] = mine;                      // 512 coalesced bytes
    }
    return (uint32_t)__builtin_amdgcn_readlane((int)metric, 0);
}

// Traceback from state 0 behind the tail into dec[in_bytes]: the state in a scalar, the words of 64 steps one per lane (each
// lane reads back the very word it stored); bit k of `bits` is the input bit of step 64 c + k
__device__ __forceinline__ void dec_traceback(const unsigned long long *surv, uint32_t T, uint32_t in_bytes, uint8_t *dec)
{
    const int lane = threadIdx.x;
    uint32_t state = 0;
    for (uint32_t c = (T + 63) / 64; c-- > 0;) {
        const unsigned long long mine = surv[c * 64 + lane];
        const int nk = (int)min(64u, T - c * 64);
        unsigned long long bits = 0;
        for (int k = nk - 1; k >= 0; --k) {
            const unsigned long long word = ((unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(mine >> 32), k) << 32) |
                                            (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)mine, k);
            bits |= (unsigned long long)(state & 1u) << k;
            state = ((uint32_t)((word >> state) & 1u) << 5) | (state >> 1);
        }
        // eight payload bytes, first bit highest (the tail's six steps lie behind byte in_bytes - 1)
        const uint32_t at = c * 8 + lane;
        if (lane < 8 && at < in_bytes) dec[at] = (uint8_t)(__brev((uint32_t)(bits >> (8 * (lane & 7))) & 0xffu) >> 24);
    }
    __syncthreads();
}

// Energy dispersal, the payload at its place in the frame; returns this lane's share of the count against the reference
template <typename Args>
__device__ __forceinline__ uint32_t dec_disperse(const Args &a, int f, uint32_t in_off, uint32_t in_bytes, const uint8_t *dec)
{
    uint8_t *out = a.out + (size_t)f * 6144 + in_off;
    const uint8_t *ref = a.ref ? a.ref + (size_t)f * 6144 + in_off : nullptr;
    uint32_t errors = 0;
    for (uint32_t i = threadIdx.x; i < in_bytes; i += kDecThreads) {
        const uint8_t v = dec[i] ^ a.prbs[i];
        out[i] = v;
        if (ref) errors += __popc((uint32_t)(v ^ ref[i]));
    }
    return errors;
}

__global__ __launch_bounds__(kDecThreads) void dec_decode_kernel(DecArgs a)
{
    // the unit's punctured bits as a stream in words whose MSB is the first bit (later: the decoded bytes); one byte per step,
    // as many as the layout's longest unit has (a.lds_bytes: the launch sizes the workgroup's LDS by it)
    __shared__ uint32_t s_pun[kDecRowWords + 2];
    extern __shared__ uint32_t s_sym[];
    const int lane = threadIdx.x;
    const int f = blockIdx.x / a.n_units, ui = blockIdx.x % a.n_units;
    const FeUnit &u = a.units[ui];
    DecUnitStats *st = a.stats + (size_t)f * a.n_units + ui;
    if (f < a.first_valid) return dec_no_output(st);
    const uint32_t in_bytes = u.in_bytes, out_words = u.out_bytes / 4;
    const uint32_t row_words = (uint32_t)a.fic_out / 4 + kDecRowWords;
    const uint32_t T = 8 * in_bytes + 6;

    // ---- the unit's punctured bytes of output frame f: the FIC from row f, a sub-channel through the time interleaver
    const uint32_t *row = (const uint32_t *)a.rows + (size_t)f * row_words;
    if (u.owner < 0) {
        for (uint32_t d = lane; d < out_words; d += kDecThreads) s_pun[d] = __builtin_bswap32(row[d]);
    } else {
        const uint32_t *src = row + (uint32_t)a.fic_out / 4 + u.dst_off / 4;
        for (uint32_t d = lane; d < out_words; d += kDecThreads) {
            uint32_t v = 0;
#pragma unroll
            for (int k = 0; k < 16; ++k) v |= src[(size_t)k * row_words + d] & delay_mask(k);
            s_pun[d] = __builtin_bswap32(v);
        }
    }
    if (lane < 2) s_pun[out_words + lane] = 0;
    __syncthreads();

    // ---- depuncture: one lane per 4-byte group of the mother code's output (8 steps); group in_bytes is the tail
    for (uint32_t i = lane; i <= in_bytes; i += kDecThreads) {
        const FeSegment g = fe_segment(u, i);
        uint32_t w = 0;
        if (g.kept) {
            const unsigned long long v = ((unsigned long long)s_pun[g.at >> 5] << 32) | s_pun[(g.at >> 5) + 1];
            w = spread_bits((uint32_t)((v << (g.at & 31u)) >> (64 - g.kept)), g.pattern, g.kept);
        }
        uint32_t lo = 0, hi = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            lo |= (((w >> (28 - 4 * k)) & 0xfu) | (((g.pattern >> (28 - 4 * k)) & 0xfu) << 4)) << (8 * k);
            hi |= (((w >> (12 - 4 * k)) & 0xfu) | (((g.pattern >> (12 - 4 * k)) & 0xfu) << 4)) << (8 * k);
        }
        s_sym[2 * i] = lo;
        s_sym[2 * i + 1] = hi;
    }
    __syncthreads();

    // ---- forward pass: a lane holds one step's byte; a branch costs the transmitted bits that differ from its nibble
    const uint32_t e0 = branch_nibble(lane);
    unsigned long long *surv = a.surv + (size_t)f * a.slot[a.n_units] + a.slot[ui];
    const uint8_t *sym = (const uint8_t *)s_sym;
    const uint32_t corrected = dec_forward(
        surv, T, 1u << 24, [&](uint32_t c) __attribute__((always_inline)) { return (int)sym[c * 64 + lane]; },
        [&](int symv, int k) __attribute__((always_inline)) {
            const uint32_t r = (uint32_t)__builtin_amdgcn_readlane(symv, k);
            const uint32_t m = r >> 4, x0 = (e0 ^ r) & m, x1 = x0 ^ m;
            return DecCosts{(uint32_t)__popc(x0), (uint32_t)__popc(x1)};
        });

    uint8_t *dec = (uint8_t *)s_pun;
    dec_traceback(surv, T, in_bytes, dec);
    uint32_t errors = dec_disperse(a, f, u.in_off, in_bytes, dec);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) errors += __shfl_xor(errors, off);
    if (lane == 0) *st = DecUnitStats{corrected, u.base[u.nseg] + 12u, errors, a.ref ? 8 * in_bytes : 0u};
}

__global__ __launch_bounds__(kDecThreads) void dec_soft_decode_kernel(DecSoftArgs a)
{
    __shared__ uint32_t s_dec[kDecRowWords + 2];         // the decoded bytes, before the energy dispersal
    extern __shared__ uint32_t s_soft[];               // the unit's punctured softs: 8 x out_bytes (a.lds_bytes)
    const int lane = threadIdx.x;
    const int f = blockIdx.x / a.n_units, ui = blockIdx.x % a.n_units;
    const FeUnit &u = a.units[ui];
    DecSoftUnitStats *st = a.stats + (size_t)f * a.n_units + ui;
    if (f < a.first_valid) return dec_no_output(st);
    const uint32_t in_bytes = u.in_bytes, soft_words = 2u * u.out_bytes;
    const size_t row_bytes = 8 * ((size_t)a.fic_out + kFeCifBytes);
    const uint32_t T = 8 * in_bytes + 6;

    // ---- the unit's punctured softs of output frame f.  Soft 8 p + b of a sub-channel lies in the row delayed by
    // {0,8,4,12,2,10,6,14}[b] + (p & 1) (delay_mask): dword d holds bits 4 (d & 1) ... of byte p = d >> 1
    const int8_t *row = a.rows + (size_t)f * row_bytes;
    if (u.owner < 0) {
        for (uint32_t d = lane; d < soft_words; d += kDecThreads) s_soft[d] = ((const uint32_t *)row)[d];
    } else {
        const uint8_t *src = (const uint8_t *)row + 8 * ((size_t)a.fic_out + u.dst_off);
        for (uint32_t d = lane; d < soft_words; d += kDecThreads) {
            const uint32_t first = 2u * (d & 1u) + ((d >> 1) & 1u);
            const uint8_t *at = src + 4 * (size_t)d;
            s_soft[d] = (uint32_t)at[(first + 0) * row_bytes] | ((uint32_t)at[(first + 8) * row_bytes + 1] << 8) |
                        ((uint32_t)at[(first + 4) * row_bytes + 2] << 16) | ((uint32_t)at[(first + 12) * row_bytes + 3] << 24);
        }
    }
    __syncthreads();

    // ---- forward pass.  sgn: 1 - 2 e_i per code bit of the branch from the predecessor whose oldest bit is 0, first code bit
    // in the lowest byte.  A lane holds one step's four softs (0 where the pattern drops the bit) and their magnitudes' sum
    struct Softs { uint32_t pk, tot; };
    const int8_t *soft = (const int8_t *)s_soft;
    const uint32_t e0 = branch_nibble(lane);
    const uint32_t sgn = ((e0 & 8u) ? 0xffu : 1u) | (((e0 & 4u) ? 0xffu : 1u) << 8) | (((e0 & 2u) ? 0xffu : 1u) << 16) |
                         (((e0 & 1u) ? 0xffu : 1u) << 24);
    unsigned long long *surv = a.surv + (size_t)f * a.slot[a.n_units] + a.slot[ui];
    const uint32_t final_metric = dec_forward(
        surv, T, 1u << 30,
        [&](uint32_t c) __attribute__((always_inline)) {
            const uint32_t t = c * 64 + lane;
            uint32_t pk = 0, tot = 0;
            if (t < T) {
                const FeSegment g = fe_segment(u, t >> 3);
                const int8_t *first = soft + g.at;     // (a local: the bit count below then adds onto one address)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const uint32_t pb = 31u - (4u * (t & 7u) + j);
                    if ((g.pattern >> pb) & 1u) {
                        const int v = first[__popcll((unsigned long long)g.pattern >> (pb + 1))];
                        pk |= ((uint32_t)v & 0xffu) << (8 * j);
                        tot += (uint32_t)abs(v);
                    }
                }
            }
            return Softs{pk, tot};
        },
        [&](Softs s, int k) __attribute__((always_inline)) {
            const int r = __builtin_amdgcn_readlane((int)s.pk, k);
            const int tt = __builtin_amdgcn_readlane((int)s.tot, k);
            const int dot = __builtin_amdgcn_sdot4((int)sgn, r, 0, false);
            const uint32_t c0 = (uint32_t)(tt + dot) >> 1, c1 = (uint32_t)tt - c0;
            return DecCosts{c0, c1};
        });

    uint8_t *dec = (uint8_t *)s_dec;
    dec_traceback(surv, T, in_bytes, dec);

    // ---- the decoded bits encoded again, against the softs: one lane per 4-byte group of the mother code (group in_bytes: the tail)
    uint32_t corrected = 0, contra = 0, soft_sum = 0, erasures = 0;
    for (uint32_t i = lane; i <= in_bytes; i += kDecThreads) {
        const uint32_t w = mother_code(i ? dec[i - 1] : 0u, i < in_bytes ? dec[i] : 0u);
        const FeSegment g = fe_segment(u, i);
        uint32_t at = g.at;
        for (int b = 31; b >= 0; --b) {
            if (!((g.pattern >> b) & 1u)) continue;
            const int v = soft[at++];
            const uint32_t mag = (uint32_t)abs(v);
            soft_sum += mag;
            if (v == 0) {
                ++erasures;
            } else if ((v > 0) != (bool)((w >> b) & 1u)) {
                ++corrected;
                contra += mag;
            }
        }
    }

    uint32_t errors = dec_disperse(a, f, u.in_off, in_bytes, dec);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        errors += __shfl_xor(errors, off);
        corrected += __shfl_xor(corrected, off);
        contra += __shfl_xor(contra, off);
        soft_sum += __shfl_xor(soft_sum, off);
        erasures += __shfl_xor(erasures, off);
    }
    if (lane == 0)
        *st = DecSoftUnitStats{final_metric, contra, soft_sum, corrected, erasures, u.base[u.nseg] + 12u, errors, a.ref ? 8 * in_bytes : 0u};
}

}  // namespace

hipError_t launch_dec_rows(const DecArgs &a, hipStream_t s)
{
    if (a.n_out <= 0) return hipSuccess;
    if (a.n_out % a.cifs || a.fic_out % 4) return hipErrorInvalidValue;
    const size_t total = (size_t)a.n_out * (size_t)(a.fic_out + kFeCifBytes) / 4;
    DABGPU_LAUNCH(dec_rows_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, a, total);
    return hipGetLastError();
}

hipError_t launch_dec_rows(const DecSoftArgs &a, hipStream_t s)
{
    if (a.n_out <= 0) return hipSuccess;
    if (a.n_out % a.cifs || a.fic_out % 4) return hipErrorInvalidValue;
    const size_t total = (size_t)a.n_out * (size_t)(a.fic_out + kFeCifBytes) * 2;
    DABGPU_LAUNCH(dec_soft_rows_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, a, total);
    return hipGetLastError();
}

hipError_t launch_dec_decode(const DecArgs &a, hipStream_t s)
{
    if (a.n_out <= 0 || a.n_units <= 0) return hipSuccess;
    if (a.lds_bytes <= 0 || a.lds_bytes % 64 || a.lds_bytes > kDecMaxSteps) return hipErrorInvalidValue;
    DABGPU_LAUNCH(dec_decode_kernel, dim3((unsigned)a.n_out * (unsigned)a.n_units), dim3(kDecThreads), (size_t)a.lds_bytes + 8, s, a);
    return hipGetLastError();
}

hipError_t launch_dec_decode(const DecSoftArgs &a, hipStream_t s)
{
    if (a.n_out <= 0 || a.n_units <= 0) return hipSuccess;
    if (a.lds_bytes <= 0 || a.lds_bytes % 4 || a.lds_bytes > 8 * kFeCifBytes) return hipErrorInvalidValue;
    DABGPU_LAUNCH(dec_soft_decode_kernel, dim3((unsigned)a.n_out * (unsigned)a.n_units), dim3(kDecThreads), (size_t)a.lds_bytes, s, a);
    return hipGetLastError();
}

}  // namespace dabgpu
