// fic.hip -- the FIC reader's kernels (dabgpu_fic_scan*; fic.h has the walk itself and the record it fills).
//   fic_fib_kernel           one lane per FIB, 256 FIBs per workgroup: the workgroup's FIBs come into LDS with coalesced dword
//                            loads (fic_offset is only four-byte aligned), every lane checks its FIB's CRC, walks its FIGs from
//                            LDS and writes one 288-byte record with 16-byte stores
//   fic_reduce_kernel        one workgroup per 256 records: per SubChId the summary of the block's run of FIBs (lane = SubChId,
//                            wave = quarter of the block, the four quarters combined in order), the EId's summary by a tree over
//                            adjacent FIBs, and the block's integer sums -- no atomics, a fixed order
//   fic_reduce_final_kernel  one workgroup: the blocks' summaries combined in block order, the sums added
// fic_combine is associative, so the split into quarters, blocks and tree levels gives what one pass over the FIBs gives:
// the result does not depend on the grid.
// LDS row pitch: a FIB is 8 dwords.  At a pitch of 8 the byte reads of 32 lanes that walk at about the same offset fall on 4 of
// the 32 banks (8-way); at 9 dwords lane l reads bank (9 l + k) mod 32, all different while the lanes are at the same k.  The
// walks diverge with the FIBs' contents, so this is the common case, not a guarantee -- and whether it can be measured at
// these sizes has not been tried.
#include "device_common.h"
#include "fic.h"

namespace dabgpu {
namespace {

constexpr int kPitch = 9;                  // dwords per FIB row in LDS
struct alignas(16) FicRecord16 {
    FicRecord r;
};
static_assert(sizeof(FicRecord16) == sizeof(FicRecord) && sizeof(FicRecord) % 16 == 0, "records are stored as 16-byte words");

__global__ __launch_bounds__(kFicBlock) void fic_fib_kernel(FicArgs a)
{
    __shared__ uint32_t rows[kFicBlock * kPitch];
    const uint32_t t = threadIdx.x, n_fibs = a.n_images * a.fibs_per_image, f0 = blockIdx.x * (uint32_t)kFicBlock;
#pragma unroll
    for (int k = 0; k < kFibBytes / 4; ++k) {
        const uint32_t idx = t + (uint32_t)kFicBlock * k, fl = idx >> 3, w = idx & 7u, f = f0 + fl;
        if (f < n_fibs) {
            const uint32_t image = f / a.fibs_per_image, i = f - image * a.fibs_per_image;
            const uint32_t *src = reinterpret_cast<const uint32_t *>(a.images + (size_t)image * 6144 + a.fic_offset + kFibBytes * i);
            rows[fl * kPitch + w] = src[w];
        }
    }
    __syncthreads();
    const uint32_t f = f0 + t;
    if (f >= n_fibs) return;
    FicRecord16 rec;
    fic_read_fib(reinterpret_cast<const uint8_t *>(&rows[t * kPitch]), &rec.r);
    uint4 *dst = reinterpret_cast<uint4 *>(a.rec + f);
    const uint4 *src = reinterpret_cast<const uint4 *>(&rec);
#pragma unroll
    for (int i = 0; i < (int)(sizeof(FicRecord) / 16); ++i) dst[i] = src[i];
}

DEV FicRun no_run()
{
    FicRun r;
    r.first_word = r.last_word = r.seen = r.changes = r.first_fib = r.last_fib = 0;
    return r;
}

__global__ __launch_bounds__(kFicBlock) void fic_reduce_kernel(FicArgs a)
{
    __shared__ FicRun quarter[4][64];
    __shared__ FicRun tree[kFicBlock];
    __shared__ uint8_t cnt[FIC_COUNTERS][kFicBlock];
    __shared__ uint32_t part[4][64];
    const uint32_t t = threadIdx.x, n_fibs = a.n_images * a.fibs_per_image, f0 = blockIdx.x * (uint32_t)kFicBlock;
    const uint32_t s = t & 63u, q = t >> 6;
    // the sub-channels: lane = SubChId, wave = quarter; every lane of a wave reads the same record
    FicRun run = no_run();
    for (uint32_t j = 0; j < 64; ++j) {
        const uint32_t f = f0 + 64 * q + j;
        if (f >= n_fibs) break;
        const FicRecord &r = a.rec[f];
        if (!(r.flags & FIC_CRC_OK)) continue;
        const uint32_t n = r.n_sub < (uint32_t)kFicRecSub ? r.n_sub : (uint32_t)kFicRecSub;
        for (uint32_t e = 0; e < n; ++e)
            if (r.sub[e].subchid == s) run = fic_combine(run, fic_sighting(r.sub[e].raw, f));
    }
    quarter[q][s] = run;
    // the EId and the sums: lane = FIB
    const uint32_t f = f0 + t;
    FicRun eid = no_run();
    if (f < n_fibs) {
        const FicRecord &r = a.rec[f];
        if ((r.flags & FIC_CRC_OK) && r.eid_seen) {
            eid.first_word = r.eid_first;
            eid.last_word = r.eid;
            eid.seen = r.eid_seen;
            eid.changes = r.eid_changes;
            eid.first_fib = eid.last_fib = f;
        }
#pragma unroll
        for (int c = 0; c < FIC_COUNTERS; ++c) cnt[c][t] = (uint8_t)fic_counter_of(r, c);
    } else {
#pragma unroll
        for (int c = 0; c < FIC_COUNTERS; ++c) cnt[c][t] = 0;
    }
    tree[t] = eid;
    __syncthreads();
    for (uint32_t stride = 1; stride < (uint32_t)kFicBlock; stride *= 2) {
        if ((t & (2 * stride - 1)) == 0) tree[t] = fic_combine(tree[t], tree[t + stride]);
        __syncthreads();
    }
    uint32_t sum = 0;
    if (s < (uint32_t)FIC_COUNTERS)
        for (uint32_t i = 0; i < 64; ++i) sum += cnt[s][64 * q + i];
    part[q][s] = sum;
    __syncthreads();
    FicReduced &out = a.partial[blockIdx.x];
    if (t < 64) {
        out.sub[t] = fic_combine(fic_combine(quarter[0][t], quarter[1][t]), fic_combine(quarter[2][t], quarter[3][t]));
        out.counter[t] = part[0][t] + part[1][t] + part[2][t] + part[3][t];
    }
    if (t == 64) out.eid = tree[0];
}

constexpr int kFinalThreads = 192;
__global__ __launch_bounds__(kFinalThreads) void fic_reduce_final_kernel(FicArgs a, uint32_t n_blocks)
{
    const uint32_t t = threadIdx.x;
    if (t < 64) {
        FicRun run = no_run();
        for (uint32_t b = 0; b < n_blocks; ++b) run = fic_combine(run, a.partial[b].sub[t]);
        a.result->sub[t] = run;
    } else if (t == 64) {
        FicRun run = no_run();
        for (uint32_t b = 0; b < n_blocks; ++b) run = fic_combine(run, a.partial[b].eid);
        a.result->eid = run;
    } else if (t >= 128) {
        uint32_t sum = 0;
        for (uint32_t b = 0; b < n_blocks; ++b) sum += a.partial[b].counter[t - 128];
        a.result->counter[t - 128] = sum;
    }
}

}  // namespace

hipError_t launch_fic(const FicArgs &a, hipStream_t s)
{
    if (!a.images || ((uintptr_t)a.images & 3u) || !a.rec || !a.partial || !a.result || a.n_images < 1 || a.n_images > (1u << 22) ||
        (a.fibs_per_image != 3 && a.fibs_per_image != 4) || (a.fic_offset & 3u) ||
        (size_t)a.fic_offset + (size_t)kFibBytes * a.fibs_per_image > 6144)
        return hipErrorInvalidValue;
    const uint32_t n_fibs = a.n_images * a.fibs_per_image, n_blocks = (n_fibs + kFicBlock - 1) / kFicBlock;
    DABGPU_LAUNCH(fic_fib_kernel, dim3(n_blocks), dim3(kFicBlock), 0, s, a);
    DABGPU_LAUNCH(fic_reduce_kernel, dim3(n_blocks), dim3(kFicBlock), 0, s, a);
    DABGPU_LAUNCH(fic_reduce_final_kernel, dim3(1), dim3(kFinalThreads), 0, s, a, n_blocks);
    return hipGetLastError();
}

}  // namespace dabgpu
