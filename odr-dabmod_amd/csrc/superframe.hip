// superframe.hip -- the DAB+ superframe reader's kernel (dabgpu_superframe*; superframe.h has the record, the field's tables and
// the header walk).
//   superframe_kernel   one workgroup per candidate (five consecutive images), four waves.  The five sub-channel frames come
//                       into LDS with dword loads (120 s <= 2880 bytes), the field's exp / log tables beside them (768 bytes).
//                       One wave per codeword, the waves loop over i < s: lane l holds positions l and l + 64 (l < 56), read as
//                       bytes at stride s.  Ten syndromes from per-lane terms (a running exponent, one table read per term),
//                       packed four to a dword and xor-reduced across the wave.  A zero syndrome vector ends the word: the
//                       common case costs twenty table reads and eighteen cross-lane steps.  Otherwise Berlekamp-Massey runs
//                       in every lane alike (ten unrolled steps on registers, the branches as selects), the Chien search
//                       evaluates the locator at the lane's two positions, a ballot counts the roots, and Forney runs in the
//                       lanes that hold one; the correction goes into LDS in place.  A word whose locator has fewer roots among
//                       the 120 real positions than its degree stays untouched (0xFF in cw_errors): the other roots lie in
//                       the shortened code's padding or nowhere.
//                       Behind a barrier: the 110 s data bytes go out, coalesced; lane 0 reads Fire code and header; lanes
//                       0 ... num_aus - 1 check one AU's CRC each; sixteen lanes store the record.
// No atomics, no state: records and bytes of a candidate depend on its five frames only, whatever the grid.
#include "device_common.h"
#include "superframe.h"

namespace dabgpu {
namespace {

alignas(16) __device__ const SfField kField{};

struct SfShared {
    uint32_t data[kSfFrames * 6 * kSfMaxS];     // the candidate's 120 s bytes, frame after frame
    uint32_t exp[128], log[64];                 // the field's tables as bytes
    SfRecord rec;
};

DEV uint32_t gf_mul(const uint8_t *ex, const uint8_t *lg, uint32_t a, uint32_t b)
{
    return (a && b) ? ex[(uint32_t)lg[a] + lg[b]] : 0u;
}
DEV uint32_t mod255(uint32_t x) { return x >= 255u ? x - 255u : x; }

// sum_j c[j] alpha^(j z) for j < N, z < 255: a running exponent, one table read per non-zero coefficient
template <int N> DEV uint32_t gf_eval(const uint8_t *ex, const uint8_t *lg, const uint32_t (&c)[N], uint32_t z)
{
    uint32_t q = c[0], e = 0;
#pragma unroll
    for (int j = 1; j < N; ++j) {
        e = mod255(e + z);
        q ^= c[j] ? ex[lg[c[j]] + e] : 0u;
    }
    return q;
}

DEV uint32_t wave_xor(uint32_t x)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x ^= (uint32_t)__shfl_xor((int)x, o, 64);
    return x;
}

__global__ __launch_bounds__(kSfBlock) void superframe_kernel(SfArgs a)
{
    __shared__ SfShared sh;
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6, s = a.s, f = blockIdx.x;
    const uint32_t frame_words = 6 * s, words = kSfFrames * frame_words;
    for (uint32_t idx = t; idx < words; idx += kSfBlock) {
        const uint32_t k = idx / frame_words, w = idx - k * frame_words;
        sh.data[idx] = reinterpret_cast<const uint32_t *>(a.images + (size_t)(f + k) * 6144 + a.offset)[w];
    }
    if (t < 128) sh.exp[t] = reinterpret_cast<const uint32_t *>(kField.exp)[t];
    else if (t < 192) sh.log[t - 128] = reinterpret_cast<const uint32_t *>(kField.log)[t - 128];
    if (t < sizeof(SfRecord) / 4) reinterpret_cast<uint32_t *>(&sh.rec)[t] = 0;
    __syncthreads();
    uint8_t *bytes = reinterpret_cast<uint8_t *>(sh.data);
    const uint8_t *ex = reinterpret_cast<const uint8_t *>(sh.exp), *lg = reinterpret_cast<const uint8_t *>(sh.log);

    const bool two = lane < (uint32_t)(kSfN - 64);
    const uint32_t e0 = (uint32_t)(kSfN - 1) - lane, e1 = two ? e0 - 64u : 0u;          // position p carries alpha^(119 - p)
    const uint32_t z0 = mod255(136u + lane), z1 = mod255(200u + lane);                    // ... and is a root at alpha^(136 + p)
    for (uint32_t i = wave; i < s; i += kSfBlock / 64) {
        const uint32_t r0 = bytes[i + s * lane], r1 = two ? bytes[i + s * (lane + 64u)] : 0u;
        // S_j = sum_p r_p alpha^(j (119 - p)), four to a dword
        uint32_t pk[3] = {0, 0, 0};
        {
            uint32_t x0 = lg[r0], x1 = lg[r1];
#pragma unroll
            for (int j = 0; j < kSfParity; ++j) {
                const uint32_t term = (r0 ? ex[x0] : 0u) ^ (r1 ? ex[x1] : 0u);
                pk[j >> 2] |= term << (8 * (j & 3));
                x0 = mod255(x0 + e0);
                x1 = mod255(x1 + e1);
            }
        }
        pk[0] = wave_xor(pk[0]);
        pk[1] = wave_xor(pk[1]);
        pk[2] = wave_xor(pk[2]);
        if ((pk[0] | pk[1] | pk[2]) == 0) continue;                                       // (cw_errors[i] is zero already)
        uint32_t syn[kSfParity];
#pragma unroll
        for (int j = 0; j < kSfParity; ++j) syn[j] = (pk[j >> 2] >> (8 * (j & 3))) & 0xffu;
        // Berlekamp-Massey, the same in every lane: lam (lam[0] = 1 throughout), b, the register length el
        uint32_t lam[kSfParity + 1], b[kSfParity + 1];
#pragma unroll
        for (int j = 0; j <= kSfParity; ++j) lam[j] = b[j] = j == 0;
        uint32_t el = 0;
#pragma unroll
        for (int r = 1; r <= kSfParity; ++r) {
            uint32_t d = 0;
#pragma unroll
            for (int j = 0; j < r; ++j) d ^= gf_mul(ex, lg, lam[j], syn[r - 1 - j]);
            const bool longer = d != 0 && 2 * el <= (uint32_t)(r - 1);
            const uint32_t di = d ? ex[255u - lg[d]] : 0u;
#pragma unroll
            for (int j = kSfParity; j >= 1; --j) {                                        // lam <- lam - d x b;  b <- lam / d or x b
                const uint32_t old = lam[j];
                lam[j] = old ^ gf_mul(ex, lg, d, b[j - 1]);
                b[j] = longer ? gf_mul(ex, lg, old, di) : b[j - 1];
            }
            b[0] = longer ? di : 0u;
            el = longer ? (uint32_t)r - el : el;
        }
        uint32_t deg = 0;
#pragma unroll
        for (int j = 1; j <= kSfParity; ++j) deg = lam[j] ? (uint32_t)j : deg;
        // Chien: the lane's two positions; every root must be among the 120 real ones
        const bool root0 = gf_eval(ex, lg, lam, z0) == 0, root1 = two && gf_eval(ex, lg, lam, z1) == 0;
        const uint32_t n_roots = (uint32_t)__popcll(__ballot(root0)) + (uint32_t)__popcll(__ballot(root1));
        if (n_roots != deg) {
            if (lane == 0) sh.rec.cw_errors[i] = (uint8_t)kSfFailed;
            continue;
        }
        // Forney: omega = syn lam mod x^deg; the error at a root alpha^z is omega(alpha^z) alpha^(-z) / lam'(alpha^z)
        uint32_t omega[kSfParity], der[kSfParity];
#pragma unroll
        for (int k = 0; k < kSfParity; ++k) {
            uint32_t acc = 0;
#pragma unroll
            for (int j = 0; j <= k; ++j) acc ^= gf_mul(ex, lg, syn[k - j], lam[j]);
            omega[k] = (uint32_t)k < deg ? acc : 0u;
            der[k] = (k & 1) ? 0u : lam[k + 1];                                           // the formal derivative keeps the odd terms
        }
        if (root0 || root1) {
            const uint32_t z = root0 ? z0 : z1;
            // (a lane may hold two roots: the second is handled below)
            const uint32_t num = gf_mul(ex, lg, gf_eval(ex, lg, omega, z), ex[mod255(255u - z)]), den = gf_eval(ex, lg, der, z);
            const uint32_t at = i + s * (root0 ? lane : lane + 64u);
            bytes[at] = (uint8_t)(bytes[at] ^ gf_mul(ex, lg, num, ex[255u - lg[den]]));
        }
        if (root0 && root1) {
            const uint32_t num = gf_mul(ex, lg, gf_eval(ex, lg, omega, z1), ex[mod255(255u - z1)]), den = gf_eval(ex, lg, der, z1);
            const uint32_t at = i + s * (lane + 64u);
            bytes[at] = (uint8_t)(bytes[at] ^ gf_mul(ex, lg, num, ex[255u - lg[den]]));
        }
        if (lane == 0) sh.rec.cw_errors[i] = (uint8_t)deg;
    }
    __syncthreads();
    const uint32_t n_out = (uint32_t)kSfK * s;
    uint8_t *out = a.out + (size_t)f * n_out;
    for (uint32_t idx = t; idx < n_out; idx += kSfBlock) out[idx] = bytes[idx];
    if (t == 0) {
        SfRecord &r = sh.rec;
        uint32_t corrected = 0, failed = 0, most = 0;
        for (uint32_t i = 0; i < s; ++i) {
            const uint32_t e = r.cw_errors[i];
            if (e == kSfFailed) {
                failed++;
            } else {
                corrected += e;
                most = e > most ? e : most;
            }
        }
        r.rs_corrected = (uint16_t)corrected;
        r.rs_failed = (uint16_t)failed;
        r.rs_max = (uint8_t)most;
        if (failed) r.flags |= SF_RS_FAILED;
        sf_read_header(bytes, s, &r);
    }
    __syncthreads();
    const bool read_aus = sf_accepted(sh.rec.flags);
    bool ok = false;
    if (read_aus && t < sh.rec.num_aus) ok = sf_au_ok(bytes, sh.rec.au_start[t], sh.rec.au_start[t + 1]);
    if (t < 64) {
        const uint32_t mask = (uint32_t)__ballot(ok);
        uint32_t w = reinterpret_cast<const uint32_t *>(&sh.rec)[t & 15u];
        if (t == 2) w |= mask << 16;                                                      // au_ok: byte 10 of the record
        if (t < sizeof(SfRecord) / 4) reinterpret_cast<uint32_t *>(a.rec + f)[t] = w;
    }
}

}  // namespace

hipError_t launch_superframe(const SfArgs &a, hipStream_t stream)
{
    if (!a.images || ((uintptr_t)a.images & 3u) || !a.rec || !a.out || a.n_images < (uint32_t)kSfFrames || a.n_images > (1u << 22) ||
        a.s < 1 || a.s > (uint32_t)kSfMaxS || (a.offset & 3u) || (size_t)a.offset + 24u * a.s > 6144)
        return hipErrorInvalidValue;
    DABGPU_LAUNCH(superframe_kernel, dim3(a.n_images - (kSfFrames - 1)), dim3(kSfBlock), 0, stream, a);
    return hipGetLastError();
}

}  // namespace dabgpu
