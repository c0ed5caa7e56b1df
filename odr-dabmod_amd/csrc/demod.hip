// demod.hip -- the receiver beside the modulator: native-rate IQ of whole transmission frames -> the coded bits a chain call
// takes as input, plus per-frame quality figures.  The frame kernel's geometry backwards: one workgroup of N/8 lanes, eight
// samples per lane, the forward transform CFR already runs (Fft<LOGN>::run<-1>), differential demodulation against the
// previous symbol's bins kept in registers, hard decisions, and the frequency interleaver undone through Tables::src_carrier.
// Written from ETSI EN 300 401 (14.5 - 14.7), like tests/receiver.py; the reference has no receiver.  No synchronisation and
// no channel estimate: the caller says where the FFT window lies (`early` samples before the end of every symbol).
#include "device_common.h"

namespace dabgpu {
namespace {

// One workgroup = one RUN of consecutive data symbols of one frame (a.syms_per_run of them; the last run of a frame may be
// shorter).  Data block b (0 ...  nb_symbols - 2) is symbol b + 2 of the frame -- symbol 0 is the null symbol, symbol 1 the
// phase reference -- and is decided against symbol b + 1, so a run first transforms the symbol in front of its first.
//
// After the transform lane t holds bins t + T m.  Occupied: bins 1 ... K/2 = 3T (m = 0 without lane 0's DC bin, m = 1, 2, and
// bin 3T itself: lane 0, m = 3) and bins N - K/2 = 5T ... N - 1 (m = 5, 6, 7): six carriers per lane, the frame kernel's set.
// Carrier position k (bins 1 ... K/2 -> k = bin - 1, bins N - K/2 ... -> k = bin - N + K) is bit n = src_carrier[k] of the
// block: I half then Q half, K/8 bytes each, MSB first.  The lanes OR their bits into one LDS image of the
// block; the first K/16 lanes store it as dwords and count the bits that differ from the reference block.
//
// SOFT (dabgpu_demod_soft*): besides all of the above, one int8 metric per coded bit -- clamp(rint(-Re d q)), clamp(rint(-Im d
// q)) with q = 64 sqrt(2) / sqrt(P / K), P = the symbol's sum of |d|^2.  P is added in a FIXED order (the lane's six terms, an
// xor butterfly inside the wave, the waves in wave order through LDS), so the bytes repeat bit for bit and do not depend on
// the run geometry.  The softs go to an LDS image of the block by byte writes (soft n of the I half, K + n of the Q half: one
// writer each) and leave as 3 T dwords, three per lane, contiguous across the lanes.  The hard instantiations carry none of it.
template <int LOGN, bool SOFT> __device__ __forceinline__ void demod_body(const DemodArgs &a)
{
    typedef Fft<LOGN> F;
    constexpr int N = F::N, T = F::T, K = 3 * N / 4, WORDS = K / 16;
    static_assert(WORDS <= T, "one lane per dword of the block");
    static_assert(2 * K == 12 * T, "three soft dwords per lane");
    constexpr int NW = (T + 63) / 64, WL = T < 64 ? T : 64;
    __shared__ cf xbuf[2 * F::LDS_ELEMS];
    __shared__ uint32_t blk[WORDS];
    __shared__ uint32_t sblk[SOFT ? 3 * T : 1];
    __shared__ float red_p[SOFT ? NW : 1];
    __shared__ double red_s[T], red_q[T];
    __shared__ float red_m[T];
    __shared__ unsigned red_e[T];

    const int t = (int)threadIdx.x;
    const int nblocks = a.g.nb_symbols - 1;
    const int frame = (int)blockIdx.x / a.runs_per_frame;
    const int run = (int)blockIdx.x - frame * a.runs_per_frame;
    const int b0 = run * a.syms_per_run;
    const int b1 = min(b0 + a.syms_per_run, nblocks);
    if (frame >= a.n_frames || b0 >= b1) return;

    cf tw[F::NTW > 0 ? F::NTW : 1];
    F::template load_twiddles<false>(a.t.twiddle, t, tw);
    if (t < WORDS) blk[t] = 0u;            // (ordered in front of the first OR by the barriers of the first transform)

    // the lane's six carriers: slot, and where the carrier's two bits go in the LDS image (word, bit inside the word)
    // (slot 0 of lane 0 is the DC bin: its first carrier is bin 3T, slot 3; selected by value, never by a register index)
    constexpr int rr[6] = {0, 1, 2, 5, 6, 7};
    int iword[6], qword[6], nsoft[SOFT ? 6 : 1];
    unsigned shift[6];
#pragma unroll
    for (int c = 0; c < 6; ++c) {
        const int bin = t + T * ((c == 0 && t == 0) ? 3 : rr[c]);
        const int k = (bin <= K / 2) ? bin - 1 : bin - N + K;
        const int n = a.t.src_carrier[k];
        const int ib = n >> 3, qb = ib + K / 8;
        iword[c] = ib >> 2;
        qword[c] = qb >> 2;
        // (K/8 is a multiple of four bytes in every mode: the byte's place inside its word is the same in both halves)
        shift[c] = 8u * ((unsigned)ib & 3u) + (7u - ((unsigned)n & 7u));
        if constexpr (SOFT) nsoft[c] = n;
    }

    const size_t first = (size_t)a.g.null_size + (size_t)(a.g.sym_size - N - a.early);      // window of symbol 1
    const float2 *in_f = reinterpret_cast<const float2 *>(a.iq) + (size_t)frame * a.frame_stride + first;
    const uint32_t *in_s = reinterpret_cast<const uint32_t *>(a.iq) + (size_t)frame * a.frame_stride + first;
    auto load = [&](int s, cf *v) __attribute__((always_inline)) {      // symbol s >= 1 of the frame
        const size_t off = (size_t)(s - 1) * (size_t)a.g.sym_size + (size_t)t;
#pragma unroll
        for (int m = 0; m < 8; ++m) {
            if (a.fmt == 0) {
                v[m] = in_f[off + T * m];
            } else {
                const uint32_t w = in_s[off + T * m];                   // s16 pair: re in the low half
                v[m] = mk((float)(short)(w & 0xffffu), (float)(short)(w >> 16));
            }
        }
    };

    int par = 0;
    cf v[8], prev[6];
    load(b0 + 1, v);
    F::template run<-1, true, cf, false>(v, xbuf, par, tw, t);
#pragma unroll
    for (int c = 0; c < 6; ++c) prev[c] = v[rr[c]];
    if (t == 0) prev[0] = v[3];

    const size_t block_words = (size_t)frame * (size_t)nblocks * WORDS;
    uint32_t *soft_out = SOFT ? reinterpret_cast<uint32_t *>(a.soft_out) + (size_t)frame * (size_t)nblocks * (3 * T) : nullptr;
    double acc_s = 0., acc_q = 0.;
    float worst = 1.0f;                    // min over the lane's decisions of min(|Re d|, |Im d|)^2 / |d|^2
    unsigned errors = 0u;
    for (int b = b0; b < b1; ++b) {
        load(b + 2, v);
        F::template run<-1, true, cf, false>(v, xbuf, par, tw, t);
        float ps = 0.f, pq = 0.f;
        float sre[SOFT ? 6 : 1], sim[SOFT ? 6 : 1];
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            const cf z = (c == 0 && t == 0) ? v[3] : v[rr[c]], p = prev[c];
            const float dre = fmaf(z.x, p.x, z.y * p.y), dim = fmaf(z.y, p.x, -(z.x * p.y));      // z conj(p)
            prev[c] = z;
            if constexpr (SOFT) { sre[c] = dre; sim[c] = dim; }
            const unsigned I = dre < 0.f ? 1u : 0u, Q = dim < 0.f ? 1u : 0u;
            if (I) atomicOr(&blk[iword[c]], 1u << shift[c]);
            if (Q) atomicOr(&blk[qword[c]], 1u << shift[c]);
            const float ar = fabsf(dre), ai = fabsf(dim);
            const float p2 = fmaf(ar, ar, ai * ai);
            const float dq = ai - ar;                       // sqrt(2) Im(d conj(c)) up to its sign
            ps += p2;
            pq = fmaf(0.5f * dq, dq, pq);
            const float lo = fminf(ar, ai);
            worst = fminf(worst, p2 > 0.f ? (lo * lo) / p2 : 0.f);
        }
        acc_s += (double)ps;
        acc_q += (double)pq;
        if constexpr (SOFT) {
            // the symbol's power: the butterfly leaves the same sum in every lane of the wave (a + b = b + a exactly)
            float pw = ps;
#pragma unroll
            for (int off = WL / 2; off >= 1; off >>= 1) pw += __shfl_xor(pw, off, WL);
            if ((t & 63) == 0) red_p[t >> 6] = pw;
        }
        lds_barrier();
        if constexpr (SOFT) {
            float P = red_p[0];
#pragma unroll
            for (int w = 1; w < NW; ++w) P += red_p[w];
            const float q = P > 0.f ? 90.50966799187809f / sqrtf(P / (float)K) : 0.f;
            int8_t *sb = reinterpret_cast<int8_t *>(sblk);
#pragma unroll
            for (int c = 0; c < 6; ++c) {
                sb[nsoft[c]] = (int8_t)(int)fminf(fmaxf(rintf(-sre[c] * q), -127.f), 127.f);
                sb[K + nsoft[c]] = (int8_t)(int)fminf(fmaxf(rintf(-sim[c] * q), -127.f), 127.f);
            }
            lds_barrier();
            uint32_t *dst = soft_out + (size_t)b * (3 * T);
#pragma unroll
            for (int j = 0; j < 3; ++j) dst[t + T * j] = sblk[t + T * j];
        }
        if (t < WORDS) {
            const uint32_t w = blk[t];
            blk[t] = 0u;                   // (the next symbol's ORs come behind the barriers of its transform)
            const size_t at = block_words + (size_t)b * WORDS + (size_t)t;
            if (a.bits_out) reinterpret_cast<uint32_t *>(a.bits_out)[at] = w;
            if (a.ref_bits) errors += (unsigned)__popc(w ^ reinterpret_cast<const uint32_t *>(a.ref_bits)[at]);
        }
    }

    // the run's share of the frame's figures: the lanes' through LDS (sixteen partial sums, then one lane), one atomic each
    red_s[t] = acc_s; red_q[t] = acc_q; red_m[t] = worst; red_e[t] = errors;
    lds_barrier();
    if (t < 16) {
        double s = 0., q = 0.;
        float m = 1.0f;
        unsigned e = 0u;
        for (int i = t; i < T; i += 16) { s += red_s[i]; q += red_q[i]; m = fminf(m, red_m[i]); e += red_e[i]; }
        red_s[t] = s; red_q[t] = q; red_m[t] = m; red_e[t] = e;
    }
    lds_barrier();
    if (t == 0) {
        double s = 0., q = 0.;
        float m = 1.0f;
        unsigned e = 0u;
        for (int i = 0; i < 16; ++i) { s += red_s[i]; q += red_q[i]; m = fminf(m, red_m[i]); e += red_e[i]; }
        DemodFrameStats *st = a.stats + frame;
        atomicAdd(&st->sum_signal, s);
        atomicAdd(&st->sum_quadrature, q);
        if (e) atomicAdd(&st->bit_errors, (unsigned long long)e);
        // the smallest margin as the LARGEST complement of its bit pattern (non-negative floats order like their bits):
        // a zeroed record is then "no decision yet"
        atomicMax(&st->min_margin_inv, ~__float_as_uint(sqrtf(m)));
    }
}

template <int LOGN> __global__ __launch_bounds__(Fft<LOGN>::T) void demod_kernel(DemodArgs a) { demod_body<LOGN, false>(a); }
template <int LOGN> __global__ __launch_bounds__(Fft<LOGN>::T) void demod_soft_kernel(DemodArgs a) { demod_body<LOGN, true>(a); }

}  // namespace

// (demod_runs: how a frame's data symbols are split into runs -- forced: symbols per run, 0 = by the batch size.  A run costs
// one transform more than its symbols, so runs stay at four symbols or more; the grid aims at four workgroups per CU.)
void demod_runs(const Geometry &g, size_t n_frames, int forced, int *runs_per_frame, int *syms_per_run)
{
    const int nblocks = g.nb_symbols - 1;
    int spr;
    if (forced > 0) {
        spr = std::min(forced, nblocks);
    } else {
        const size_t want = n_frames ? (1024 + n_frames - 1) / n_frames : 1;
        const int runs = (int)std::min<size_t>(std::max<size_t>(want, 1), (size_t)((nblocks + 3) / 4));
        spr = (nblocks + runs - 1) / runs;
    }
    *syms_per_run = spr;
    *runs_per_frame = (nblocks + spr - 1) / spr;
}

hipError_t launch_demod(const DemodArgs &a, hipStream_t s)
{
    if (a.n_frames <= 0) return hipSuccess;
    if (a.early < 0 || a.early > a.g.sym_size - a.g.N || a.runs_per_frame < 1 || a.syms_per_run < 1 ||
        (a.fmt != 0 && a.fmt != 1) || a.g.K != 3 * a.g.N / 4)
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)a.n_frames * (unsigned)a.runs_per_frame);
    if (a.soft_out) {
        switch (a.g.logN) {
        case 8: DABGPU_LAUNCH(demod_soft_kernel<8>, grid, dim3(Fft<8>::T), 0, s, a); break;
        case 9: DABGPU_LAUNCH(demod_soft_kernel<9>, grid, dim3(Fft<9>::T), 0, s, a); break;
        case 10: DABGPU_LAUNCH(demod_soft_kernel<10>, grid, dim3(Fft<10>::T), 0, s, a); break;
        case 11: DABGPU_LAUNCH(demod_soft_kernel<11>, grid, dim3(Fft<11>::T), 0, s, a); break;
        default: return hipErrorInvalidValue;
        }
        return hipGetLastError();
    }
    switch (a.g.logN) {
    case 8: DABGPU_LAUNCH(demod_kernel<8>, grid, dim3(Fft<8>::T), 0, s, a); break;
    case 9: DABGPU_LAUNCH(demod_kernel<9>, grid, dim3(Fft<9>::T), 0, s, a); break;
    case 10: DABGPU_LAUNCH(demod_kernel<10>, grid, dim3(Fft<10>::T), 0, s, a); break;
    case 11: DABGPU_LAUNCH(demod_kernel<11>, grid, dim3(Fft<11>::T), 0, s, a); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace dabgpu
