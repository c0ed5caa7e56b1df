// rx_symbols.h -- what the kernels that walk the data symbols of whole frames share (demod.hip: demod_body and the float64
// state pass; clock.hip: the estimator): the run of symbols a workgroup takes and where their FFT windows lie (RxSymbolArgs,
// dabgpu_internal.h), and the six carriers a lane of the fp32 walkers holds after the transform.  Written from ETSI
// EN 300 401 (14.5 - 14.7); the reference has no receiver.  Anonymous namespace, as device_common.h.
#pragma once
#include "device_common.h"
#include "turn_phase.h"      // ld_iq

namespace dabgpu {
namespace {

// One workgroup = one RUN of consecutive data symbols of one frame (a.syms_per_run of them; the last run of a frame may be
// shorter), workgroup frame * runs_per_frame + run.  Data block b (0 ...  nb_symbols - 2) is symbol b + 2 of the frame --
// symbol 0 is the null symbol, symbol 1 the phase reference -- and is decided against symbol b + 1, so a run first
// transforms the symbol in front of its first: symbol b0 + 1, then symbol b + 2 for b = b0 ... b1 - 1.  idle: no such
// frame, or no block left for this run -- the workgroup returns.
struct RxRun { int frame, b0, b1; bool idle; };
DEV RxRun rx_run(const RxSymbolArgs &a)
{
    RxRun r;
    const int nblocks = a.g.nb_symbols - 1;
    r.frame = (int)blockIdx.x / a.runs_per_frame;
    const int run = (int)blockIdx.x - r.frame * a.runs_per_frame;
    r.b0 = run * a.syms_per_run;
    r.b1 = min(r.b0 + a.syms_per_run, nblocks);
    r.idle = r.frame >= a.n_frames || r.b0 >= r.b1;
    return r;
}
// Where the N-sample FFT windows of frame `frame` lie, a.early samples before the end of every symbol: of(s) = index into
// a.iq of symbol s >= 1's.  Formed behind the idle workgroups' return; the kernels load through an always_inline lambda.
template <int N> struct RxWindows {
    long long base;           // the window of symbol 1
    int sym_size;
    DEV RxWindows(const RxSymbolArgs &a, int frame)
    {
        const size_t first = (size_t)a.g.null_size + (size_t)(a.g.sym_size - N - a.early);
        base = (long long)((size_t)frame * a.frame_stride + first);
        sym_size = a.g.sym_size;
    }
    DEV long long of(int s) const { return base + (long long)(s - 1) * (long long)sym_size; }
};

// carrier position k (the frame kernel's order: Tables::src_carrier, phase_q, the weights) <-> bin of the N-point transform:
// bins 1 ... K/2 are k = bin - 1, bins N - K/2 ... N - 1 are k = bin - N + K
template <int N> DEV int bin_position(int bin) { return (bin <= 3 * N / 8) ? bin - 1 : bin - N + 3 * N / 4; }
template <int N> DEV int position_bin(int k) { return k < 3 * N / 8 ? k + 1 : k - 3 * N / 4 + N; }

// The fp32 walkers: one workgroup of T = N/8 lanes, eight samples per lane (sample t + T m in v[m]), the forward transform
// CFR already runs (Fft<LOGN>::run<-1>).  After it lane t holds bins t + T m.  Occupied: bins 1 ... K/2 = 3T (m = 0 without
// lane 0's DC bin, m = 1, 2, and bin 3T itself: lane 0, m = 3) and bins N - K/2 = 5T ... N - 1 (m = 5, 6, 7): six carriers per
// lane, the frame kernel's set.  A lane keeps the previous symbol's six in registers.
template <int LOGN> struct SixCarriers {
    static constexpr int N = 1 << LOGN, T = N / 8;
    cf prev[6];
    static DEV int slot(int c) { constexpr int rr[6] = {0, 1, 2, 5, 6, 7}; return rr[c]; }       // carrier c's slot m
    static constexpr bool upper(int c) { return c < 3; }                // carrier c lies above the centre (bins 1 ... K/2)
    // position of the lane's carrier c (slot 0 of lane 0 is the DC bin: its first carrier is bin 3T, slot 3)
    static DEV int position(int c, int t) { return bin_position<N>(t + T * ((c == 0 && t == 0) ? 3 : slot(c))); }
    // the lane's eight samples of symbol s.  The kernels call this through an always_inline lambda of their own, as their
    // load was before it moved here: called directly from the symbol loop, the compiler orders sco_kernel's loop another way
    static DEV void load(const RxSymbolArgs &a, const RxWindows<N> &w, int s, int t, cf *v)
    {
        const long long off = w.of(s) + t;
#pragma unroll
        for (int m = 0; m < 8; ++m) v[m] = ld_iq(a.iq, a.fmt, off + T * m);
    }
    // the symbol in front of the run's first
    DEV void start(const cf *v, int t)
    {
#pragma unroll
        for (int c = 0; c < 6; ++c) prev[c] = v[slot(c)];
        if (t == 0) prev[0] = v[3];
    }
    // d = z conj(p) of carrier c against the previous symbol, which this one then replaces (lane 0's first carrier is
    // selected by value, never by a register index)
    DEV cf against_previous(const cf *v, int c, int t)
    {
        const cf z = (c == 0 && t == 0) ? v[3] : v[slot(c)], p = prev[c];
        const float dre = fmaf(z.x, p.x, z.y * p.y), dim = fmaf(z.y, p.x, -(z.x * p.y));
        prev[c] = z;
        return mk(dre, dim);
    }
};

}  // namespace
}  // namespace dabgpu
