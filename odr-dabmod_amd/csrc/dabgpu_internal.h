// dabgpu_internal.h -- shared between the kernel file and the C-ABI file.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <initializer_list>
#include <type_traits>

#include "conv_code.h"
#include "resampler_runs.h"
#include "welch.h"

namespace dabgpu {

constexpr int kMaxTaps = 128;        // fused (spectral) FIR of the frame kernel
constexpr int kEqTaps = 160;         // length of the inverse filter of the equalised-boundary variant (TF_EQ), centre at kEqCentre:
constexpr int kEqCentre = 56;        //   x[n] = sum_j eq_g[j] z[n - (j - kEqCentre)]
constexpr int kMaxTapsUnfused = 512; // direct FIR kernels (the chain falls back to them for longer filters)

// Transmission-mode geometry (reference src/DabModulator.cpp:84-122).
struct Geometry {
    int mode;
    int nb_symbols;  // 76 / 153 (phase reference + data symbols)
    int K;           // carriers
    int N;           // FFT size ("spacing")
    int logN;
    int null_size;
    int sym_size;
};
// samples of one transmission frame (the host's tf_samples is this as a size_t; stage_kernels.hip still writes the sum out)
__host__ __device__ inline long long frame_samples(const Geometry &g) { return (long long)g.null_size + (long long)g.nb_symbols * g.sym_size; }

// Device-resident constant tables, built once per context.
struct Tables {
    const float2 *twiddle;        // N entries, exp(+2 pi i m / N)
    const uint16_t *src_carrier;  // K: interleaved position k -> carrier index n before interleaving
    const uint16_t *dst_pos;      // K: carrier n -> interleaved position (reference's m_indices)
    const uint8_t *phase_q;       // K: quarter-turn index (0..3) of the phase reference at position k
    const float *mag;             // nb_symbols: |y| after s differential multiplications (fp32 recurrence)
    const float *taps;            // kMaxTaps floats, zero padded
    const float *window;          // 2*overlap floats (guard-interval raised cosine)
    const float2 *fir_h;          // N: frequency response of the taps, sum_j taps[j] e^{+2 pi i jk/N}
    const float *eq_g;            // TF_EQ: kEqTaps + 1 floats, the inverse of the taps on the occupied bins (see tf_kernel<..., EQ>)
};

// Launch trace (dabgpu_debug_last_variant): every kernel launch of the library goes through DABGPU_LAUNCH, which names the
// kernel to the calling thread's trace sink when one is set -- the chain entry points set it for the duration of the call.
// Off the traced path this is one thread-local pointer test per launch.
bool trace_on();
void trace_launch(const char *what);
#define DABGPU_LAUNCH(kernel, ...)                                      \
    do {                                                                \
        if (::dabgpu::trace_on()) ::dabgpu::trace_launch(#kernel);      \
        hipLaunchKernelGGL(kernel, __VA_ARGS__);                        \
    } while (0)
// The same for a kernel template whose arguments the launch holds as constants without spelling them out (by_fft_size):
// DABGPU_LAUNCH_T(kernel, (L, 0), ...) launches kernel<L, 0> and names it with the arguments' values, "kernel<11, 0>".
void trace_launch(const char *what, std::initializer_list<int> targs);
#define DABGPU_TARGS(...) __VA_ARGS__
#define DABGPU_LAUNCH_T(kernel, targs, ...)                                                     \
    do {                                                                                        \
        if (::dabgpu::trace_on()) ::dabgpu::trace_launch(#kernel, {DABGPU_TARGS targs});        \
        hipLaunchKernelGGL((kernel<DABGPU_TARGS targs>), __VA_ARGS__);                          \
    } while (0)
// The launch by FFT size: logN = 8 ... 11 as a compile-time constant L to f, whose result it returns; any other size is refused.
template <typename F> hipError_t by_fft_size(int logN, F &&f)
{
    switch (logN) {
    case 8: return f(std::integral_constant<int, 8>());
    case 9: return f(std::integral_constant<int, 9>());
    case 10: return f(std::integral_constant<int, 10>());
    case 11: return f(std::integral_constant<int, 11>());
    default: return hipErrorInvalidValue;
    }
}

// stream_probe.hip: streams on hardware queues of their own (the lanes of a context; the async host path's copy stream)
bool streams_overlap(hipStream_t a, hipStream_t b);
hipError_t create_stream_apart(const hipStream_t *others, int n, hipStream_t *out, bool *own);

struct GainParams {
    int mode;            // 0 fix, 1 max, 2 var
    float constant;      // normalise * digital  (reference src/GainControl.cpp:118)
    float var_variance;
    float var_c1;        // mode var: 32767 * constant / var_variance, formed in float64 (the fused kernel's multiplier is
                         // var_c1 / sqrt(exact variance): two roundings instead of seven)
    float var_c1_lo;     // var_c1 + var_c1_lo = the float64 value to 48 bits
    float var_sq;        // var_variance^2 (the "(int)(var_variance sigma) == 0" test on sigma^2)
};

// Arguments of the fused per-transmission-frame kernel.
struct TfArgs {
    Geometry g;
    Tables t;
    GainParams gain;
    int ntaps;
    int n_frames;
    int chunks_per_frame;
    int syms_per_chunk;
    const uint8_t *bits;      // FROM_BITS: n_frames * (nb_symbols-1)*K/4 bytes
    const float2 *carriers;   // else: n_frames * (nb_symbols+1)*K samples
    float2 *out;
    size_t out_stride;        // samples per frame in `out`
    float *gain1;             // FROM_BITS, optional: per frame, the multiplier applied to symbol 1 (TII)
    // TII inside the frame kernel (f-4; variants tf_has_tii names): the unit-gain response of the TII null symbol (its segment,
    // g.null_size samples), added -- times the multiplier of symbol 1 -- on the frames whose index parity says so
    // (TII::m_insert, src/TII.cpp:241-242).  nullptr: blank null symbol (launch_tii_add adds it afterwards, or TII is off).
    const float2 *tii_seg;
    int tii_insert0;          // frame 0 of this launch carries TII (then every other one)
    // TF_CFR: crest-factor reduction inside OfdmGenerator (f-3) and its statistics
    float cfr_clip, cfr_errclip;
    int cfr_mer_base;         // the MER symbol of frame f is (cfr_mer_base + f) % (nb_symbols + 1)
    unsigned *cfr_counts;     // [frame][2]: clipped samples, clipped errors (pre-zeroed)
    double *cfr_mer;          // [frame][2]: sum |before|^2, sum |after - before|^2 of the MER symbol (pre-zeroed)
    double *cfr_papr;         // [frame][nb_symbols+1][4]: peak, mean of |x|^2 before / after CFR (pre-zeroed)
    // TF_OUT_S16 / _U8 / _S8: `out` holds 4-byte s16 pairs / 2-byte u8 or s8 pairs; the number of clipped components is ADDED to *clipped
    unsigned long long *clipped;
    // TF_WINDOW: raised-cosine overlap of the guard interval (t.window holds the 2 * overlap factors)
    int overlap;
    // tool builds only (-DDABGPU_PHASE_TIMING, tools/phase_timing.py): 16 counters the symbol loop adds its per-phase
    // shader cycles to; nullptr (and ignored) in the product
    unsigned long long *phase_cycles;
};

enum TfFlags { TF_FROM_BITS = 1, TF_GAIN = 2, TF_GUARD = 4, TF_FIR = 8, TF_CFR = 16, TF_GVAR = 32 /* internal */,
               TF_OUT_S16 = 64, TF_WINDOW = 256, TF_EQ = 512, TF_OUT_U8 = 1024, TF_OUT_S8 = 2048 };
// the integer format the frame kernel is asked to store itself: 0 = none (complexf), else DABGPU_FMT_S16 / _U8 / _S8 (1 / 2 / 3)
inline int tf_ofmt(unsigned flags) { return (flags & TF_OUT_S16) ? 1 : (flags & TF_OUT_U8) ? 2 : (flags & TF_OUT_S8) ? 3 : 0; }
inline unsigned tf_ofmt_flag(int fmt) { return fmt == 1 ? TF_OUT_S16 : fmt == 2 ? TF_OUT_U8 : fmt == 3 ? TF_OUT_S8 : 0u; }

hipError_t launch_tf(const TfArgs &a, unsigned flags, hipStream_t s);
size_t tf_lds_bytes(int logN, unsigned flags, int nt = 0, int overlap = 0, int ntaps = 0);
int tf_max_fused_taps();   // longest FIR the fused kernel handles (longer ones take the unfused path)
bool tf_has_eq(const TfArgs &a, unsigned flags);     // the equalised-boundary variant exists for this chain (TF_EQ; needs t.eq_g)
bool tf_small45(const TfArgs &a, unsigned flags);    // modes II - IV: the chain is one of those built with the compile-time tap count
bool tf_has_window(const TfArgs &a, unsigned flags); // a frame-kernel variant windows the guard interval itself (TF_WINDOW)
bool tf_has_fmt(const TfArgs &a, unsigned flags);   // a frame-kernel variant stores the format of flags' TF_OUT_* bit itself
bool tf_has_tii(const TfArgs &a, unsigned flags);   // the variant these flags select adds the TII null symbol itself (a.tii_seg)

// Stand-alone stage kernels (per-stage drop-ins and the non-fused fallbacks).
hipError_t launch_qpsk(const uint8_t *in, size_t nbytes, int K, float2 *out, hipStream_t s);
hipError_t launch_freq_interleave(const float2 *in, size_t nsamples, int K,
                                  const uint16_t *src_carrier, float2 *out, hipStream_t s);
hipError_t launch_phase_reference(const uint8_t *phase_q, int K, float2 *out, hipStream_t s);
hipError_t launch_diff_mod(const float2 *phase, const float2 *data, size_t nsym_data, int K,
                           float2 *out, hipStream_t s);
hipError_t launch_gain(const float2 *in, size_t nsym, int N, GainParams gp, float2 *out,
                       hipStream_t s);
// gain mode var with the reference's running recurrence (chain calls under dabgpu_set_gain_rounding(ctx, 1)): x0 holds
// n_frames x nsym unscaled symbols of N samples; the multipliers are left in gains[n_frames * nsym] (symbol 1's also in gain1[frame]
// when given); apply: scale the symbols in place -- or leave that to the guard kernels below (their `gains` argument)
hipError_t launch_gain_replay(float2 *x0, size_t n_frames, int nsym, int N, GainParams gp, float *gains, float *gain1,
                              bool apply, hipStream_t s);
// (gains: optional, n_frames x (nb_symbols + 1) multipliers applied to the symbols as they are gathered -- symbol 0 with symbol 1's)
hipError_t launch_guard_copy(const float2 *in, size_t n_frames, Geometry g, float2 *out,
                             hipStream_t s, const float *gains = nullptr);
hipError_t launch_guard_window(const float2 *in, size_t n_frames, Geometry g, int overlap,
                               const float *window, float2 *out, hipStream_t s, const float *gains = nullptr);
// guard interval (copy or windowed) + FIR in one pass over the IFFT output ((nb_symbols+1) x N per frame).
// For this and launch_fir, `taps` is a HOST pointer to ntaps floats: they travel as a kernel argument.
hipError_t launch_guard_fir(const float2 *in, size_t n_frames, Geometry g, int overlap, const float *window,
                            const float *taps, int ntaps, float2 *out, hipStream_t s, const float *gains = nullptr);
hipError_t launch_fir(const float2 *in, size_t frame_samples, size_t n_frames, const float *taps,
                      int ntaps, float2 *out, hipStream_t s);
hipError_t launch_poly(const float2 *in, size_t nsamples, const float *am, const float *pm,
                       float2 *out, hipStream_t s);
// a12 CicEqualizer: out[i] = in[i] * filter[i % K]
hipError_t launch_cic(const float2 *in, size_t nsamples, int K, const float *filter, float2 *out, hipStream_t s);
// carriers.hip: coded bits -> the SignalMultiplexer output ([frame][nb_symbols + 1][K] cf32), with TII and CicEqualizer applied
struct CarrierArgs {
    Geometry g;
    Tables t;                 // src_carrier, phase_q, mag
    const uint8_t *bits;      // n_frames x (nb_symbols - 1) * K / 4 bytes, dword aligned
    float2 *out;
    int n_frames;
    const float *cic;         // K per-carrier factors, or nullptr: no CicEqualizer
    const uint8_t *acp;       // K: the TII carrier set A_{c,p} (tii_carrier_set), or nullptr: the null symbol is blank
    int tii_old_variant;
    int tii_insert0;          // frame 0 of this launch carries TII (then every other one)
};
hipError_t launch_carriers_from_bits(const CarrierArgs &a, hipStream_t s);
// demod.hip: native-rate IQ of whole transmission frames -> coded bits and per-frame quality figures (dabgpu_demod*, the monitor)
struct DemodFrameStats {                  // zeroed before the launch; every run of the frame adds its share
    double sum_signal, sum_quadrature;
    unsigned long long bit_errors;
    unsigned min_margin_inv;              // ~(bit pattern of the smallest margin so far); 0: no decision yet
    unsigned reserved;
};
// what the kernels that walk the data symbols of whole frames take (rx_symbols.h); the host fills it in fill_rx_symbols
struct RxSymbolArgs {
    Geometry g;
    Tables t;                 // twiddle, src_carrier
    const void *iq;           // n_frames x frame_stride samples: cf32 (fmt 0) or s16 pairs (fmt 1 = DABGPU_FMT_S16)
    int fmt;
    size_t frame_stride;      // samples per frame
    int n_frames;
    int runs_per_frame, syms_per_run;   // (demod_runs)
    int early;                // the FFT window ends this many samples before the end of the symbol; 0 ... sym_size - N
};
struct DemodArgs : RxSymbolArgs {
    uint8_t *bits_out;        // nullptr, or n_frames x (nb_symbols - 1) * K / 4 bytes, dword aligned
    const uint8_t *ref_bits;  // nullptr, or the same shape: differing bits are counted
    DemodFrameStats *stats;   // n_frames records
    int8_t *soft_out;         // nullptr (the hard kernel), or n_frames x (nb_symbols - 1) * 2 K soft metrics, dword aligned
    // the carrier state (dabgpu_demod_csi*): csi_sums set = the state pass alone (n_frames x K x (A, V) integers, zeroed
    // before the launch; nothing else is written); csi_w set with soft_out = the weighted soft kernel (n_frames x K fp32)
    unsigned long long *csi_sums;
    const float *csi_w;
};
void demod_runs(const Geometry &g, size_t n_frames, int forced, int *runs_per_frame, int *syms_per_run);
hipError_t launch_demod(const DemodArgs &a, hipStream_t s);
// the weights of n_frames frames from their carrier state (unit: every weight 1, dabgpu_debug_csi_unit_weights)
hipError_t launch_csi_weights(const unsigned long long *sums, float *w, int K, int n_frames, bool unit, hipStream_t s);
// sync.hip: the synchroniser (dabgpu_sync*): frame starts and carrier offset of a native-rate capture, and the frames extracted
constexpr int kSyncMaxShift = 31;         // integer carrier offsets searched: -max_shift ... max_shift, at most this
struct SyncHead {                         // written by the coarse kernel
    long long coarse0;                    // b* B: the coarse start of candidate 0
    int count;                            // candidate frames: coarse0 + (k + 1) tf <= n, at most `slots`
    int reserved;
    double null_depth;
    double reserved2;
};
struct SyncFrame {                        // one per candidate, the layout of dabgpu_sync_frame; zeroed before the launch
    long long start;
    int shift, valid;
    double eps, cfo_hz, quality, null_depth;
};
struct SyncArgs {
    Geometry g;
    Tables t;                 // twiddle, phase_q
    const void *iq;           // n samples: cf32 (fmt 0) or s16 pairs (fmt 1 = DABGPU_FMT_S16)
    int fmt;
    long long n;
    int max_shift;
    int slots;                // frame records (and frames of an extraction): min(max_frames, n / tf)
    float *power;             // nblk block powers (scratch)
    int nblk;                 // whole blocks of N / 32 samples in the first min(n, tf + null) samples
    SyncHead *head;
    SyncFrame *frames;
};
hipError_t launch_sync(const SyncArgs &a, hipStream_t s);
hipError_t launch_sync_extract(const SyncArgs &a, float2 *out, hipStream_t s);
// channel.hip: the channel emulator (dabgpu_channel*): sparse multipath, a Doppler rotation per path, seeded Gaussian noise
constexpr int kChMaxPaths = 64;           // DABGPU_CH_MAX_PATHS
constexpr int kChMaxDelay = 2047;         // DABGPU_CH_MAX_DELAY: the history holds this many input samples
constexpr int kChLane = 4;                // consecutive samples per lane
constexpr int kChTile = 256 * kChLane;    // samples per workgroup and pass
struct ChannelPath {
    uint32_t delay;
    float gr, gi;
    uint32_t reserved;
    unsigned long long step;              // rint(doppler_hz / rate_hz 2^64), two's complement
};
struct ChannelArgs {                      // by value in the kernel arguments: a new configuration is ordered behind what is queued
    const void *in;                       // n samples, in_fmt 0 (complexf) or 1 (s16 pairs)
    void *out;                            // n samples, out_fmt likewise
    const float2 *hist;                   // kChMaxDelay samples: hist[kChMaxDelay + j] = sample j < 0 of this call
    long long n;
    unsigned long long position;          // absolute index of sample 0
    int in_fmt, out_fmt;
    int n_static, n_paths;                // path[0 ... n_static - 1]: step = 0; path[n_static ... n_paths - 1]: step != 0
    int run;                              // samples per workgroup, a multiple of kChLane
    float sigma;
    uint32_t seed_lo, seed_hi;
    ChannelPath path[kChMaxPaths];
};
int channel_run(size_t n, int forced);
hipError_t launch_channel(const ChannelArgs &a, hipStream_t s);
// clock.hip: the clock's resampler (dabgpu_clock*): a sampling-clock offset put on a sample stream, or taken off it
constexpr int kClkTaps = 32;              // taps of the interpolator, tap kClkCentre on the input position
constexpr int kClkCentre = 15;
constexpr int kClkPhases = 512;           // rows 0 ... 512 of the tap table
constexpr int kClkHist = 31;              // the history holds this many input samples
constexpr int kClkMaxRun = 2048;          // outputs per workgroup at most (the staged input span: kClkSpan samples of LDS)
constexpr int kClkSpan = kClkMaxRun + kClkMaxRun / 999 + 1 + kClkTaps;
struct ClockArgs {
    const void *in;                       // n samples, in_fmt 0 (complexf) or 1 (s16 pairs)
    void *out;                            // count samples, out_fmt likewise
    const float2 *hist;                   // kClkHist samples: hist[kClkHist + r] = sample r < 0 of this call
    const float2 *tab;                    // [kClkPhases][kClkTaps]: (T[p][j], T[p + 1][j] - T[p][j])
    long long n;
    unsigned long long T;                 // absolute index of input sample 0 of the call
    unsigned long long m0;                // absolute index of the call's first output
    long long count;                      // outputs of the call
    long long step;                       // llrint(ppm 1e-6 2^64)
    int in_fmt, out_fmt;
    int run;                              // outputs per workgroup, 1 ... kClkMaxRun
};
int clock_run(size_t count, int forced);
hipError_t launch_clock(const ClockArgs &a, hipStream_t s);
// clock.hip, the estimator (dabgpu_sco*): per data block of whole frames the sums of e = d conj(c) over either half of the
// carriers and of |e|, in the receiver's geometry (demod_runs); then the blocks of a frame in index order
constexpr int kScoSums = 5;               // Re A_hi, Im A_hi, Re A_lo, Im A_lo, S
struct ScoArgs : RxSymbolArgs {
    double *rows;             // n_frames x (nb_symbols - 1) x kScoSums: every block's sums
    double *frames;           // n_frames x kScoSums: the frames' sums
};
hipError_t launch_sco(const ScoArgs &a, hipStream_t s);
// tuner.hip: the tuner (dabgpu_tuner*): mixer, channel filter and rational decimator L / M from any capture rate to the native one
constexpr int kTunMaxL = 512;             // rows of the tap table at most
constexpr int kTunMaxTaps = 768;          // taps per output at most: 96 x ceil(M / L), M <= 8 L
constexpr int kTunMaxHist = kTunMaxTaps - 1;
constexpr int kTunSpan = 5120;            // samples of LDS a workgroup stages its input span in (40 KB)
constexpr int kTunMaxRun = 2048;          // outputs per workgroup at most (fewer where the span does not hold them: tuner_run_max)
struct TunerArgs {
    const void *in;                       // n samples, in_fmt 0 (complexf), 1 (s16 pairs), 2 (u8 pairs, byte - 128), 3 (s8 pairs)
    void *out;                            // count samples, out_fmt 0 or 1
    const float2 *hist;                   // P - 1 samples as floats, not mixed: hist[P - 1 + r] = sample r < 0 of this call
    const float *tab;                     // [L][P]
    long long n;
    unsigned long long T;                 // absolute index of input sample 0 of the call
    unsigned long long m0;                // absolute index of the call's first output
    long long count;                      // outputs of the call
    unsigned long long step;              // the mixer's turns per input sample x 2^64 (two's complement); 0: no mixer
    int L, M, P;
    int in_fmt, out_fmt;
    int run;                              // outputs per workgroup, 1 ... tuner_run_max
};
int tuner_run_max(int L, int M, int P);
int tuner_run(int L, int M, int P, int forced);
hipError_t launch_tuner(const TunerArgs &a, hipStream_t s);
// stream_history.hip: the history behind a call of the three stages above (H = kChMaxDelay, kClkHist, the tuner's P - 1):
// next[j] = sample n - H + j of the call, in_fmt 0 ... 3 as TunerArgs, from `in` or (calls shorter than H) from `cur`
constexpr int kStreamMaxHist = kChMaxDelay;
static_assert(kClkHist <= kStreamMaxHist && kTunMaxHist <= kStreamMaxHist, "the largest history in use");
hipError_t launch_stream_history(const void *in, int in_fmt, long long n, int H, const float2 *cur, float2 *next, hipStream_t s);
// tii_scan.hip: the TII analyser (dabgpu_tii_scan*): which (comb, pattern) the null symbols of whole frames carry, the level
// and the delay of every comb
constexpr int kTiiCombs = 24;             // combs, and entry slots of a result
constexpr int kTiiCells = 192;            // cells (c, b): 24 combs x 8 pattern bits, cell (c, b) at 8 c + b
constexpr int kTiiGrid = 16384;           // the fine delay's grid: N / 16384 samples
struct TiiScanHead {                      // the layout of dabgpu_tii_scan_head; written by the decide kernel
    int n_used, parity, n_entries, reserved;
    double floor, total[2];
};
struct TiiEntry {                         // the layout of dabgpu_tii_entry; zeroed before the launch
    int comb, pattern, mask, n_set;
    double energy, delay_coarse, delay, runner_up;
};
struct TiiScanArgs {
    Geometry g;
    Tables t;                 // twiddle, phase_q
    const void *iq;           // n_frames x tf samples: cf32 (fmt 0) or s16 pairs (fmt 1 = DABGPU_FMT_S16)
    int fmt;
    int n_frames;
    int early, old_variant;
    float min_ratio, min_rel;
    double *rows;             // scratch, n_frames x 3 x kTiiCells: E_f, Re G_f, Im G_f
    float2 *bins;             // scratch, n_frames x K: the occupied bins of every frame's null symbol
    TiiScanHead *head;
    TiiEntry *entries;        // kTiiCombs slots
    int *centre;              // kTiiCombs: rint(tau1 / s) of every entry, from the decide kernel to the delay kernel
};
hipError_t launch_tii_scan(const TiiScanArgs &a, hipStream_t s);
// cir.hip: the channel estimator (dabgpu_cir*): the impulse response a capture's phase reference symbols went through, its
// echoes with level and delay, and the response on the carriers
constexpr int kCirMaxPaths = 16;          // DABGPU_CIR_MAX_PATHS: path slots of a result
struct CirHead {                          // the layout of dabgpu_cir_head; written by the decide kernel
    int n_frames, n_peaks, n_paths, window, peak_index, resp_min_bin, resp_max_bin, reserved;
    double floor, threshold, peak, total, path_power, mean_delay, delay_spread, first_delay, outside_guard, resp_mean, resp_min,
        resp_max;
};
struct CirPath {                          // the layout of dabgpu_cir_path; zeroed before the launch
    int index, reserved;
    double delay, fine, power;
};
struct CirArgs {
    Geometry g;
    Tables t;                 // phase_q
    const void *iq;           // n_frames x tf samples: cf32 (fmt 0) or s16 pairs (fmt 1 = DABGPU_FMT_S16)
    int fmt;
    int n_frames;
    int early, window;
    float min_ratio, min_rel;
    double sum_w;             // S_w: the sum of the K weights in ascending carrier order
    double *rows;             // scratch, n_frames x 2 N: |h_f|^2 per tap, then |H_f|^2 per bin
    CirHead *head;
    CirPath *paths;           // kCirMaxPaths slots
    double *pdp, *resp;       // N each
};
hipError_t launch_cir(const CirArgs &a, hipStream_t s);
// welch.h: what the two Welch launches share -- the run geometry (spectrum_runs), the table, the rows and the sums
struct WelchArgs {
    long long n_segments;     // the segments used: one range, every lane sees the same
    int n_runs, segs_per_run; // (spectrum_runs)
    const float2 *twiddle;    // exp(+2 pi i m / 2048), 2048 entries
    double *rows;             // scratch, n_runs rows: a workgroup's partial sums, bins in FFT order
    double *acc;              // the sums (a row's width), then the segment count as one unsigned long long
};
// what either launch checks of them first (spectrum.hip)
hipError_t check_welch(const WelchArgs &a, int max_runs);
// spectrum.hip: Welch periodogram of one sample buffer (dabgpu_spectrum*, the spectrum monitor): segments of SPECTRUM_NFFT
// samples at a hop of half that, in every transmission mode.  n_segments: welch_n_segments.  A row is 2048 sums.
struct SpectrumArgs : WelchArgs {
    const void *iq;           // the samples: cf32 (fmt 0), s16 pairs (1), u8 pairs, value byte - 128 (2), s8 pairs (3)
    int fmt;
    const float *window;      // 2048 fp32 factors
    int accumulate;           // the reduce kernel adds to acc (else stores)
};
hipError_t launch_spectrum(const SpectrumArgs &a, hipStream_t s);
// dpd.hip: the predistortion measurement (dabgpu_dpd_*).  The cross-spectrum is the spectrum kernel's walk over two buffers
// (welch.h), rectangular window; a row is 4 x 2048 sums: Re S, Im S, P_tx, P_rx.
enum { DPD_TAPS = 32, DPD_TAP_CENTRE = 15, DPD_MAX_BINS = 256, DPD_TILE_MAX = 2048, DPD_FIGURES = 6 };
struct DpdXspecArgs : WelchArgs {
    const void *tx;           // cf32 (fmt 0) or s16 pairs (fmt 1)
    int fmt;
    const float2 *rx;         // cf32; segment i of rx is samples 1024 i + rx_offset ... + 2047
    long long rx_offset;
    long long seg_first;      // the first segment whose rx range lies inside the buffer; n_segments follow it (dpd_segments)
};
// (n_samples: of either buffer; the launch checks the range of segments in `a` against it)
hipError_t launch_dpd_xspectrum(const DpdXspecArgs &a, size_t n_samples, hipStream_t s);
struct DpdStatsArgs {
    const void *tx;           // cf32 (fmt 0) or s16 pairs (fmt 1)
    int fmt;
    const float2 *rx;
    long long n, lag;         // samples in either buffer; the aligned rx sample of i is centred on rx[i + lag]
    long long i_first, i_end; // the samples used: all 32 taps inside rx (launch_dpd_stats forms the range, dpd_used_range)
    long long tile_first;     // the tile of workgroup 0 (launch_dpd_stats: the tile that holds i_first)
    float h[DPD_TAPS];        // fractional-delay taps (dabgpu_dpd_delay_taps)
    float g_re, g_im;         // complex gain on the filtered rx sample
    float peak;               // amplitudes are counted in units of peak 2^-24
    int n_bins;
    const float *edge2;       // n_bins + 1 squared bin edges, fp32
    int tile;                 // samples per workgroup: a multiple of 256, at most DPD_TILE_MAX
    unsigned long long *sums; // DPD_MAX_BINS x DPD_FIGURES integers, then overflow and samples used
};
void dpd_used_range(long long n, long long lag, long long *i_first, long long *i_end);
hipError_t launch_dpd_stats(DpdStatsArgs a, hipStream_t s);
// f-4 TII: the sparse symbol (stand-alone stage), and its addition to a stream whose null symbol is blank
hipError_t launch_tii(const float2 *in, const uint8_t *acp, int K, int old_variant, int insert, float2 *out,
                      hipStream_t s);
hipError_t launch_tii_add(float2 *out, size_t stride, const float2 *seg, int seg_len, const float *gain1,
                          int insert0, size_t n_frames, hipStream_t s);
// f-2 FormatConverter: fmt 1 = s16, 2 = u8, 3 = s8; *clipped (device) is incremented
hipError_t launch_format(const float *in, size_t nfloats, int fmt, void *out, unsigned long long *clipped,
                         hipStream_t s);
hipError_t launch_lut(const float2 *in, size_t nsamples, float scale, const float *lut,
                      float2 *out, hipStream_t s);

// The front-end (frontend.hip).  FeUnit, a unit's place in the frame and its puncturing segments: conv_code.h.
struct FeArgs {
    const uint8_t *eti;                   // n_eti x 6144
    const uint8_t *prbs;                  // kFeCifBytes: the x^9 + x^5 + 1 sequence
    const FeUnit *units;
    const int16_t *owner;                 // 864: which sub-channel a capacity unit belongs to (the last in STC order), -1 padding
    uint8_t *hist;                        // (kFeHistory + n_eti) x kFeCifBytes
    uint8_t *fic;                         // n_eti x fic_out
    uint8_t *out;                         // n_tf x cifs x (fic_out + kFeCifBytes)
    int n_eti, n_units, cifs, fic_out;
    // the encode launch: the first unit it runs and the history row frame 0 goes to.  0 and kFeHistory in a call that
    // produces output (FIC and sub-channels, rows 15 ...); 1 and r0 <= kFeHistory - n_eti for a seed: the sub-channel units
    // alone, straight into rows r0 ... r0 + n_eti - 1 of the history
    int unit0, row0;
};
hipError_t launch_fe_encode(const FeArgs &a, hipStream_t s);
hipError_t launch_fe_assemble(const FeArgs &a, hipStream_t s);

// The channel decoder (decode.hip): the front-end backwards, from the tables the front-end uploads.  A received row is the
// punctured FIC of one ETI frame followed by its CIF (fic_out + kFeCifBytes bytes); `rows` holds the fifteen rows before the
// call (the decoder's history) and the call's n rows behind them.  Output i of a call is decoded from rows i ... i + 15.
constexpr int kDecThreads = 64;           // one wave: lane = state of the K = 7 code
constexpr int kDecMaxSteps = 48 * 1024;   // trellis steps of one unit the kernel's LDS holds (a frame's payload gives < 48 294)
struct DecUnitStats {                     // per (output, unit); plain stores, every record of a launch is written
    uint32_t corrected, coded_bits, bit_errors, n_bits;
};
struct DecSoftUnitStats {
    uint32_t metric, contra_sum, soft_sum, corrected, erasures, coded_bits, bit_errors, n_bits;
};
// One struct for either metric width, hard (In = uint8_t: coded bits, rows of fic_out + kFeCifBytes bytes) and soft (In =
// int8_t: one metric per coded bit, rows eight times as long); survivor scratch and slots are shared
template <typename In, typename Stats>
struct DecArgsT {
    const In *in;                         // n_tf transmission frames in the chain's input layout, soft: x 8 (dword aligned)
    In *rows;                             // (kFeHistory + n_out) rows
    const uint8_t *prbs;
    const FeUnit *units;
    const uint32_t *slot;                 // n_units + 1: where a unit's survivor words start inside an output's scratch
    unsigned long long *surv;             // n_out x slot[n_units] survivor words
    uint8_t *out;                         // n_out x 6144, zeroed before the launch
    const uint8_t *ref;                   // nullptr, or n_out x 6144
    Stats *stats;                         // n_out x n_units
    int n_out, n_units, cifs, fic_out;
    // what sizes the workgroup's LDS.  Hard: the steps of the layout's longest unit, rounded up to 64.  Soft: 8 x out_bytes
    // of the layout's largest unit, the punctured softs a workgroup stages
    int lds_bytes;
    int first_valid;                      // outputs before this one lie before the start of the stream: nothing is decoded
};
using DecArgs = DecArgsT<uint8_t, DecUnitStats>;
using DecSoftArgs = DecArgsT<int8_t, DecSoftUnitStats>;
hipError_t launch_dec_rows(const DecArgs &a, hipStream_t s);
hipError_t launch_dec_rows(const DecSoftArgs &a, hipStream_t s);
hipError_t launch_dec_decode(const DecArgs &a, hipStream_t s);
hipError_t launch_dec_decode(const DecSoftArgs &a, hipStream_t s);

// Resampler (reference src/Resampler.cpp:131-195), power-of-two FFT sizes.
struct ResamplerArgs {
    int nin, nout;          // FFT sizes (e.g. 4096 -> 16384)
    float factor;
    const float *window;    // nin
    const float2 *tw_in;    // nin entries exp(+2 pi i m / nin)
    const float2 *tw_out;   // nout entries
    const float2 *in;       // nhops * nin/2 samples (one stream)
    const float2 *halo;     // nin samples: the two hops before `in` (zeros at stream start)
    float2 *halo_out;       // non-null (the x2 / x4 kernel at nin = 4096 only, see resampler_writes_halo): the kernel leaves the
                            // last two hops of [halo | in] there -- the next call's halo -- instead of a copy launched behind it
    float2 *out;            // nhops * nout/2
    const float *poly;      // nullptr, or am[5] at [0..4] and pm[5] at [8..12]: MemlessPoly fused into the store
    unsigned long long *clipped;   // non-null: store s16 pairs (FormatConverter fused, x2 / x4 kernels with nin = 4096)
    size_t nhops;
    // rational ratios L/M (the general kernel): nout = (nin / M) * L
    int L, M;
    const float2 *tw_s;     // nin / M entries exp(+2 pi i m / (nin / M))
    const float2 *tw_l;     // L entries exp(+2 pi i m / L)
    int run_hops;           // hops per workgroup, forced (dabgpu_debug_resampler_run_hops); 0: by the call size (resampler_runs.h)
};
hipError_t launch_resampler(const ResamplerArgs &a, hipStream_t s);
bool resampler_has_s16(const ResamplerArgs &a);
// the geometry of the calling thread's most recent resampler launch (the launchers note it; run_resampler keeps it in the context
// for dabgpu_debug_resampler_last_launch)
void note_resampler_launch(int hops_per_run, unsigned grid);
void resampler_last_launch(int *hops_per_run, unsigned *grid);
bool resampler_writes_halo(const ResamplerArgs &a);   // the kernel this geometry runs honours halo_out

}  // namespace dabgpu
