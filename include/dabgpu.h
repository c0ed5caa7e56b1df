/*
 * dabgpu.h -- C-ABI of the MI355X-native DAB COFDM hot path (libdabgpu.so).
 *
 * This is the drop-in boundary: plain C, no exceptions, no C++/torch types.
 * Every stage entry point replaces the `process()` of one ODR-DabMod flowgraph
 * plugin (reference file:line cited at each declaration); the C++ adapters in
 * odr-dabmod_amd/host/ keep the reference's ModPlugin class names and
 * constructor signatures and call these functions (INTEGRATION.md shows the
 * binding a maintainer adds to src/DabModulator.cpp).
 *
 * Conventions
 *   - return 0 on success, <0 on error (DABGPU_E_*); dabgpu_last_error(ctx)
 *     gives the message the adapter throws as std::runtime_error, mirroring
 *     the reference's own size-check throws.
 *   - samples are interleaved (re,im) float32 == std::complex<float>
 *     (reference src/Buffer.h:40).
 *   - `*_process` take HOST pointers (what a ModPlugin's Buffer holds) and
 *     stage through pinned memory; `*_dev` take DEVICE pointers plus a HIP
 *     stream handle (hipStream_t cast to void*, NULL = the context's stream)
 *     and are asynchronous on that stream.
 *   - out_cap is the capacity of the output buffer in bytes; *out_bytes
 *     receives the produced length (the producer sizes its output, like
 *     Buffer::setLength at the top of every reference process()).
 *   - setters may be called from another thread (remote-control thread in the
 *     reference); they take effect at the next *_process call.
 *   - There is NO CPU fallback: every entry point fails with
 *     DABGPU_E_DEVICE when no gfx950 device/kernel is available.
 */
#ifndef DABGPU_H
#define DABGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DABGPU_API __attribute__((visibility("default")))

enum {
    DABGPU_OK = 0,
    DABGPU_E_INVALID = -1, /* bad argument / size check failed (reference throws std::runtime_error) */
    DABGPU_E_DEVICE = -2,  /* HIP error, no device, kernel image missing */
    DABGPU_E_NOMEM = -3,
    DABGPU_E_CAPACITY = -4 /* out_cap too small / n_frames > max_frames */
};

/* GainMode, reference src/GainControl.h:45 */
enum { DABGPU_GAIN_FIX = 0, DABGPU_GAIN_MAX = 1, DABGPU_GAIN_VAR = 2 };

/* stage mask for the fused chain (order of src/DabModulator.cpp:385-419).
 * QPSK map, frequency interleave, differential modulation, signal mux, OFDM
 * IFFT and guard-interval insertion always run. */
enum {
    DABGPU_STAGE_GAIN = 1u << 0,     /* GainControl   */
    DABGPU_STAGE_FIR = 1u << 1,      /* FIRFilter     */
    DABGPU_STAGE_RESAMPLE = 1u << 2, /* Resampler     */
    DABGPU_STAGE_POLY = 1u << 3,     /* MemlessPoly   */
    DABGPU_STAGE_NOGUARD = 1u << 8   /* stop after OfdmGenerator(+GainControl): no guard interval */
};

typedef struct dabgpu_ctx dabgpu_ctx;

typedef struct {
    int mode;          /* transmission mode 1..4 (src/DabModulator.cpp:84-122); 0 = IV, as the stage classes
                        * read it (src/PhaseReference.cpp:72-76, src/FrequencyInterleaver.cpp:57-58) */
    int device;        /* HIP device ordinal */
    int max_frames;    /* largest n_frames of a *_process call (scratch sizing); 0 -> 1 */
    int chunks_per_frame; /* workgroups per transmission frame for the fused kernel; 0 = auto */
} dabgpu_config;

DABGPU_API int dabgpu_create(const dabgpu_config *cfg, dabgpu_ctx **out);
DABGPU_API void dabgpu_destroy(dabgpu_ctx *ctx);
DABGPU_API const char *dabgpu_last_error(const dabgpu_ctx *ctx); /* ctx may be NULL: last create error */
DABGPU_API const char *dabgpu_version(void);

/* geometry of the configured mode (src/DabModulator.cpp:84-122) */
typedef struct {
    int mode, nb_symbols, carriers, spacing, null_size, sym_size;
    size_t tf_input_bytes; /* hot-path input per transmission frame (BlockPartitioner output) */
    size_t tf_samples;     /* complex samples per transmission frame at the native rate */
} dabgpu_geometry;
DABGPU_API int dabgpu_get_geometry(const dabgpu_ctx *ctx, dabgpu_geometry *g);

/* ---- runtime parameters (remote-control setters of the reference) -------- */

/* GainControl::set_parameter digital/mode/var, src/GainControl.cpp:505-554; normalise is the
 * constructor argument derived from the sink, src/DabMod.cpp:259-347 */
DABGPU_API int dabgpu_set_gain(dabgpu_ctx *ctx, int gain_mode, float digital, float normalise,
                               float var_variance);
/* How a CHAIN call forms the multiplier of gain mode var (computeGainVar, src/GainControl.cpp:251-340).  The reference walks a
 * symbol with four fp32 running means and four running variances (mean += (x - mean) / count), 2 x N/2 dependent divisions
 * whose rounding error (up to 5.8e-7 relative, tests/test_oracle_golden.py) is part of its output.
 *   DABGPU_GAIN_ROUNDING_EXACT (default): the exact population variance inside the frame kernel -- closer to the arithmetic
 *     the reference approximates, 5.8 ... 6.2e-7 from ITS scalar, one kernel per chain call.
 *   DABGPU_GAIN_ROUNDING_REFERENCE: the reference's recurrence operation for operation, as the stand-alone stage
 *     (dabgpu_gain_process) does: the frame kernel stops after OfdmGenerator, a kernel of four lanes per symbol replays the
 *     recurrence, and the guard interval / FIRFilter run as kernels of their own that scale the symbols as they read them.  The gain
 *     scalars then equal the reference's bit for bit on the same symbols (along a chain: within 2.3e-7, the recurrence's own
 *     sensitivity to the last bits of its input; chain total 2.5e-7 instead of 6.3e-7); cfg 3 runs at about 30 % of its rate.
 * No effect on gain modes fix and max (their scalars are exact either way).  Takes effect at the next *_process call. */
enum { DABGPU_GAIN_ROUNDING_EXACT = 0, DABGPU_GAIN_ROUNDING_REFERENCE = 1 };
DABGPU_API int dabgpu_set_gain_rounding(dabgpu_ctx *ctx, int rounding);
/* FIRFilter::load_filter_taps, src/FIRFilter.cpp:95-141 (n <= 512; up to 128 taps run fused) */
DABGPU_API int dabgpu_set_fir_taps(dabgpu_ctx *ctx, const float *taps, size_t n);
/* FIRFilter("default"): the built-in 45 taps, src/FIRFilter.cpp:59-71 */
DABGPU_API int dabgpu_set_fir_default_taps(dabgpu_ctx *ctx);
/* GuardIntervalInserter::update_window, src/GuardIntervalInserter.cpp:96-113.  (The fused chain windows overlaps up to 128
 * samples inside the frame kernel; up to 10 on the Mode I chain with a filter of up to the default length it stays the
 * one-transform-per-symbol kernel of that chain.) */
DABGPU_API int dabgpu_set_window_overlap(dabgpu_ctx *ctx, size_t overlap);
/* Resampler(inputRate, outputRate, resolution = spacing), src/Resampler.cpp:51-112;
 * resets the stream state at the next *_process call: the halo (the last two hops of native-rate
 * input, which live in the context's device memory) to zeros and nothing else -- the TII frame
 * parity is not the Resampler's.  The state is read, installed and computed from outside with
 * dabgpu_get_stream_state / dabgpu_set_stream_state / dabgpu_chain_seed ("stream state" below).  Built: every ratio L / M (the
 * rates reduced by their gcd) with M a power of two up to the FFT size -- up- AND down-sampling
 * (1.024, 1.536, 2.4, 3.072, 4.096, 6.144, 8.192 ... Msps in Mode I; x2 and x4 have their own
 * faster kernel).  Any other ratio is refused HERE with DABGPU_E_INVALID (the reference's own
 * hop loop cannot run those on whole transmission frames). */
DABGPU_API int dabgpu_set_resampler(dabgpu_ctx *ctx, size_t in_rate, size_t out_rate);
/* MemlessPoly::load_coefficients format 1, src/MemlessPoly.cpp:154-202 */
DABGPU_API int dabgpu_set_poly(dabgpu_ctx *ctx, const float am[5], const float pm[5]);
/* MemlessPoly::load_coefficients format 2, src/MemlessPoly.cpp:203-226 */
DABGPU_API int dabgpu_set_lut(dabgpu_ctx *ctx, float scalefactor, const float lut[32]);

/* ---- per-stage entry points (HOST buffers; one per reference plugin) ----- */

/* QpskSymbolMapper::process, src/QpskSymbolMapper.cpp:39-213 */
DABGPU_API int dabgpu_qpsk_process(dabgpu_ctx *ctx, const void *in, size_t in_bytes, void *out,
                                   size_t out_cap, size_t *out_bytes);
/* FrequencyInterleaver::process, src/FrequencyInterleaver.cpp:128-145 */
DABGPU_API int dabgpu_freq_interleave_process(dabgpu_ctx *ctx, const void *in, size_t in_bytes,
                                              void *out, size_t out_cap, size_t *out_bytes);
/* PhaseReference::process, src/PhaseReference.cpp:174-190 */
DABGPU_API int dabgpu_phase_reference_process(dabgpu_ctx *ctx, void *out, size_t out_cap,
                                              size_t *out_bytes);
/* DifferentialModulator::process, src/DifferentialModulator.cpp:80-108 (in0 phase ref, in1 data) */
DABGPU_API int dabgpu_diff_mod_process(dabgpu_ctx *ctx, const void *phase, size_t phase_bytes,
                                       const void *data, size_t data_bytes, void *out,
                                       size_t out_cap, size_t *out_bytes);
/* NullSymbol::process src/NullSymbol.cpp:49-57 */
DABGPU_API int dabgpu_null_symbol_process(dabgpu_ctx *ctx, void *out, size_t out_cap,
                                          size_t *out_bytes);
/* SignalMultiplexer::process, src/SignalMultiplexer.cpp:45-71: out = first ++ rest */
DABGPU_API int dabgpu_signal_mux_process(dabgpu_ctx *ctx, const void *first, size_t first_bytes,
                                         const void *rest, size_t rest_bytes, void *out,
                                         size_t out_cap, size_t *out_bytes);
/* OfdmGeneratorCF32::process, src/OfdmGenerator.cpp:157-308 (CFR off) */
DABGPU_API int dabgpu_ofdm_process(dabgpu_ctx *ctx, const void *in, size_t in_bytes, void *out,
                                   size_t out_cap, size_t *out_bytes);
/* GainControl::internal_process, src/GainControl.cpp:82-192 */
DABGPU_API int dabgpu_gain_process(dabgpu_ctx *ctx, const void *in, size_t in_bytes, void *out,
                                   size_t out_cap, size_t *out_bytes);
/* GuardIntervalInserter::process, src/GuardIntervalInserter.cpp:325-336 */
DABGPU_API int dabgpu_guard_process(dabgpu_ctx *ctx, const void *in, size_t in_bytes, void *out,
                                    size_t out_cap, size_t *out_bytes);
/* FIRFilter::internal_process, src/FIRFilter.cpp:144-309 (any length, one frame per call) */
DABGPU_API int dabgpu_fir_process(dabgpu_ctx *ctx, const void *in, size_t in_bytes, void *out,
                                  size_t out_cap, size_t *out_bytes);
/* Resampler::process, src/Resampler.cpp:131-195 (stateful across calls) */
DABGPU_API int dabgpu_resampler_process(dabgpu_ctx *ctx, const void *in, size_t in_bytes,
                                        void *out, size_t out_cap, size_t *out_bytes);
/* MemlessPoly::internal_process, src/MemlessPoly.cpp:342-411 */
DABGPU_API int dabgpu_poly_process(dabgpu_ctx *ctx, const void *in, size_t in_bytes, void *out,
                                   size_t out_cap, size_t *out_bytes);

/* Crest-factor reduction inside OfdmGenerator: the constructor arguments / RC
 * parameters cfr, clip, errorclip of OfdmGeneratorCF32 (src/OfdmGenerator.h:50-56, .cpp:376-404).
 * When enabled every symbol is clipped, transformed forward, its error against the input
 * constellation clipped, and transformed back (cfr_one_iteration, src/OfdmGenerator.cpp:310-373),
 * in dabgpu_ofdm_process and in the chain entry points alike.  Any float is taken, as by the reference's remote control: the
 * thresholds act through their squares (a negative one is its magnitude), 0 clips every non-zero sample (bin) to 0, one whose
 * square overflows clips nothing; the output stays finite where |x|^2 is subnormal (tests/test_cfr_gpu.py). */
DABGPU_API int dabgpu_set_cfr(dabgpu_ctx *ctx, int enable, float clip, float error_clip);
/* Per-frame raw statistics of the most recent call that ran with CFR on (frame = index inside that
 * call); the reference's running averages (clip_stats, papr: src/OfdmGenerator.cpp:285-306,419-451,
 * src/PAPRStats.cpp) are formed from these by the caller.  Waits for the call to finish. */
typedef struct dabgpu_cfr_stats {
    uint64_t num_clip, num_error_clip; /* samples / errors clipped in the frame (:275-276) */
    uint64_t num_samples;              /* nbSymbols * spacing (:286) */
    int mer_symbol;                    /* myMERCalcIndex of this frame (:198); 0 = no MER pushed (:250) */
    double mer_sum_iq, mer_sum_delta;  /* the two sums of :262-266 for that symbol */
    int nb_symbols;                    /* entries used below (transmission-frame symbols incl. null) */
    double papr_before[154][2];        /* per symbol {peak, mean} of |x|^2 before CFR (PAPRStats::process_block) */
    double papr_after[154][2];         /* after CFR; symbol 0 is not measured (:246-248) */
} dabgpu_cfr_stats;
DABGPU_API int dabgpu_get_cfr_stats(dabgpu_ctx *ctx, size_t frame, dabgpu_cfr_stats *out);

/* TII.  dabgpu_set_tii = tii_config_t + the RC parameters enable / comb / pattern /
 * old_variant (src/TII.h:42-69, src/TII.cpp:339-372); invalid mode (only I and II carry TII), comb
 * outside [0,23] or pattern outside [0,69] is DABGPU_E_INVALID with the reference's TIIError text
 * (src/TII.cpp:119-150).  In the fused chain (dabgpu_chain_process*) an enabled TII replaces the
 * null symbol on every other frame of the stream, starting with the first (TII::m_insert,
 * src/TII.h:112, src/TII.cpp:226-242); the frame parity is per context and advances whether or
 * not TII is enabled, like the reference's.
 * dabgpu_tii_process = TII::process, src/TII.cpp:213-245: `in` is the PhaseReference symbol
 * (carriers x cf32), out the TII symbol or zeros; each call toggles the insert flag. */
DABGPU_API int dabgpu_set_tii(dabgpu_ctx *ctx, int enable, int comb, int pattern, int old_variant);
DABGPU_API int dabgpu_tii_process(dabgpu_ctx *ctx, const void *in, size_t in_bytes, void *out,
                                  size_t out_cap, size_t *out_bytes);

/* CicEqualizer(nbCarriers, spacing, R)::process, src/CicEqualizer.cpp:29-91: every
 * symbol of `carriers` samples times the per-carrier compensation gain of an R-fold, 4-stage CIC
 * interpolator.  The stage drop-in; in the fused chain it is a setting, dabgpu_set_cic_equalizer below (the reference wires it in
 * only when an FPGA clockRate is configured, src/DabModulator.cpp:154-176). */
DABGPU_API int dabgpu_cic_equalizer_process(dabgpu_ctx *ctx, size_t spacing, int R, const void *in,
                                            size_t in_bytes, void *out, size_t out_cap,
                                            size_t *out_bytes);
/* CicEqualizer inside the fused chain: the reference's decision to wire it in (src/DabModulator.cpp:155-176: a configured
 * dac_clk_rate gives cic_ratio = clockRate / outputRate / 4 and the constructor arguments (carriers, spacing * outputRate /
 * 2048000, cic_ratio)) stays with the caller; this is its result.  enable = 0 (the default): no equaliser, spacing and R are
 * ignored.  enable with spacing == 0 or R <= 0 is DABGPU_E_INVALID with the stage entry's message.  While it is on, every chain
 * call (dabgpu_chain_process / _process_dev / _submit / _process_eti / _submit_eti, the seeds) runs carriers first: ONE kernel
 * forms the equalised carriers of the call's frames from the coded bits -- cifMap ... cifSig with the TII symbol in place of
 * the null symbol on the frames that carry it, times the per-carrier factor as CicEqualizer::process does
 * (src/CicEqualizer.cpp:66-91) -- and the from-carriers chain (what dabgpu_symbols_process_dev runs) does the rest, with every
 * gain mode, filter, window, CFR, resampler, predistorter and output format; dabgpu_symbols_process_dev equalises the carriers
 * it is handed (the reference's cifCicEq sits behind cifSig, :399).  The stage entry above keeps a table of its own.  The
 * table is a setting like the taps: it takes effect at the next *_process call, after the context has drained. */
DABGPU_API int dabgpu_set_cic_equalizer(dabgpu_ctx *ctx, int enable, size_t spacing, int R);
/* Coded bits -> the SignalMultiplexer output, (nb_symbols + 1) x carriers cf32 per frame in the order
 * dabgpu_symbols_process_dev takes: the sub-graph cifMap -> cifFreq -> cifDiff(+cifRef) -> cifSig(+NullSymbol / TII)
 * [-> cifCicEq] of src/DabModulator.cpp:385-399 in one kernel, bit for bit the reference's classes
 * (QpskSymbolMapper::process, src/QpskSymbolMapper.cpp:39-213 ... CicEqualizer::process, src/CicEqualizer.cpp:66-91).  With
 * the context's TII and CIC settings; consecutive frames of the stream: advances the TII frame parity like a chain call.
 * in_bytes: a whole number of frames of tf_input_bytes, anything else is DABGPU_E_INVALID. */
DABGPU_API int dabgpu_carriers_process(dabgpu_ctx *ctx, const uint8_t *bits, size_t in_bytes, void *out, size_t out_cap,
                                       size_t *out_bytes);
/* same (src/DabModulator.cpp:385-399), device-resident and asynchronous on `stream` (NULL: the context's own stream, behind every lane) */
DABGPU_API int dabgpu_carriers_process_dev(dabgpu_ctx *ctx, const void *d_bits, size_t n_frames, void *d_carriers,
                                           size_t out_cap, size_t *out_bytes, void *stream);

/* FormatConverter::process, float input path, src/FormatConverter.cpp:111-178:
 * cf32 -> interleaved s16 / u8 / s8 with the reference's range test, truncation toward zero and
 * count of clipped components (FormatConverter::get_num_clipped_samples, :186-189).
 * An unknown format is DABGPU_E_INVALID ("FormatConverter: Invalid format", :171-173). */
enum {
    DABGPU_FMT_S16 = 1,
    DABGPU_FMT_U8 = 2,
    DABGPU_FMT_S8 = 3
};
/* bytes per I/Q pair, FormatConverter::get_format_size, src/FormatConverter.cpp:192-208 (0 = unknown) */
DABGPU_API size_t dabgpu_format_size(int format);
DABGPU_API int dabgpu_format_process(dabgpu_ctx *ctx, const void *in, size_t in_bytes, int format,
                                     void *out, size_t out_cap, size_t *out_bytes,
                                     size_t *num_clipped);
/* same, device-resident and asynchronous on `stream`; *d_num_clipped (device, 8 bytes, may be
 * NULL) is INCREMENTED by the number of clipped components */
DABGPU_API int dabgpu_format_process_dev(dabgpu_ctx *ctx, const void *d_in, size_t n_floats,
                                         int format, void *d_out, size_t out_cap,
                                         size_t *out_bytes, unsigned long long *d_num_clipped,
                                         void *stream);

/* Host-side helper of the fused chain, no device involved: the inverse filter the Mode I frame kernel uses to
 * correct the FIR outputs at symbol boundaries from the FILTERED symbols alone ("equalised
 * boundary").  For `taps` (the reference's FIRFilter taps, src/FIRFilter.cpp:59-133) it returns in g[0 .. 160) the
 * real filter with  x[n] = sum_j g[j] z[n - (j - 56)]  wherever z[n] = sum_j taps[j] x[n + j] (cyclically) and x
 * has energy on the 1536 occupied carriers of a 2048-point symbol only; *fit = max |G H - 1| over those carriers.
 * Returns DABGPU_OK when such a filter exists to 1e-7 (the chain then uses it), DABGPU_E_INVALID when the taps
 * have no well-conditioned inverse there or ntaps is outside 1 ... 45 (the chain keeps the packed dual transform; a
 * filter of fewer than 45 taps runs as the 45-tap filter with zero taps behind it). */
DABGPU_API int dabgpu_fir_inverse_design(const float *taps, size_t ntaps, float *g, double *fit);

/* How the fused Mode I chain forms the FIRFilter outputs whose look-ahead crosses a symbol boundary (the last
 * ntaps - 1 of every symbol; reference loop src/FIRFilter.cpp:168-191).  AUTO (the default): from the filtered
 * symbols alone through the inverse above whenever the taps have one, otherwise as DIRECT.  DIRECT: always by the
 * direct sum over the unfiltered samples (a second, pruned transform per symbol).  Same results within the FIRFilter
 * bar either way; exists so that both kernels can be selected from a test or a measurement -- it is not read from
 * the environment.  Takes effect at the next *_process call. */
enum { DABGPU_FIR_BOUNDARY_AUTO = 0, DABGPU_FIR_BOUNDARY_DIRECT = 1 };
DABGPU_API int dabgpu_set_fir_boundary_mode(dabgpu_ctx *ctx, int mode);

/* ---- the fused chain ----------------------------------------------------- */

/* FormatConverter as the last step of the chain (the reference wires it after cifPoly when the output is not
 * complexf, src/DabModulator.cpp:270-276, :407): format = 0 (complexf, the default) or DABGPU_FMT_*.  The chain's last
 * kernel stores the integers itself where it has a variant for it -- s16: every Mode I coded-bits chain that is one frame kernel
 * (any filter the fused FIRFilter takes, any gain mode, with or without crest-factor reduction; a windowed guard interval
 * without FIRFilter, or with it up to 10 samples of overlap), and the x2 / x4 resampler with or without the polynomial
 * predistorter; u8 / s8: Mode I coded-bits chain ending in the guard interval or in a filter of up to the default length whose
 * boundary outputs come through the taps' inverse (the default), also with up to 10 samples of OFDM windowing -- half / a
 * quarter of the bytes written and copied to the host; every other combination converts in a kernel of its own.  Output sizes of
 * dabgpu_chain_out_bytes_per_frame / _process / _submit follow the format.  dabgpu_get_num_clipped: the number of
 * clipped components of the most recent chain call (FormatConverter::get_num_clipped_samples, :56-59), after
 * waiting for that call -- or, on the asynchronous path, of the batch dabgpu_chain_collect returned last. */
DABGPU_API int dabgpu_set_output_format(dabgpu_ctx *ctx, int format);
DABGPU_API int dabgpu_get_num_clipped(dabgpu_ctx *ctx, size_t *num_clipped);

/* bytes of IQ produced per transmission frame for a stage mask */
DABGPU_API size_t dabgpu_chain_out_bytes_per_frame(const dabgpu_ctx *ctx, unsigned stage_mask);

/* cifPart output (n_frames x tf_input_bytes) -> IQ.  Replaces the sub-graph
 * cifMap .. cifGuard/cifFilter/cifRes/cifPoly of src/DabModulator.cpp:385-419
 * with ONE plugin.  Frames are consecutive frames of one stream: the stream state
 * (the resampler's halo in the context's device memory, the TII frame parity in the
 * context) carries from frame to frame and from call to call -- and, through
 * dabgpu_get_stream_state / dabgpu_set_stream_state / dabgpu_chain_seed below, from
 * context to context. */
DABGPU_API int dabgpu_chain_process(dabgpu_ctx *ctx, const uint8_t *bits, size_t n_frames,
                                    unsigned stage_mask, void *iq_out, size_t out_cap,
                                    size_t *out_bytes);
/* same, device-resident input and output, asynchronous on `stream` */
DABGPU_API int dabgpu_chain_process_dev(dabgpu_ctx *ctx, const void *d_bits, size_t n_frames,
                                        unsigned stage_mask, void *d_iq, size_t out_cap,
                                        size_t *out_bytes, void *stream);
/* SignalMultiplexer output ((nb_symbols+1) x carriers cf32 per frame) -> IQ:
 * the OfdmGenerator[+GainControl][+Guard][+FIR..] part of the chain. */
DABGPU_API int dabgpu_symbols_process_dev(dabgpu_ctx *ctx, const void *d_carriers,
                                          size_t n_frames, unsigned stage_mask, void *d_iq,
                                          size_t out_cap, size_t *out_bytes, void *stream);

/* Resampler::process -> MemlessPoly::internal_process (cifRes -> cifPoly, src/DabModulator.cpp:403-406) on a native-rate
 * stream that is already in device memory: the tail of the chain by itself.  stage_mask = DABGPU_STAGE_RESAMPLE and / or
 * DABGPU_STAGE_POLY; n_samples complex samples in (a whole number of resampler hops), n_samples * L / M out.  Stateful like
 * the Resampler: it reads and advances the context's halo, the same one the chain calls and dabgpu_resampler_process use and
 * dabgpu_get_stream_state returns; asynchronous on `stream`. */
DABGPU_API int dabgpu_post_process_dev(dabgpu_ctx *ctx, const void *d_native, size_t n_samples, unsigned stage_mask,
                                       void *d_iq, size_t out_cap, size_t *out_bytes, void *stream);

/* ---- stream state: one resampled stream checkpointed, moved, or split over contexts ---------------------------------- *
 * A chain call with DABGPU_STAGE_RESAMPLE (at a ratio other than 1) reads and leaves two pieces of stream state:
 *   - the Resampler's halo: the last rs_nin = 2 x FFT size native-rate INPUT samples, i.e. two hops (the overlap-add sits in
 *     front of the forward transform; reference: the input window it keeps, src/Resampler.cpp:142-147, :188-191);
 *   - the TII frame parity (TII::m_insert, src/TII.cpp:226-242), which every chain call from coded bits advances.
 * The blob below is exactly that, in HOST memory, self-describing (all fields little endian, as the host has them):
 *     offset  0  uint32  magic        DABGPU_STREAM_STATE_MAGIC ("DGSS")
 *             4  uint32  version      DABGPU_STREAM_STATE_VERSION
 *             8  uint32  mode         transmission mode 1..4
 *            12  uint32  tii_insert   1: the next frame of the stream is one that carries TII
 *            16  uint64  rs_in        the rates of dabgpu_set_resampler
 *            24  uint64  rs_out
 *            32  uint32  rs_nin       complex samples that follow: 2 x FFT size, or 0 at equal rates (no Resampler in the chain)
 *            36  uint32  reserved     0
 *            40  rs_nin x (float re, float im): what the next call reads as its halo, oldest sample first
 * (Which of the library's two halo buffers is current never shows.  The symbol index of the CFR statistics' MER measurement,
 * src/OfdmGenerator.cpp:198, is a statistic of the context, not stream state: it is not carried.)
 * dabgpu_stream_state_bytes: the size of the blob for the settings as they stand.
 * dabgpu_get_stream_state: waits for the context, as dabgpu_set_lanes does, then describes the stream after everything queued
 *   on it so far (chain calls, dabgpu_resampler_process, dabgpu_post_process_dev on the context's own stream, the batches of
 *   dabgpu_chain_submit); *bytes (may be NULL) receives the size; DABGPU_E_CAPACITY when cap is smaller.  A fresh context
 *   gives a zero halo and tii_insert = 1; after dabgpu_set_resampler the halo is zero again and the parity is where it was.
 * dabgpu_set_stream_state: waits, then installs the blob.  DABGPU_E_INVALID (with a message) for a NULL argument, a size that
 *   is not the blob's, a wrong magic or version, and a blob taken in another mode, at another ratio or with another rs_nin.
 *   A dabgpu_set_resampler after it resets the state as ever.
 * dabgpu_chain_seed / _dev: leaves the context in the state it would have after frames 0 ... frame_index - 1 of a stream whose
 *   frame frame_index - 1 has the coded bits `leadin_bits` (one frame, tf_input_bytes), under the settings in force: every
 *   transmission frame is at least 96 hops long, so that state is a function of the settings, frame_index and that one frame.
 *   frame_index == 0 is the start of a stream (zero halo, tii_insert = 1; leadin_bits may be NULL).  Otherwise the lead-in
 *   frame runs through the part of stage_mask in front of the Resampler -- as complexf whatever the output format and gain
 *   rounding, with the TII parity of frame frame_index - 1 --, its last rs_nin samples become the halo, and tii_insert =
 *   (frame_index even).  No output; dabgpu_get_cfr_stats, dabgpu_get_num_clipped and dabgpu_debug_last_variant keep describing
 *   the last real chain call.  Ordered like a chain call with DABGPU_STAGE_RESAMPLE: _dev is asynchronous on `stream` and uses
 *   the context's scratch; stream == NULL and the host-pointer form go to lane 0, where the resampler chain calls that follow
 *   go (the host-pointer form has staged the frame when it returns).  At equal rates the call is host-only: it sets the parity.
 *   A seed that fails leaves halo and parity as they were when no kernel of it was queued; after a failure behind that point
 *   (a HIP error) the parity is put back, the halo is undefined and the context is to be seeded or set again.
 *   A context seeded this way produces frames frame_index ... bit for bit as the uninterrupted stream does
 *   (tests/test_stream_state_gpu.py), which is what lets N contexts take the chunks of one stream in turn without waiting
 *   for one another (odr-dabmod_amd/streams.py: PartitionedStream; dabmod_file --contexts). */
#define DABGPU_STREAM_STATE_MAGIC 0x53534744u /* "DGSS" */
#define DABGPU_STREAM_STATE_VERSION 1u
#define DABGPU_STREAM_STATE_HEADER_BYTES 40
DABGPU_API size_t dabgpu_stream_state_bytes(const dabgpu_ctx *ctx);
DABGPU_API int dabgpu_get_stream_state(dabgpu_ctx *ctx, void *buf, size_t cap, size_t *bytes);
DABGPU_API int dabgpu_set_stream_state(dabgpu_ctx *ctx, const void *buf, size_t bytes);
DABGPU_API int dabgpu_chain_seed(dabgpu_ctx *ctx, const uint8_t *leadin_bits, unsigned stage_mask,
                                 uint64_t frame_index);
DABGPU_API int dabgpu_chain_seed_dev(dabgpu_ctx *ctx, const void *d_leadin_bits, unsigned stage_mask,
                                     uint64_t frame_index, void *stream);

/* ---- batches in flight inside one context --------------------------------- *
 * The reference overlaps its stages by handing frame i + 1 to a stage while frame i is still inside it
 * (PipelinedModCodec, src/ModPlugin.cpp:90-154).  The counterpart here: a chain call on the context's OWN stream
 * (dabgpu_chain_process_dev / dabgpu_symbols_process_dev with stream == NULL, and the two batches of dabgpu_chain_submit)
 * goes to one of `lanes` internal HIP streams in turn, each with its own scratch, so that the kernels of consecutive
 * calls overlap where one launch alone cannot fill the chip (frames are independent units).  Consequences for the caller:
 *   - outputs of calls on the context's own stream are complete after dabgpu_synchronize (all lanes), or, in stream
 *     order, for work queued on `stream` after dabgpu_stream_wait_for(ctx, stream);
 *   - inputs produced on a stream of the caller's are ordered in front with dabgpu_wait_for_stream(ctx, stream);
 *   - calls that carry stream state (DABGPU_STAGE_RESAMPLE at a ratio other than 1) and batches of more than 2048 frames
 *     stay on lane 0, in call order (to overlap such calls, split the stream over contexts: "stream state" above);
 *   - a call with an explicit stream argument is what it always was: asynchronous on that stream, the context's scratch.
 *     Do not mix the two on one context without a dabgpu_synchronize in between;
 *   - every receive-side `_dev` entry with stream == NULL (dabgpu_demod_dev, dabgpu_demod_soft_dev, dabgpu_demod_csi_dev,
 *     dabgpu_demod_carrier_state_dev, dabgpu_sync_dev,
 *     dabgpu_sync_extract_dev, dabgpu_channel_dev, dabgpu_tii_scan_dev, dabgpu_cir_dev, dabgpu_decode_dev,
 *     dabgpu_decode_soft_dev, dabgpu_spectrum_dev, dabgpu_dpd_xspectrum_dev, dabgpu_dpd_align_dev, dabgpu_dpd_measure_dev)
 *     runs on the context's own stream, behind everything queued on ANY lane before it: its input may be the output of a
 *     chain call that is still in flight, without a dabgpu_synchronize in between.  Chain calls queued after it start behind
 *     it, whichever lane they go to: one of them may overwrite the buffer the entry reads.  (Two chain calls are not ordered
 *     against each other: a buffer goes to a second chain call only behind such an entry, or a synchronise.)  The result
 *     getters (dabgpu_get_sync_result, dabgpu_get_tii_scan, ...) wait for that stream only, not for the lanes.
 *     tests/test_receive_lanes_gpu.py holds all of this to the bytes of a one-lane context.
 * dabgpu_set_lanes: 1 ... 4 (default 3: measured best at 1 ... 64 frames per call, tools/experiments/exp_r05.py lanes; 1 = every call on the one context stream, in order).  Waits for the context. */
DABGPU_API int dabgpu_set_lanes(dabgpu_ctx *ctx, int lanes);
/* Diagnostic: how many lanes exist so far (lane 0 = the context's stream, the others are created on first use), and in
 * *own_queue_mask, bit i: lane i was found a hardware queue of its own.  (The HIP runtime multiplexes streams onto a few
 * hardware queues, four by default -- GPU_MAX_HW_QUEUES --, and streams that share one run in order; which queue a new
 * stream joins depends on the process's history, so a lane's stream is probed against the lanes before it and replaced
 * until it overlaps with all of them.  A process that keeps more busy streams of its own than the device has hardware
 * queues left cannot be given that.) */
DABGPU_API int dabgpu_debug_lanes(dabgpu_ctx *ctx, int *own_queue_mask);
/* everything the context queues from now on starts after what `stream` holds now */
DABGPU_API int dabgpu_wait_for_stream(dabgpu_ctx *ctx, void *stream);
/* everything queued on `stream` from now on starts after what the context has queued so far, on every lane */
DABGPU_API int dabgpu_stream_wait_for(dabgpu_ctx *ctx, void *stream);

/* The hand-over of the native-rate stream from FIRFilter to Resampler (src/DabModulator.cpp:403-406) inside the fused
 * chain: in pieces of `frames` transmission frames through a two-piece ring (2 x frames x 1.57 MB: sized to stay in
 * the 256 MiB last-level cache), the producer of piece i + 1 on a second internal stream while the x2 / x4 resampler works on
 * piece i.  0 = one piece: the whole batch goes through memory between the two kernels.  `frames` is even (TII frame
 * parity).  Same samples either way (the resampler's state runs through the pieces).  Waits for the context. */
DABGPU_API int dabgpu_set_handover_frames(dabgpu_ctx *ctx, int frames);

/* Asynchronous host path: the streaming shape of dabgpu_chain_process.  submit() stages the coded
 * bits in pinned memory and queues upload, kernels and -- on a second HIP stream -- the copy back
 * into a pinned buffer owned by the context; up to TWO batches may be in flight, so the copy of
 * batch i overlaps the kernels of batch i+1 (a third submit is DABGPU_E_CAPACITY).  collect() waits
 * for the OLDEST batch and hands out its buffer: *iq stays valid until the second next submit.
 * Same settings snapshot, stream state (resampler halo, TII parity) and ordering as the synchronous
 * call; do not mix the two on one context while batches are in flight. */
DABGPU_API int dabgpu_chain_submit(dabgpu_ctx *ctx, const uint8_t *bits, size_t n_frames,
                                   unsigned stage_mask);
DABGPU_API int dabgpu_chain_collect(dabgpu_ctx *ctx, const void **iq, size_t *out_bytes);

/* Which kernels did the most recent chain call (dabgpu_chain_process / _process_dev / _submit, dabgpu_symbols_process_dev,
 * and dabgpu_ofdm_process: the frame kernel from carriers without its epilogue) launch?  A "; "-separated list of kernel
 * names in launch order, the frame kernel with the VALUES of its template arguments
 * ("tf_kernel<logn=11 bits=1 gain=1 guard=1 fir=1 nt=45 cfr=0 gvar=0 zonly=0 ofmt=0 win=0 eq=1>").  The fused chain picks
 * one of ~120 instantiations from the settings (mode, gain mode, filter length, windowing, CFR, TII, output format): this
 * makes the choice observable, so that a test can walk the whole matrix (tests/test_dispatch_matrix.py) and a user can see
 * what a configuration costs.  Diagnostic: not part of the reference's interface. */
DABGPU_API int dabgpu_debug_last_variant(dabgpu_ctx *ctx, char *buf, size_t cap);
/* The trace is OFF by default (a launch then costs one pointer test); dabgpu_debug_trace(ctx, 1) turns it on for the chain
 * calls that follow.  Both calls belong to the thread that issues the chain calls (the trace is not guarded by the settings
 * mutex). */
DABGPU_API int dabgpu_debug_trace(dabgpu_ctx *ctx, int enable);

/* ---- the front-end on the device: ETI(NI) frames -> coded bits -> IQ ------------------------------------------------- *
 * The sub-graph in front of the chain (the CPU classes of odr-dabmod_amd/host/Frontend.h) as two kernels:
 * energy dispersal, the K = 7 mother code and puncturing per (ETI frame, FIC or sub-channel); then the 16-frame time
 * interleaver, CIF assembly over the padding sequence and the BlockPartitioner layout per output word.  Pure integer work:
 * the same bytes as the CPU front-end (tests/test_gpu_frontend_gpu.py).
 *
 * dabgpu_frontend_describe: host only, no context, no device.  Reads FC and the STC words of one raw 6144-byte ETI(NI) frame
 *   and fills the layout below.  DABGPU_E_INVALID, with the message of the CPU class that throws (dabgpu_last_error(NULL),
 *   per thread), for: FICF = 0 (EtiReader::loadEtiData); a protection profile without rules or without a size
 *   (SubchannelSource); a punctured size that is neither 8 x CU nor 8 x CU - 1 (PuncturingEncoder::process); a sub-channel
 *   that ends behind CU 864 (FrameMultiplexer::process); payload that overruns the 6144 bytes (EtiReader).
 * Stream state: the time interleaver reads the last fifteen punctured frames of the stream; they live in the context's device
 *   memory, zero after configure / reset, like the Resampler's halo.  The stream-state blob does NOT carry them (a seed
 *   would need fifteen lead-in ETI frames, not one transmission frame): dabgpu_chain_seed / _dev after a
 *   dabgpu_frontend_configure is refused.  They have a blob and seeds of their own: "front-end stream state" below.
 * All calls below take whole transmission frames (n_eti a multiple of 4 / 1 / 1 / 2 in modes I ... IV; at most max_frames
 *   transmission frames per call), and the frame phase FP of a call's first frame must be a multiple of that count.  Finding
 *   the start of the stream -- the first frame with FP = 0, src/DabMod.cpp:684-693 -- stays with the caller.  The host-pointer
 *   entries compare byte 5 (FICF, NST), the MID bits and the STC words of every frame with the configured layout: a
 *   difference is DABGPU_E_INVALID ("FrameMultiplexer detected ...", as the reference throws on a multiplex reconfiguration),
 *   nothing is queued and the history stays as it was, as after every call that fails before its first launch.  They carry
 *   stream state, so they stay on lane 0 in call order, like resampler chains. */
#define DABGPU_FE_MAX_SUBCH 127 /* NST is a 7-bit field */
#define DABGPU_FE_MAX_RULES 4
typedef struct {
    uint32_t groups;  /* 4-byte groups of mother-code output the rule covers (PuncturingRule::length() / 4) */
    uint32_t pattern; /* 32-bit puncturing vector, MSB first */
} dabgpu_fe_rule;
typedef struct {
    uint32_t sad, stl, tpl; /* start address in capacity units, length in 64-bit words, protection (6 bits) */
    uint32_t framesize;     /* 8 x STL: bytes of payload per ETI frame */
    uint32_t cu;            /* capacity units of 64 bits in the CIF */
    uint32_t padding_byte;  /* 1: the punctured size is 8 x CU - 1 (EN 300 401 table 31), one zero byte follows */
    uint32_t offset;        /* of the payload inside the 6144-byte frame */
    uint32_t n_rules;
    dabgpu_fe_rule rule[DABGPU_FE_MAX_RULES];
} dabgpu_fe_subch;
typedef struct {
    uint32_t mode;       /* 1..4, from MID (0 reads as Mode IV) */
    uint32_t fic_bytes;  /* 96, or 128 in Mode III */
    uint32_t fic_offset; /* 12 + 4 x NST */
    uint32_t fic_n_rules;
    dabgpu_fe_rule fic_rule[DABGPU_FE_MAX_RULES];
    uint32_t tail_bytes, tail_pattern; /* the tail rule of every unit: 3 bytes, 0xcccccc */
    uint32_t nst;
    dabgpu_fe_subch sub[DABGPU_FE_MAX_SUBCH]; /* in STC order */
} dabgpu_fe_layout;
DABGPU_API int dabgpu_frontend_describe(const uint8_t frame[6144], dabgpu_fe_layout *out);
/* describes `frame6144`, checks its mode against the context's, uploads the tables, zeroes the history; waits for the context */
DABGPU_API int dabgpu_frontend_configure(dabgpu_ctx *ctx, const uint8_t *frame6144);
/* zero history, layout kept; waits for the context */
DABGPU_API int dabgpu_frontend_reset(dabgpu_ctx *ctx);
/* n_eti raw ETI(NI) frames (n_eti x 6144 bytes) -> the chain's input, n_eti / (4|1|1|2) x tf_input_bytes: the sub-graph
 * cifFicPrbs ... cifPart of src/DabModulator.cpp:281-385 (PrbsGenerator, ConvEncoder, PuncturingEncoder, TimeInterleaver,
 * FrameMultiplexer, BlockPartitioner) */
DABGPU_API int dabgpu_frontend_process(dabgpu_ctx *ctx, const uint8_t *eti, size_t n_eti, void *bits, size_t out_cap,
                                       size_t *out_bytes);
/* same, device-resident and asynchronous on `stream`.  This entry CANNOT look at the frames: layout, FICF and FP are the
 * caller's to check (a frame of another layout gives bytes of no meaning, within the buffers). */
DABGPU_API int dabgpu_frontend_process_dev(dabgpu_ctx *ctx, const void *d_eti, size_t n_eti, void *d_bits, size_t out_cap,
                                           size_t *out_bytes, void *stream);
/* ETI in, IQ out: dabgpu_frontend_process and dabgpu_chain_process in one call; the coded bits never leave the device */
DABGPU_API int dabgpu_chain_process_eti(dabgpu_ctx *ctx, const uint8_t *eti, size_t n_eti, unsigned stage_mask, void *iq_out,
                                        size_t out_cap, size_t *out_bytes);
/* the streaming shape: dabgpu_chain_submit from ETI frames (lane 0, in call order); dabgpu_chain_collect as it is */
DABGPU_API int dabgpu_chain_submit_eti(dabgpu_ctx *ctx, const uint8_t *eti, size_t n_eti, unsigned stage_mask);

/* ---- front-end stream state: an ETI-fed stream checkpointed, handed over, or split over contexts ------------------------ *
 * A context with a configured front-end carries three pieces of stream state: the Resampler's halo and the TII frame parity
 * ("stream state" above, unchanged: same blob, same version, same size with or without a front-end) and the time
 * interleaver's history, the last DABGPU_FE_HISTORY_FRAMES punctured ETI frames.  A WHOLE ETI-fed stream is moved with BOTH
 * blobs: dabgpu_get_stream_state + dabgpu_frontend_get_state on the one side, dabgpu_frontend_configure (from a frame of the
 * stream), dabgpu_set_stream_state + dabgpu_frontend_set_state on the other.
 * The front-end blob, in HOST memory, self-describing, of one size for every layout (all fields little endian):
 *     offset  0  uint32  magic      DABGPU_FE_STATE_MAGIC ("DGFS")
 *             4  uint32  version    DABGPU_FE_STATE_VERSION
 *             8  uint32  mode       transmission mode 1..4
 *            12  uint32  fc         byte 5 of the ETI frame (FICF, NST) | the MID bits of byte 6 (mask 0x18) << 8
 *            16  uint32  rows       DABGPU_FE_HISTORY_FRAMES
 *            20  uint32  row_bytes  6912 (one CIF)
 *            24  uint32  nst        sub-channels
 *            28  uint32  reserved   0
 *            32  127 x 4 bytes      the STC words of the layout as the ETI frame has them, nst of them, zeros behind
 *           540  rows x row_bytes   the history, oldest frame first: row r is the punctured CIF (before time interleaving) of
 *                                   ETI frame e - 15 + r, zero where that lies before the start of the stream and on every
 *                                   capacity unit no sub-channel owns
 *   (mode, fc, nst and the STC words are the layout identity the host-pointer entries compare every frame with.)  Blobs taken
 *   at the same position of the same stream are equal byte for byte, however the context got there: through calls of any
 *   size, an installed blob or a seed.
 * dabgpu_frontend_state_bytes: the size of the blob (DABGPU_FE_STATE_HEADER_BYTES + 15 x 6912).
 * dabgpu_frontend_get_state: waits for the context, as dabgpu_get_stream_state does, then describes the history after
 *   everything queued so far; *bytes (may be NULL) receives the size; DABGPU_E_CAPACITY when cap is smaller, DABGPU_E_INVALID
 *   when the front-end is not configured.
 * dabgpu_frontend_set_state: waits, then installs the history.  DABGPU_E_INVALID (with a message), the history untouched, when
 *   the front-end is not configured, for a blob from another mode or another multiplex layout, and for a malformed one (size,
 *   magic, version).
 * The seeds compute the state from the ETI frames in front of a position of the stream.  e = the index in the stream of the
 *   first ETI frame the context is to process next (0 = the start of the stream), a multiple of cifs = 4 / 1 / 1 / 2 in modes
 *   I ... IV; the lead-in is the n_leadin frames e - n_leadin ... e - 1, in stream order.
 * dabgpu_frontend_seed / _dev: the history in front of frame e.  n_leadin = min(e, 15), anything else is DABGPU_E_INVALID;
 *   rows from before the start of the stream are zero; e == 0 is dabgpu_frontend_reset under another name.  Cost: one memset
 *   and one launch of the encode kernel over the sub-channels of the lead-in frames -- no FIC, no assembly, no output.
 * dabgpu_chain_seed_eti / _dev: the front-end seed and dabgpu_chain_seed together, for a chain fed from ETI frames.
 *   n_leadin = min(e, 15 + cifs).  The first n_leadin - cifs frames give the history in front of transmission frame
 *   e / cifs - 1; the last cifs frames ARE that transmission frame: they go through the front-end into scratch, and their
 *   coded bits seed the chain as dabgpu_chain_seed does with frame_index = e / cifs (halo, TII parity).  Afterwards the history
 *   is the one in front of frame e.  No output; dabgpu_get_cfr_stats, dabgpu_get_num_clipped and dabgpu_debug_last_variant
 *   keep describing the last real chain call.  (dabgpu_chain_seed / _dev keep refusing a context with a front-end.)
 * The host-pointer forms compare every lead-in frame with the configured layout, as the other host-pointer entries do, and
 *   want the frame phase of the LAST lead-in frame at cifs - 1 modulo cifs (the lead-in ends where a transmission frame ends;
 *   its first frame need not start one); they return when the frames have been read.  The _dev forms cannot look at the
 *   frames; they are asynchronous on `stream` -- NULL: lane 0, the context's own stream -- in order with the calls that
 *   follow there.  Every refusal (not configured, e, n_leadin, a frame of another layout, a ratio the Resampler does not run)
 *   comes before anything is queued: history, halo and parity stay as they were.
 * A context seeded this way produces frames e ... byte for byte as the uninterrupted stream does
 *   (tests/test_frontend_state_gpu.py; odr-dabmod_amd/streams.py: PartitionedStream.modulate_eti). */
#define DABGPU_FE_HISTORY_FRAMES 15
#define DABGPU_FE_STATE_MAGIC 0x53464744u /* "DGFS" */
#define DABGPU_FE_STATE_VERSION 1u
#define DABGPU_FE_STATE_HEADER_BYTES 540
DABGPU_API size_t dabgpu_frontend_state_bytes(const dabgpu_ctx *ctx);
DABGPU_API int dabgpu_frontend_get_state(dabgpu_ctx *ctx, void *buf, size_t cap, size_t *bytes);
DABGPU_API int dabgpu_frontend_set_state(dabgpu_ctx *ctx, const void *buf, size_t bytes);
DABGPU_API int dabgpu_frontend_seed(dabgpu_ctx *ctx, const uint8_t *eti_leadin, size_t n_leadin, uint64_t e);
DABGPU_API int dabgpu_frontend_seed_dev(dabgpu_ctx *ctx, const void *d_eti_leadin, size_t n_leadin, uint64_t e,
                                        void *stream);
DABGPU_API int dabgpu_chain_seed_eti(dabgpu_ctx *ctx, const uint8_t *eti_leadin, size_t n_leadin, unsigned stage_mask,
                                     uint64_t e);
DABGPU_API int dabgpu_chain_seed_eti_dev(dabgpu_ctx *ctx, const void *d_eti_leadin, size_t n_leadin,
                                         unsigned stage_mask, uint64_t e, void *stream);

/* ---- the receiver: native-rate IQ -> coded bits, per-frame MER and bit errors --------------------------------------------- *
 * The modulator's output decoded back on the device: per OFDM symbol the forward transform over the window that ends `early`
 * samples before the end of the symbol, differential demodulation against the symbol before, hard QPSK decisions, the
 * frequency interleaver undone -- ETSI EN 300 401 14.5 - 14.7 backwards.  The reference has no receiver; these entries replace
 * nothing of its flowgraph.  No synchronisation (since built: dabgpu_sync* below) and no channel estimate: the input is whole transmission frames as a chain
 * call without the Resampler writes them (tf_samples each), complexf (format 0) or DABGPU_FMT_S16; u8 / s8 are not taken.
 * `early` (0 ... sym_size - spacing, the data symbols' cyclic prefix; anything else is DABGPU_E_INVALID) moves the window away
 * from what FIRFilter's look-ahead and the guard window's overlap leave at the end of a symbol: ntaps - 1 for a filtered
 * chain, plus the overlap for a windowed one.  Any window inside the cyclic extension only rotates all symbols alike.
 * Output: n_frames x tf_input_bytes, the layout dabgpu_chain_process takes.  Per frame, over all data symbols and carriers,
 * with d = z_s conj(z_{s-1}) per carrier and c = ((1 - 2 I) + j (1 - 2 Q)) / sqrt(2) its decided point:
 *   sum_signal      sum |d|^2
 *   sum_quadrature  sum Im(d conj(c))^2 -- the part of d at right angles to its decision; independent of the per-symbol gain,
 *                   of |H[k]|^2 and of `early`.  MER in dB = 10 log10(sum_signal / sum_quadrature), formed by the caller
 *   bit_errors      bits that differ from the reference bits, n_bits the number compared (0 without reference bits)
 *   min_margin      min of min(|Re d|, |Im d|) / |d|: how close the worst decision came (at most sqrt(1/2))
 * The sums are float64 sums of fp32 terms, added in no fixed order: they repeat to about 1e-7, not bit for bit.
 * dabgpu_demod_dev: device pointers (four-byte aligned), asynchronous on `stream` (NULL: the context's own stream, behind every
 *   lane); d_bits_out and d_ref_bits may be NULL.  dabgpu_demod: the host-pointer form.  dabgpu_get_demod_stats: frame `frame`
 *   of the most recent of these calls or monitored chain call, after waiting for it, as dabgpu_get_cfr_stats does. */
typedef struct dabgpu_demod_stats {
    double sum_signal, sum_quadrature;
    uint64_t bit_errors, n_bits;
    double min_margin;
} dabgpu_demod_stats;
DABGPU_API int dabgpu_demod_dev(dabgpu_ctx *ctx, const void *d_iq, int format, size_t n_frames, int early,
                                void *d_bits_out, const void *d_ref_bits, void *stream);
DABGPU_API int dabgpu_demod(dabgpu_ctx *ctx, const void *iq, int format, size_t n_frames, int early, uint8_t *bits_out,
                            const uint8_t *ref_bits);
DABGPU_API int dabgpu_get_demod_stats(dabgpu_ctx *ctx, size_t frame, dabgpu_demod_stats *out);
/* Soft output: the same call with one int8 metric per coded bit besides (d_soft_out / soft_out, not NULL, four-byte aligned on
 * the device); bits, reference count and per-frame figures exactly as above (same kernel, same sums, dabgpu_get_demod_stats).
 * Layout: n_frames x 8 tf_input_bytes.  Soft 8 p + b of a frame belongs to bit 0x80 >> b of byte p of the coded-bit layout:
 *   per block the I softs in interleaver-undone order, then the Q softs.  soft > 0: the bit is more likely 1; soft < 0: more
 *   likely 0; 0 says nothing.
 * Scale, per data symbol s over its K carriers: P = sum_k |d_k|^2, q = 64 sqrt(2) / sqrt(P / K),
 *   soft_I = clamp(rint(-Re d_k q), -127, 127), soft_Q likewise from Im d_k; all zero when P = 0.  A clean, flat symbol gives
 *   +-64.  Per symbol on purpose: independent of the per-symbol gain (as the MER figure is), the carriers' relative reliability
 *   is kept, and no second pass over the frame is needed.  P is added in a fixed order: the softs repeat bit for bit and do not
 *   depend on the run geometry (dabgpu_debug_demod_run_symbols).  Same `early` rule and the same refusals as dabgpu_demod*. */
DABGPU_API int dabgpu_demod_soft_dev(dabgpu_ctx *ctx, const void *d_iq, int format, size_t n_frames, int early,
                                     void *d_soft_out, void *d_bits_out, const void *d_ref_bits, void *stream);
DABGPU_API int dabgpu_demod_soft(dabgpu_ctx *ctx, const void *iq, int format, size_t n_frames, int early, int8_t *soft_out,
                                 uint8_t *bits_out, const uint8_t *ref_bits);
/* ---- the carrier state: soft metrics weighted by the noise on their carrier, MER per carrier ------------------------------ *
 * d = z_s conj(z_{s-1}) carries |H[k]|^2 already; what the metrics above lack for a log-likelihood ratio is 1 / sigma_k^2, the
 * noise-plus-interference power on carrier k -- nothing on white noise, everything behind a spur or a co-channel carrier, whose
 * carriers have the largest |d| of the symbol and random signs.  The state is measured on the frame itself, per carrier
 * POSITION k (0 ... K - 1 in frequency order: bins 1 ... K/2 -> k = bin - 1, bins N - K/2 ... N - 1 -> k = bin - N + K; the
 * index in front of the frequency interleaver), over the S = nb_symbols - 1 data symbols s of the frame, with q_s the soft
 * scale above and u = d_k q_s:
 *   A_k = sum_s rint(2^F (|Re u| + |Im u|) / 2)      the folded amplitude
 *   V_k = sum_s rint(2^F (|Im u| - |Re u|)^2 / 2)    the power at right angles to the decision (sum_quadrature's term)
 * with F = DABGPU_CSI_FRAC_BITS, rint to the nearest integer (ties to even); int64 sums.  Integer sums do not depend on the
 * order of their terms: the state, the weights and the softs are the same bytes for every run geometry
 * (dabgpu_debug_demod_run_symbols), batch size and repetition.  The state is formed in float64 from the samples on -- the
 * transform, d, P, q_s = 64 sqrt(2) / sqrt(P / K) and the terms -- so that a float64 evaluation of these lines gives the same
 * integers: one count is 2^-16 of a metric step, finer than fp32 resolves at a metric's magnitude.  (Against another float64
 * transform a term lies some 1e-8 counts off.)  The weighted metrics below use dabgpu_demod_soft's fp32 d and q_s.
 * The weights, float64, operation by operation (every one IEEE-754 correctly rounded, so a model reproduces the bits):
 *   T_0 = all K carriers; for i = 0 ... DABGPU_CSI_TRIM_PASSES - 1, with n_i = |T_i| and SV_i = sum of V_k over T_i (integers):
 *                       T_(i+1) = { k of all K carriers : V_k n_i <= DABGPU_CSI_TRIM_FACTOR SV_i }      (integer comparison)
 *   T the last set, n = |T| (never empty: the smallest V_k is always in), SA = sum of A_k over T, SV = sum of V_k over T
 *   SA = 0 or SV = 0:   w_k = 1 for every k          (all-zero input; a clean loop whose quadrature terms all round to 0)
 *   otherwise           floor = double(SV) / double(64 n)
 *                       r_k = (double(A_k) * double(SV)) / (double(SA) * max(double(V_k), floor))
 *                       w_k = float(min(DABGPU_CSI_MAX_WEIGHT, r_k))
 *   i.e. w_k = (A_k / mean A) / (max(V_k, mean V / 64) / mean V), the means over T: the Gaussian LLR 2 A x / V with the |H|^2
 *   that x carries taken out, 1 on a flat channel with white noise, at most DABGPU_CSI_MAX_WEIGHT, 0 on a carrier without
 *   signal; always finite.  The means leave out the carriers whose V_k lies far above the rest, because those carriers are what
 *   the weights exist for: with plain means a strong spur raises mean V until every clean carrier sits at the maximum weight
 *   and its metrics at +-127 (on the models that rule gained 4 dB against a tone, this one 14 dB: profiles/csi.txt).  On white
 *   noise V_k scatters by sqrt(2 / S) about its mean and no carrier comes near the factor: nothing is left out.
 * The weighted metric: soft_I = clamp(rint((-Re d_k q_s) w_k), -127, 127), soft_Q likewise, fp32 in this order -- with every
 *   w_k = 1 the bytes dabgpu_demod_soft writes.  The weights of a frame come from that frame alone: no state across frames.
 * Per-carrier MER in dB, formed by the caller: 20 log10(A_k / sqrt(2^(F - 1) S V_k))  (= 10 log10 of 2 (A_k / S)^2 over V_k / S
 *   in units of u^2; +inf where V_k = 0).
 * dabgpu_demod_csi_dev / dabgpu_demod_csi: the arguments, formats, `early` rule, refusals (all before anything is queued), output
 *   layout, bits and per-frame figures (dabgpu_get_demod_stats) of dabgpu_demod_soft_dev / dabgpu_demod_soft; the softs are the
 *   weighted ones.  Three launches: the state (a float64 transform pass), the weights, the weighted softs (the fp32 pass of
 *   dabgpu_demod_soft with the weights).
 * dabgpu_demod_carrier_state_dev / dabgpu_demod_carrier_state: the state and the weights alone -- no softs, no bits, and the
 *   figures of dabgpu_get_demod_stats stay those of the call before.
 * dabgpu_get_carrier_state: frame `frame` of the most recent of these four calls, after waiting for it: K int64 each to A and V,
 *   K floats to w (any of them NULL: not wanted).  DABGPU_E_INVALID before any such call and for a frame beyond it.
 * stream == NULL: the context's own stream behind every lane, as every receive-side _dev entry. */
#define DABGPU_CSI_FRAC_BITS 16
#define DABGPU_CSI_MAX_WEIGHT 4
#define DABGPU_CSI_TRIM_PASSES 3
#define DABGPU_CSI_TRIM_FACTOR 4
DABGPU_API int dabgpu_demod_csi_dev(dabgpu_ctx *ctx, const void *d_iq, int format, size_t n_frames, int early,
                                    void *d_soft_out, void *d_bits_out, const void *d_ref_bits, void *stream);
DABGPU_API int dabgpu_demod_csi(dabgpu_ctx *ctx, const void *iq, int format, size_t n_frames, int early, int8_t *soft_out,
                                uint8_t *bits_out, const uint8_t *ref_bits);
DABGPU_API int dabgpu_demod_carrier_state_dev(dabgpu_ctx *ctx, const void *d_iq, int format, size_t n_frames, int early,
                                              void *stream);
DABGPU_API int dabgpu_demod_carrier_state(dabgpu_ctx *ctx, const void *iq, int format, size_t n_frames, int early);
DABGPU_API int dabgpu_get_carrier_state(dabgpu_ctx *ctx, size_t frame, int64_t *A, int64_t *V, float *w);
/* Diagnostic: every weight 1 whatever the state says (the sums are still formed): dabgpu_demod_csi* then writes
 * dabgpu_demod_soft*'s bytes. */
DABGPU_API int dabgpu_debug_csi_unit_weights(dabgpu_ctx *ctx, int enable);
/* host only, no context, no device: the range test of `early` for a transmission mode (1..4; 0 = IV), with the message the
 * entries above give (dabgpu_last_error(NULL), per thread) */
DABGPU_API int dabgpu_demod_check_early(int mode, int early);
/* The monitor: off by default, and while it is off nothing changes.  While it is on, every dabgpu_chain_process /
 * _process_dev / _process_eti call runs the receiver behind its last kernel, on the same stream, on the call's own output
 * against the call's own coded bits (the ETI form: the front-end's), without a bit output; dabgpu_get_demod_stats then
 * describes the most recent such call.  early < 0: (ntaps - 1 if FIRFilter is in the call's mask) + the window overlap.
 * The IQ is what the call writes with the monitor off.  Monitored calls stay on lane 0, like resampler chains.  Refused with
 * DABGPU_E_INVALID before anything is queued: a mask with the Resampler (at a ratio other than 1) or without the guard
 * interval, u8 / s8 output, dabgpu_chain_submit* -- and an `early` beyond the cyclic prefix.  Takes effect at the next call. */
DABGPU_API int dabgpu_set_monitor(dabgpu_ctx *ctx, int enable, int early);
/* Diagnostic: data symbols per workgroup of the receiver's kernel (a workgroup transforms one symbol more than it decides);
 * 0 (the default) = chosen from the batch size.  Same bits for every value; exists so that a test can walk the run geometry. */
DABGPU_API int dabgpu_debug_demod_run_symbols(dabgpu_ctx *ctx, int symbols);

/* ---- the synchroniser: frame starts and carrier offset of a capture, frames for the receiver ------------------------------- *
 * The stage in front of dabgpu_demod*: a native-rate capture that starts at an arbitrary sample and sits a few carrier spacings
 * off (a feedback or monitoring receiver's, as dabgpu_dpd_* takes them) -> where its transmission frames start, the carrier
 * frequency offset of each, and the frames rotated back and cut out, so that capture -> sync -> demod(_soft) -> decode(_soft)
 * runs on the device.  The reference has no receiver; these entries replace nothing of its flowgraph.
 * Input: n_samples at the native rate, complexf (format 0) or DABGPU_FMT_S16.  With N = spacing, K = carriers, L = nb_symbols,
 * null = null_size, sym = sym_size, CP = sym - N, tf = tf_samples, B = N / 32, NB = floor(null / B), P[k] the phase reference
 * symbol on carrier k:
 *   1. block power     p[b] = sum_{j < B} |x[b B + j]|^2 over the whole blocks of the first tf + null samples
 *   2. coarse start    S[b] = p[b] + ... + p[b + NB - 1]; b* = the first b in 0 ... tf / B - 1 with the lowest S;
 *                      coarse_0 = b* B.  Frame k is a candidate when coarse_k = coarse_0 + k tf has coarse_k + tf <= n_samples,
 *                      at most max_frames (the context's) of them.  null_depth = (S[b*] / NB) / mean(p): 0 for exact-zero nulls
 *   3. fractional offset, per candidate: gamma = sum_s sum_{i = 2 B}^{CP - 2 B - 1} x[a_s + i] conj(x[a_s + i + N]),
 *                      a_s = coarse_k + null + s sym, s < L;  eps = -arg(gamma) / 2 pi in [-1/2, 1/2)
 *   4. integer offset  R = FFT_N(x[w0 + i] e^{-j 2 pi eps i / N}), w0 = coarse_k + null + CP;  for m = -max_shift ... max_shift
 *                      D(m) = sum_k R[k + 1 + m] conj(R[k + m]) conj(P[k + 1] conj(P[k])) over the pairs k, k + 1 both occupied;
 *                      shift = the first m with the largest |D|^2 (a timing error only rotates D)
 *   5. fine start      C[k] = R[k + shift] conj(P[k]) on the occupied carriers, c = N IFFT_N(C), l* = the first index of the
 *                      largest |c|^2, taken as l* - N from N / 2 on;  start = coarse_k + l*;
 *                      quality = |c[l*]|^2 / (K sum |C|^2): at most 1, 1 for a clean flat single path
 *   6. per frame       start, shift, eps, cfo_hz = (shift + eps) 2 048 000 / N, quality, null_depth,
 *                      valid = (start >= 0 and start + tf <= n_samples)
 *   7. extraction      out[k][i] = x[start_k + i] e^{j phi_i}, i < tf, complexf;  phi_i = 2 pi ((i step mod 2^64) >> 32) / 2^32,
 *                      step = rint(-(shift + eps) / N 2^64): an integer phase, nothing accumulates over a frame.  Frames that
 *                      are not valid are zeros.
 * The coarse start lands at or after the true start, by less than B: a capture needs a tail behind its last frame for that
 * frame to be a candidate.  Near eps = +-1/2 consecutive frames may report (12, +0.4998) and (13, -0.4999): ONLY shift + eps
 * IS MEANINGFUL.  Every sum and search runs in a fixed order: a call on the same samples gives the same bytes, ties go to the
 * first index.  The extracted frames start on the strongest path; demodulate them with `early` inside the cyclic prefix
 * (CP / 2 leaves room on either side).
 * dabgpu_sync_dev: device pointer (aligned to a sample), asynchronous on `stream` (NULL: the context's own stream, behind every
 *   lane); no host round trip between its kernels.  dabgpu_sync: the host-pointer form.  dabgpu_get_sync_result: waits for the
 *   most recent of them, as dabgpu_get_demod_stats does; *n_frames = the candidates, min(*n_frames, cap) records to `out`.
 * dabgpu_sync_extract_dev / dabgpu_sync_extract: step 7 with the records of the most recent dabgpu_sync* call on the context,
 *   straight from device memory (same stream, or ordered behind it by the caller).  The output holds
 *   min(max_frames, n_samples / tf) frames of tf complexf samples, eight-byte aligned; those beyond the candidates are zeros too.
 * Refused with DABGPU_E_INVALID and a message before anything is queued: a format other than 0 / DABGPU_FMT_S16, a null or
 *   misaligned pointer, n_samples < 2 tf + null (no whole frame is guaranteed in less), max_shift outside 0 ... 31 (31 =
 *   (N - K) / 2 - 1 in Mode III), an extraction without a dabgpu_sync* call on the same n_samples before it.
 * dabgpu_sync_check: host only, no context, no device: the shape refusals for a mode (1..4; 0 = IV), message via
 *   dabgpu_last_error(NULL).
 * Out of scope: sampling-clock offset (since built: the clock), fractional-sample timing, multipath beyond the strongest path, tracking across calls,
 *   resampled (non-native-rate) captures, u8 / s8. */
typedef struct dabgpu_sync_frame {
    int64_t start;
    int shift, valid;
    double eps, cfo_hz, quality, null_depth;
} dabgpu_sync_frame;
DABGPU_API int dabgpu_sync_dev(dabgpu_ctx *ctx, const void *d_iq, int format, size_t n_samples, int max_shift, void *stream);
DABGPU_API int dabgpu_sync(dabgpu_ctx *ctx, const void *iq, int format, size_t n_samples, int max_shift);
DABGPU_API int dabgpu_get_sync_result(dabgpu_ctx *ctx, size_t *n_frames, dabgpu_sync_frame *out, size_t cap);
DABGPU_API int dabgpu_sync_extract_dev(dabgpu_ctx *ctx, const void *d_iq, int format, size_t n_samples, void *d_frames_out,
                                       void *stream);
DABGPU_API int dabgpu_sync_extract(dabgpu_ctx *ctx, const void *iq, int format, size_t n_samples, void *frames_out);
DABGPU_API int dabgpu_sync_check(int mode, size_t n_samples, int max_shift);

/* ---- the channel decoder: coded bits -> the ETI payload, per-unit corrected bits and payload bit errors -------------------- *
 * What a DAB receiver runs behind the demodulator, on the device: the time de-interleaver, depuncturing, the K = 7 Viterbi
 * decoder (hard decisions) and the energy dispersal -- the two kernels of the front-end backwards, from the very tables
 * dabgpu_frontend_configure uploads.  The reference has no receiver; these entries replace nothing of its flowgraph.  No
 * synchronisation (since built: dabgpu_sync* above), no ETI header or FIG reconstruction; soft decisions: dabgpu_decode_soft* below.
 * Input: n_tf transmission frames of coded bits in the chain's input layout (what dabgpu_frontend_process writes and
 *   dabgpu_demod returns), at most max_frames per call, four-byte aligned on the device.
 * Output: n = n_tf x (4 | 1 | 1 | 2) images of 6144 bytes.  An image holds the decoded FIC and sub-channel payload at their
 *   places in the ETI frame (fic_offset, the sub-channels' offsets) and zeros everywhere else: headers, EOF and TIST are not
 *   reconstructed.
 * Stream state: the time interleaver spreads a frame over sixteen, so the context keeps the last fifteen received rows (the
 *   punctured FIC of an ETI frame followed by its CIF) on the device, zero after dabgpu_frontend_configure (the layout is new)
 *   and after dabgpu_decode_reset; dabgpu_frontend_reset does not touch them.  The decoder is a delay line of fifteen ETI
 *   frames: a call that brings rows e ... e + n - 1 of a stream returns ETI frames e - 15 ... e + n - 16.  Outputs with a
 *   negative index are the lead-in: zero bytes, valid = 0, all counts 0.  THE LAST FIFTEEN FRAMES OF A FINITE STREAM ARE NEVER
 *   RETURNED: the transmitter has not sent all of their bits yet.  The calls carry stream state, so they stay on lane 0 in
 *   call order, like the front-end's.  There is no state blob and no seed for this history (out of scope here): a stream
 *   is decoded from its start, or the first fifteen outputs after a reset are discarded by the caller.
 * d_ref_eti / ref_eti (may be NULL): n x 6144 bytes, row i the ETI frame output i should equal; the differing payload bits
 *   are counted per unit (headers and padding are not compared).
 * Per (output, unit) figures, all integers, the same for every call geometry: corrected = the final path metric = received
 *   coded bits that disagree with the decoded codeword; coded_bits = transmitted bits of the unit; bit_errors / n_bits against
 *   the reference payload (0 / 0 without one).  dabgpu_get_decode_stats: output `frame` of the most recent call, after waiting
 *   for it; unit -1 = the whole frame (sums), 0 = the FIC, 1 + i = sub-channel i in STC order.
 * Refused before anything is queued, the history untouched: front-end not configured; a layout in which two sub-channels cover
 *   one capacity unit (DABGPU_E_INVALID: the front-end lets the last one win, the other's bits were never transmitted);
 *   n_tf = 0; n_tf above max_frames and out_cap below n x 6144 (DABGPU_E_CAPACITY; *out_bytes receives the size).
 * dabgpu_decode_check_layout: host only, no context, no device: DABGPU_E_INVALID and the message (dabgpu_last_error(NULL), per
 *   thread) for a layout the decoder refuses. */
typedef struct dabgpu_decode_stats {
    uint32_t valid; /* 0: lead-in output (stream index < 0) */
    uint64_t corrected, coded_bits;
    uint64_t bit_errors, n_bits;
} dabgpu_decode_stats;
DABGPU_API int dabgpu_decode_check_layout(const dabgpu_fe_layout *layout);
/* zero history, layout kept; waits for the context */
DABGPU_API int dabgpu_decode_reset(dabgpu_ctx *ctx);
DABGPU_API int dabgpu_decode_dev(dabgpu_ctx *ctx, const void *d_bits, size_t n_tf, void *d_eti_out, size_t out_cap,
                                 const void *d_ref_eti, size_t *out_bytes, void *stream);
DABGPU_API int dabgpu_decode(dabgpu_ctx *ctx, const uint8_t *bits, size_t n_tf, uint8_t *eti_out, size_t out_cap,
                             const uint8_t *ref_eti, size_t *out_bytes);
DABGPU_API int dabgpu_get_decode_stats(dabgpu_ctx *ctx, size_t frame, int unit, dabgpu_decode_stats *out);
/* The soft decoder: the same calls on soft metrics.  Input: n_tf x 8 tf_input_bytes int8 in the layout dabgpu_demod_soft writes
 * (soft 8 p + b belongs to bit 0x80 >> b of byte p; > 0: more likely 1).  Any int8 is accepted; -128 counts with magnitude 128.
 * Stream state of its own: fifteen soft rows of 8 (fic_out + 6912) bytes, allocated at the first soft call, zero after
 *   dabgpu_frontend_configure and dabgpu_decode_reset, independent of the hard decoder's history -- hard and soft calls may be
 *   mixed on one context, and each stream sees only its own rows.  The same delay line of fifteen ETI frames, the same lead-in
 *   outputs, the same refusals before anything is queued, the same lane.
 * Metric, in integers.  With e_i the expected bit and r_i the soft of a branch's four code bits (0 where the bit was not
 *   transmitted): cost = sum_i max(0, (1 - 2 e_i) r_i), the magnitude of every soft whose sign contradicts the branch; the
 *   complementary branch costs sum |r_i| - cost.  State 0 starts at 0, every other state at 1 << 30.  uint32 without
 *   normalisation: at most 4 x 128 = 512 per step over fewer than 48 294 steps stays below 2^32 (even doubled).  Tie rule and
 *   traceback are the hard decoder's: the predecessor whose oldest bit is 0 survives unless the other is strictly smaller;
 *   traceback starts from state 0 behind the tail.  On softs that are +-1 the decisions are the hard decoder's, ties included.
 * Per (output, unit) figures, all integers, the same for every call geometry:
 *   metric      final metric of state 0 = sum |soft| over the received bits that contradict the decoded codeword
 *   contra_sum  that sum formed a second way, from the decoded bits encoded again: always equal to metric
 *   soft_sum    sum |soft| over the unit's transmitted bits
 *   corrected   transmitted bits with a non-zero soft whose sign contradicts the re-encoded codeword
 *   erasures    transmitted bits with soft 0
 *   coded_bits, bit_errors, n_bits as dabgpu_decode_stats */
typedef struct dabgpu_decode_soft_stats {
    uint32_t valid; /* 0: lead-in output (stream index < 0) */
    uint64_t metric, contra_sum, soft_sum;
    uint64_t corrected, erasures, coded_bits;
    uint64_t bit_errors, n_bits;
} dabgpu_decode_soft_stats;
DABGPU_API int dabgpu_decode_soft_dev(dabgpu_ctx *ctx, const void *d_soft, size_t n_tf, void *d_eti_out, size_t out_cap,
                                      const void *d_ref_eti, size_t *out_bytes, void *stream);
DABGPU_API int dabgpu_decode_soft(dabgpu_ctx *ctx, const int8_t *soft, size_t n_tf, uint8_t *eti_out, size_t out_cap,
                                  const uint8_t *ref_eti, size_t *out_bytes);
DABGPU_API int dabgpu_get_decode_soft_stats(dabgpu_ctx *ctx, size_t frame, int unit, dabgpu_decode_soft_stats *out);

/* ---- the spectrum monitor: Welch power spectrum of any sample buffer, mask check ----------------------------------------- *
 * The other half of what a transmitter operator watches: the out-of-band shoulders FIRFilter exists for, which CFR, the
 * predistorter, the guard window and the integer formats all trade against MER.  The reference has no such stage; these
 * entries replace nothing of its flowgraph.  The estimate is an averaged periodogram: segments of 2048 samples (in every
 * transmission mode) at a hop of 1024, segment i = samples 1024 i ... 1024 i + 2047 for i = 0 ... floor((n_samples - 2048) /
 * 1024); fewer than 2048 samples give no segment, the tail that fills no segment is not used, segments never span two calls.
 * Each segment is multiplied by a window table (fp32), transformed on the device (fp32) and |X_w[k]|^2 is added in float64.
 * It needs no symbol timing, no native rate and no particular format: `format` is 0 (complexf), DABGPU_FMT_S16 (int16 pairs,
 * value as it is), DABGPU_FMT_U8 (byte - 128: what FormatConverter adds, undone) or DABGPU_FMT_S8 (value as it is).  The
 * null symbol and whatever else lies in the buffer are part of the estimate.  There are no floating-point atomics: the sums
 * are a function of input, window and run geometry alone, and repeat bit for bit.
 * dabgpu_spectrum_window: host only, no context.  window 0 rectangular, 1 Hann 0.5 - 0.5 cos(2 pi k / N), 2 four-term
 *   Blackman-Harris (0.35875, 0.48829, 0.14128, 0.01168); periodic form, evaluated in float64 and rounded to fp32 -- the very
 *   table the kernel multiplies by.  DABGPU_E_INVALID for another window or a null pointer (dabgpu_last_error(NULL)).
 * dabgpu_spectrum_dev: device pointer aligned to the sample size (8 / 4 / 2 / 2 bytes), asynchronous on `stream` (NULL: the
 *   context's own stream, behind every lane).  accumulate 0: the sums start over with this call; otherwise it adds to them,
 *   and must use the window they were formed with.  n_samples < 2048 is accepted and adds nothing.  Calls on different streams
 *   share one accumulator and one scratch: the caller orders them.  dabgpu_spectrum: the host-pointer form.
 * dabgpu_get_spectrum: waits for the most recent spectrum work, then raw[k] = sum over segments of |X_w[k]|^2, bins in FFT
 *   order (k = 0 is DC, k >= 1024 the negative frequencies), and info (either may be NULL).  A power density estimate is
 *   raw / (segments * sum_w2).  rate_hz: 2 048 000 L / M of the context's resampler for monitored chain calls (2 048 000
 *   without the Resampler in the mask), 0 for the stand-alone entries, which do not know the rate.
 * dabgpu_reset_spectrum: sums and segment count to zero.
 * Refused with DABGPU_E_INVALID and a message before anything is queued: unknown format or window, a pointer not aligned to
 * the sample size, a null pointer with samples, accumulating with another window than the sums hold. */
typedef struct dabgpu_spectrum_info {
    uint64_t segments;
    int nfft, window;
    double sum_w2;      /* sum of w^2 over the fp32 table, in float64 */
    double rate_hz;
} dabgpu_spectrum_info;
DABGPU_API int dabgpu_spectrum_window(int window, float *out2048);
DABGPU_API int dabgpu_spectrum_dev(dabgpu_ctx *ctx, const void *d_iq, int format, size_t n_samples, int window,
                                   int accumulate, void *stream);
DABGPU_API int dabgpu_spectrum(dabgpu_ctx *ctx, const void *iq, int format, size_t n_samples, int window, int accumulate);
DABGPU_API int dabgpu_get_spectrum(dabgpu_ctx *ctx, double *raw2048, dabgpu_spectrum_info *info);
DABGPU_API int dabgpu_reset_spectrum(dabgpu_ctx *ctx);
/* dabgpu_set_spectrum_monitor -- the spectrum monitor: off by default, and while it is off launches, bytes and trace are what they were.  While it is on,
 * every dabgpu_chain_process / _process_dev / _process_eti call queues the two kernels behind its last kernel (behind the
 * receiver's when dabgpu_set_monitor is on too), on the same stream, over whatever samples the call wrote, in the call's
 * output format -- chains with the Resampler, MemlessPoly, u8 / s8 output and without the guard interval included -- and the
 * sums accumulate from call to call until dabgpu_reset_spectrum (or until the window or the output rate changes, which starts
 * them over; a stand-alone dabgpu_spectrum / _dev call in between takes the sums for itself, so the next monitored call starts
 * them over as well).  The IQ is what the call writes with the monitor off.  Monitored calls stay on lane 0: two reduce kernels must
 * not race on the sums.  dabgpu_chain_submit* is refused before anything is queued.  Takes effect at the next call. */
DABGPU_API int dabgpu_set_spectrum_monitor(dabgpu_ctx *ctx, int enable, int window);
/* dabgpu_debug_spectrum_run_segments -- diagnostic: segments per workgroup of spectrum_kernel; 0 (the default) = chosen from the input size (about 1024 workgroups,
 * four segments or more each).  At most 65536 workgroups whatever is asked.  The sums agree to float64 reordering for every
 * value; exists so that a test can walk the run geometry. */
DABGPU_API int dabgpu_debug_spectrum_run_segments(dabgpu_ctx *ctx, int segments);
/* dabgpu_debug_resampler_run_hops -- diagnostic: hops per workgroup of every resampler kernel; 0 (the default) = by the call size. */
DABGPU_API int dabgpu_debug_resampler_run_hops(dabgpu_ctx *ctx, int hops);
/* dabgpu_debug_resampler_last_launch -- diagnostic: hops per workgroup and workgroups of the context's most recent resampler launch (0, 0: none yet). */
DABGPU_API int dabgpu_debug_resampler_last_launch(dabgpu_ctx *ctx, int *hops, unsigned *grid);
/* dabgpu_spectrum_check_mask -- host only, no context, no device: a spectrum against a mask.  Bin k of nfft lies at f_k = (k < nfft/2 ? k : k - nfft) rate_hz
 * / nfft.  ref = mean of raw over the bins with 0 < |f_k| <= 768 kHz (the occupied band in all four modes); level_k =
 * 10 log10(raw[k] / ref).  The mask is n_points (offs_hz, limit_db) pairs with offs_hz strictly increasing: the limit at |f_k| is
 * piecewise linear in dB between the points, the last value holds beyond the last offset, bins below the first offset are not
 * checked.  Out: ref, worst_margin_db = min over the checked bins of limit - level and the frequency it lies at, the number of
 * bins with level > limit, and oob_max_db = max level over |f_k| >= oob_from_hz with its frequency (callers default to 970 kHz,
 * which is only a default; -infinity when no bin lies there).  With n_points = 0 only ref and oob_max_db are formed (worst_margin_db 0, n_checked 0).  Refused
 * (DABGPU_E_INVALID, dabgpu_last_error(NULL)): null raw / out, nfft < 2, a rate_hz with no bin in the band, offsets not strictly
 * increasing, a ref that is zero or not finite. */
typedef struct dabgpu_mask_result {
    double ref;
    double worst_margin_db, worst_freq_hz;
    int n_violations, n_checked;
    double oob_max_db, oob_freq_hz;
} dabgpu_mask_result;
DABGPU_API int dabgpu_spectrum_check_mask(const double *raw, int nfft, double rate_hz, const double *offs_hz,
                                          const double *limit_db, int n_points, double oob_from_hz, dabgpu_mask_result *out);

/* ---- DPD measurement: align the feedback capture, bin AM/AM and AM/PM, fit MemlessPoly ----------------------------------- *
 * The numbers dabgpu_set_poly takes, from a block of transmitted samples (tx: complexf, format 0, or DABGPU_FMT_S16) and the
 * matching capture of the amplifier's feedback path (rx: complexf), n samples each, without the IQ leaving the device.  The
 * reference does this outside the modulator (python/dpd: ExtractStatistic.py, Model_Poly.py); no entry is named *_process.
 * Three steps: cross-spectrum -> alignment (host), aligned statistics per amplitude bin, polynomial fit (host).
 * dabgpu_dpd_xspectrum_dev / dabgpu_dpd_xspectrum: a Welch cross-spectrum in the spectrum monitor's geometry -- segments of
 *   2048 samples at a hop of 1024, rectangular window; segment i of tx is samples 1024 i ... 1024 i + 2047, of rx the same
 *   range shifted by rx_offset; a segment whose rx range leaves the buffer is not used.  Per bin (FFT order) S += TX conj(RX),
 *   P_tx += |TX|^2, P_rx += |RX|^2: fp32 transforms and products, float64 sums, no floating-point atomics (the sums repeat
 *   bit for bit; they agree to float64 reordering across run geometries).  Every call starts the sums over.
 *   dabgpu_get_dpd_xspectrum waits and returns S (2048 complex doubles, re / im interleaved), P_tx, P_rx and the number of
 *   segments used (any pointer may be NULL).
 * dabgpu_dpd_solve_alignment: host only, no context.  c = inverse DFT of conj(S); lag = the l in -1024 ... 1023 of the largest
 *   |c[l]|; tau in (-1, 1) maximises |sum_k conj(S[k]) e^{j w_k (lag + tau)}|, w_k = 2 pi f_k / 2048 with f_k the signed bin
 *   number, found to better than 1e-9 in float64 (a scan at 1/32 sample, then bisection on the derivative of that power,
 *   which a search on the power itself cannot reach: it is flat to 1e-8 around its maximum); gain = sum_k S[k] e^{-j w_k (lag + tau)} /
 *   sum P_rx, the least-squares gain that maps the aligned rx onto tx; coherence = |sum_k S[k] e^{-j w_k (lag + tau)}|^2 /
 *   (sum P_tx sum P_rx).  rx[i + lag + tau] belongs to tx[i].
 * dabgpu_dpd_align_dev / dabgpu_dpd_align: two cross-spectrum passes and two solves.  Pass 1 at offset 0 gives the integer
 *   lag, refused with a message when |lag| > DABGPU_DPD_MAX_LAG; pass 2 at rx_offset = lag gives tau, gain and coherence (and
 *   moves lag by one where pass 1 landed next to the peak).  Waits for the device: the result is host data.
 * dabgpu_dpd_delay_taps: host only.  taps[j] = sinc(j - 15 - tau) kaiser(j - 15 - tau), Kaiser window with beta = 10 over
 *   +-16 samples around the sinc's peak, so that sum_j taps[j] x[i + j - 15] is x at i + tau; tau = 0 gives the unit impulse at tap 15 exactly.
 *   |tau| < 1.
 * dabgpu_dpd_measure_dev / dabgpu_dpd_measure: the statistics.  The aligned rx sample of tx sample i is
 *   r = gain * sum_{j=0..31} taps[j] rx[i + lag + j - 15] (taps of al->tau, fp32); al = NULL means lag 0, tau 0, gain 1.
 *   Sample i is used if and only if all 32 taps lie inside rx, whatever tau is.  a2 = re re + im im of the tx sample in fp32,
 *   each operation rounded (no fused multiply-add); its bin is b = #{ j >= 1 : edge2[j] <= a2 } with edge2[j] the fp32
 *   rounding of (j peak / n_bins)^2 formed in float64; n_bins is 1 ... DABGPU_DPD_MAX_BINS (the reference uses 64).  a2 >=
 *   edge2[n_bins] counts as overflow and lands in no bin.  Two differences from ExtractStatistic.py: its strict inequalities
 *   on both sides drop a sample that sits exactly on an edge, here it belongs to the bin above; and it keeps only the first
 *   ES_n_per_bin samples of a bin in arrival order, which has no meaning on a device -- here every sample counts.
 *   Per bin: n, sum |t|, sum |r|, sum phi, sum |r|^2, sum phi^2 with phi = atan2(Im(r conj t), Re(r conj t)).  Each term is
 *   rounded once to an integer -- |t| and |r| in units of peak 2^-24, |r|^2 in units of peak^2 2^-24, phi in units of 2^-24
 *   rad, phi^2 in units of 2^-24 rad^2 -- and integers are added: the sums are the same bits for every repetition and every
 *   run geometry.  |r| is clamped at 16 peak, so no term passes 2^32, and the sums hold at most 2^31 samples: a call whose n
 *   would take the samples offered since the sums started over past 2^31 is refused.  accumulate 0 starts the sums over;
 *   otherwise the call adds to them and must use the peak and n_bins they were formed with.
 * dabgpu_get_dpd_stats: waits; counts, the sums as doubles in their natural units, the raw integers (raw[b][0..5] = n,
 *   sum |t|, sum |r|, sum phi, sum |r|^2, sum phi^2), overflow, samples_used (overflow included), peak, n_bins.
 * dabgpu_reset_dpd: sums to zero, peak and n_bins forgotten.
 * dabgpu_dpd_fit_poly: host only, no context.  Bins with n >= min_count are used; per bin t = mean |t|, r = mean |r|, p = mean
 *   phi.  DABGPU_DPD_BASIS_MAGSQ (the default) is indirect learning for the predistorter this library runs, which evaluates both
 *   polynomials in |x|^2 (src/MemlessPoly.cpp:244-258): t ~ sum am[i] r^(2i+1), p ~ sum pm[i] r^(2i); MemlessPoly applies
 *   -sum pm, so am and pm go to dabgpu_set_poly as they are.  DABGPU_DPD_BASIS_REFERENCE restates Model_Poly.py, which fits
 *   powers of the amplitude and therefore does NOT fit MemlessPoly: tx = sum c_i rx^i (i = 1 ... 5), phase = sum c_i tx^i
 *   (i = 0 ... 4), tx the bin CENTRE (ExtractStatistic._tx_value_per_bin), phase zero where tx < tx_min, over the leading run
 *   of bins with n >= min_count (the reference's crop rule with "full" replaced), tx / rx / phase rounded to fp32 as the
 *   arrays Model_Poly.train takes are, and every power rounded to fp32 as `sig ** i` on those arrays is: the correctly
 *   rounded power, which numpy's plain float32 power gives.  (numpy's AVX-512 float32 power is off by up to an ulp per entry
 *   and moves Model_Poly's own coefficients by some 1e-5 from machine to machine; the pin is against the former.)  Either way: columns scaled by the largest abscissa, Householder QR in float64, rows times
 *   sqrt(n) when `weighted`.  out = prev + lr (fit - prev), applied ONCE (prev NULL: am 1 0 0 0 0, pm 0).  Model_Poly.train
 *   applies its rate twice, so the reference's effective rate is lr^2; the two agree at lr = 1.  info (may be
 *   NULL): bins used, max |R_kk| / min |R_kk| of each scaled system and each fit's rms residual.  Fewer than six usable
 *   bins is refused.
 * Refused with DABGPU_E_INVALID and a message before anything is queued: a tx format other than 0 / DABGPU_FMT_S16, a pointer
 * not aligned to the sample size, a null pointer with samples, n_bins outside 1 ... 256, peak <= 0 or not finite, another peak
 * or n_bins while accumulating, the sample cap, |al->lag| > DABGPU_DPD_MAX_LAG, |al->tau| >= 1, |rx_offset| > 2^40. */
#define DABGPU_DPD_MAX_LAG 1000
#define DABGPU_DPD_MAX_BINS 256
#define DABGPU_DPD_BASIS_MAGSQ 0
#define DABGPU_DPD_BASIS_REFERENCE 1
typedef struct dabgpu_dpd_alignment {
    int lag;
    double tau;
    double gain_re, gain_im;
    double coherence;
} dabgpu_dpd_alignment;
typedef struct dabgpu_dpd_stats {
    int n_bins;
    float peak;
    uint64_t overflow, samples_used;
    uint64_t count[DABGPU_DPD_MAX_BINS];
    double sum_tx[DABGPU_DPD_MAX_BINS], sum_rx[DABGPU_DPD_MAX_BINS], sum_phase[DABGPU_DPD_MAX_BINS];
    double sum_rx2[DABGPU_DPD_MAX_BINS], sum_phase2[DABGPU_DPD_MAX_BINS];
    int64_t raw[DABGPU_DPD_MAX_BINS][6];
} dabgpu_dpd_stats;
typedef struct dabgpu_dpd_fit_info {
    int bins_used;
    double cond_am, cond_pm;
    double resid_am, resid_pm;
} dabgpu_dpd_fit_info;
DABGPU_API int dabgpu_dpd_xspectrum_dev(dabgpu_ctx *ctx, const void *d_tx, int tx_format, const void *d_rx, size_t n_samples,
                                        long long rx_offset, void *stream);
DABGPU_API int dabgpu_dpd_xspectrum(dabgpu_ctx *ctx, const void *tx, int tx_format, const void *rx, size_t n_samples,
                                    long long rx_offset);
DABGPU_API int dabgpu_get_dpd_xspectrum(dabgpu_ctx *ctx, double *s2048x2, double *p_tx2048, double *p_rx2048,
                                        uint64_t *segments);
DABGPU_API int dabgpu_dpd_solve_alignment(const double *s2048x2, const double *p_tx2048, const double *p_rx2048,
                                          dabgpu_dpd_alignment *out);
DABGPU_API int dabgpu_dpd_align_dev(dabgpu_ctx *ctx, const void *d_tx, int tx_format, const void *d_rx, size_t n_samples,
                                    dabgpu_dpd_alignment *out, void *stream);
DABGPU_API int dabgpu_dpd_align(dabgpu_ctx *ctx, const void *tx, int tx_format, const void *rx, size_t n_samples,
                                dabgpu_dpd_alignment *out);
DABGPU_API int dabgpu_dpd_delay_taps(double tau, float taps[32]);
DABGPU_API int dabgpu_dpd_measure_dev(dabgpu_ctx *ctx, const void *d_tx, int tx_format, const void *d_rx, size_t n_samples,
                                      const dabgpu_dpd_alignment *al, float peak, int n_bins, int accumulate, void *stream);
DABGPU_API int dabgpu_dpd_measure(dabgpu_ctx *ctx, const void *tx, int tx_format, const void *rx, size_t n_samples,
                                  const dabgpu_dpd_alignment *al, float peak, int n_bins, int accumulate);
DABGPU_API int dabgpu_get_dpd_stats(dabgpu_ctx *ctx, dabgpu_dpd_stats *out);
DABGPU_API int dabgpu_reset_dpd(dabgpu_ctx *ctx);
/* diagnostics: segments per workgroup of dpd_xspectrum_kernel (0, the default: about 1024 workgroups, four segments or more
 * each) and tx samples per workgroup of dpd_stats_kernel (a multiple of 256 up to 2048; 0, the default: 2048).  The
 * cross-spectrum agrees to float64 reordering for every value, the statistics are the same bits. */
DABGPU_API int dabgpu_debug_dpd_run_segments(dabgpu_ctx *ctx, int segments);
DABGPU_API int dabgpu_debug_dpd_tile(dabgpu_ctx *ctx, int samples);
DABGPU_API int dabgpu_dpd_fit_poly(const dabgpu_dpd_stats *stats, int basis, uint64_t min_count, int weighted, double tx_min,
                                   const float prev_am[5], const float prev_pm[5], double lr_am, double lr_pm, float am[5],
                                   float pm[5], dabgpu_dpd_fit_info *info);

/* ---- the channel: sparse multipath, a Doppler rotation per path, seeded Gaussian noise, on a sample stream ------------------ *
 * The stage between the modulator's IQ and the receiver (dabgpu_sync*, dabgpu_demod*): what a channel emulator next to a
 * modulator does, on samples that are on the device already.  The reference has no such stage; these entries replace nothing
 * of its flowgraph.  The output is a function of the input stream, the settings, the seed and the absolute sample position
 * alone: a stream cut into calls of any lengths gives the bytes of one call.
 * Let a = position + i be the absolute index of sample i of a call; `position` counts the samples the stream has taken since
 * the last dabgpu_channel_reset (0 before the first), x[.] is the input stream, zero before the reset:
 *   y[a] = sum_{p < n_paths} g_p e^{j 2 pi theta_p(a)} x[a - d_p]  +  sigma (n_re(a) + j n_im(a))
 * Paths: 0 <= n_paths <= DABGPU_CH_MAX_PATHS.  d_p = delay, an integer number of samples, 0 ... DABGPU_CH_MAX_DELAY (2047: 1 ms
 *   at the native rate, longer than every guard interval -- Mode I's is 504 samples).  g_p = gain_re + j gain_im, fp32; it
 *   carries the path's initial phase.
 * Doppler: step_p = rint(doppler_hz / rate_hz 2^64) as a two's-complement 64-bit integer (both float64, the quotient first;
 *   |doppler_hz| < rate_hz / 2, rate_hz > 0: 2 048 000 for the native rate, the output rate for a resampled chain);
 *   theta_p(a) = (the upper 32 bits of a step_p mod 2^64) / 2^32: an integer phase, nothing accumulates along the stream.  The
 *   rotation is e^{j 2 pi theta}: the nearest quarter turn comes off theta exactly in integers, the rest (at most 1/8 turn, 30
 *   bits) is rounded to fp32 once and goes through sincospif -- dabgpu_sync_extract's rotation.  A carrier offset is the same
 *   Doppler on every path.
 * Path sum, in fp32, complex products as (re re - im im, re im + im re) with one fused multiply-add each:
 *   S0 = the sum of g_p x[a - d_p] over the paths with step_p = 0, in their given order, starting from zero (such a path
 *        multiplies by g_p alone);
 *   S1 = the sum of (g_p e^{j 2 pi theta_p(a)}) x[a - d_p] over the paths with step_p != 0, in their given order, starting
 *        from zero;  y = (S0 + S1) + sigma n, the last step one fused multiply-add per component, left out when sigma = 0.
 * Noise: Philox4x32-10 (Salmon et al., SC11) with the key (seed mod 2^32, seed >> 32) and the counter (c mod 2^32, c >> 32, 0,
 *   0), c = a >> 1.  Of its four output words w0 ... w3 an even a takes (wa, wb) = (w0, w1), an odd a (w2, w3).
 *   u = ((wa >> 9) + 0.5) 2^-23 (exact in fp32, never 0 or 1);  r = sqrtf(-2 logf(u));
 *   n_re + j n_im = r (cos, sin)(2 pi wb / 2^32), the angle reduced exactly as above.
 *   The components are unit Gaussians CUT OFF at sqrt(48 ln 2) = 5.77 (u >= 2^-24).  sigma >= 0 is fp32 and absolute, per
 *   component; with sigma = 0 no generator runs.
 * Formats: input complexf (format 0) or DABGPU_FMT_S16 (a value becomes its float on load, as in dabgpu_demod*); output
 *   complexf or DABGPU_FMT_S16 -- dabgpu_format_process's conversion of the complexf result byte for byte (saturating,
 *   toward zero), without a clip count.  u8 / s8 are refused.
 * State: the last 2047 input samples, kept as floats, and `position`.  Calls may mix the two input formats.
 * dabgpu_channel_check: host only, no context, no device: the refusals of the settings, message via dabgpu_last_error(NULL).
 * dabgpu_set_channel: installs a configuration; history and position stay.  It takes effect at the next call and is ordered
 *   behind the calls queued before it (the path table travels with each launch).
 * dabgpu_channel_reset: zero history, the stream continues at `position` (the next call zeroes it, on its own stream).
 * dabgpu_get_channel_position: waits for the most recent call, as dabgpu_get_sync_result does.
 * dabgpu_channel_dev: device pointers (aligned to a sample), asynchronous on `stream` (NULL: the context's own stream, behind
 *   every lane); two launches, no host round trip.  The calls carry stream state: the caller keeps them in order.
 *   dabgpu_channel: the host-pointer form.
 * Refused with DABGPU_E_INVALID and a message before anything is queued (position, history and the output untouched): a null
 *   pointer or one not aligned to a sample, n_samples = 0 (or above 2^40), input and output ranges that overlap, a format
 *   other than the two, more than 64 paths, a delay above 2047, a gain or sigma that is not finite, sigma < 0, rate_hz <= 0,
 *   |doppler_hz| >= rate_hz / 2, a call before any dabgpu_set_channel.
 * Out of scope: fractional-sample delays, sampling-clock offset (since built: the clock), correlated (Jakes) fading inside the kernel (the caller
 *   composes it from paths: a sum of sinusoids per delay), u8 / s8. */
#define DABGPU_CH_MAX_PATHS 64
#define DABGPU_CH_MAX_DELAY 2047
typedef struct dabgpu_channel_path {
    uint32_t delay;
    float gain_re, gain_im;
    double doppler_hz;
} dabgpu_channel_path;
typedef struct dabgpu_channel_config {
    uint32_t n_paths;
    float sigma;
    uint64_t seed;
    double rate_hz;
    dabgpu_channel_path paths[DABGPU_CH_MAX_PATHS];
} dabgpu_channel_config;
DABGPU_API int dabgpu_channel_check(const dabgpu_channel_config *cfg);
DABGPU_API int dabgpu_set_channel(dabgpu_ctx *ctx, const dabgpu_channel_config *cfg);
DABGPU_API int dabgpu_channel_reset(dabgpu_ctx *ctx, uint64_t position);
DABGPU_API int dabgpu_get_channel_position(dabgpu_ctx *ctx, uint64_t *position);
DABGPU_API int dabgpu_channel_dev(dabgpu_ctx *ctx, const void *d_in, int in_format, size_t n_samples, void *d_out,
                                  int out_format, void *stream);
DABGPU_API int dabgpu_channel(dabgpu_ctx *ctx, const void *in, int in_format, size_t n_samples, void *out, int out_format);
/* Diagnostic: samples per workgroup of the channel's kernel (rounded up to a multiple of 4); 0 (the default) = chosen from the
 * call size.  Same bytes for every value; exists so that a test can walk the run geometry. */
DABGPU_API int dabgpu_debug_channel_run_samples(dabgpu_ctx *ctx, int samples);

/* ---- the clock: a sampling-clock offset on a sample stream -- put on, taken off (the resampler) and measured (the estimator) - *
 * No capture is made on the transmitter's clock.  The resampler emulates a relative clock offset delta = ppm 1e-6 on samples
 * that are on the device already and, with the opposite sign, corrects one; the estimator (further down) reads delta from the
 * data symbols of whole frames.  The reference has no such stage; these entries replace nothing of its flowgraph.  The output
 * is a function of the input stream, ppm and the absolute output index alone: a stream cut into calls of any lengths gives the
 * bytes of one call.  delta > 0: the capture runs through the signal faster, y[m] ~ x(m (1 + delta)).
 * Step and position: step = llrint(ppm 1e-6 2^64), the product evaluated in float64 from the left, an int64; |ppm| <= 1000.
 *   For the absolute output index m >= 0: D(m) = m step as a signed 128-bit product; the input position
 *   i_m = m + floor(D / 2^64); F = the upper 32 bits of the low 64 bits of D; mu = F / 2^32.  Nothing accumulates along the
 *   stream: every output is a function of m alone.  A slip is where floor(D / 2^64) steps: i_m advances by 2, or by 0 for
 *   delta < 0.
 * Output: y[m] = sum_{j = 0 ... 31} h_j(mu) x[i_m + j - 15], x[.] the input stream counted from the last reset's position,
 *   zero before the reset.
 * Taps: a table T[p][j], p = 0 ... 512 (DABGPU_CLOCK_PHASES + 1 rows of DABGPU_CLOCK_TAPS).  Row p < 512 is
 *   dabgpu_dpd_delay_taps(p / 512): sinc(j - 15 - tau) kaiser(beta = 10 over +-16 samples), float64 rounded to fp32 once; row 0
 *   is the unit impulse at tap 15; row 512 is the unit impulse at tap 16 (dabgpu_clock_phase_taps returns any row).
 *   p = F >> 23, f = (F & 0x7fffff) 2^-23 (exact in fp32), h_j = fmaf(f, T[p + 1][j] - T[p][j], T[p][j]), the difference an
 *   fp32 subtraction.
 * Sum, in fp32, the ONE order of every instantiation: re = im = +0; for j = 0, 1, ... 31 in this order
 *   re = fmaf(h_j, Re x[i_m + j - 15], re), im = fmaf(h_j, Im x[i_m + j - 15], im).  With ppm = 0 the output is the input
 *   (a negative zero comes out positive).
 * Formats: input complexf (format 0) or DABGPU_FMT_S16 (a value becomes its float on load); output complexf or DABGPU_FMT_S16
 *   -- dabgpu_format_process's conversion of the complexf result byte for byte (saturating, toward zero), without a clip
 *   count.  u8 / s8 are refused.  Calls may mix the formats.
 * State: T, the absolute number of input samples received (the reset's position included), and the last 31
 *   (DABGPU_CLOCK_HISTORY) input samples, kept as floats in two buffers that take turns.  M(T) = the number of m >= 0 with
 *   i_m + 16 <= T - 1: the outputs all of whose taps have arrived (= ceil((T - 16) 2^64 / (2^64 + step)), 0 for T <= 16).  A
 *   call that brings n_in samples writes the outputs M(T) ... M(T + n_in) - 1 and returns their count in *n_out (it may be
 *   0); the first of them has i_m + 16 >= T, so it reads no further back than T - 31.  The count is integer arithmetic on
 *   the host, before anything is queued: no device round trip.  dabgpu_clock_count gives M, dabgpu_clock_out_max(n_in) =
 *   n_in + n_in / 999 + 2 bounds the count of any call of n_in samples.  The output trails the input by 16 samples: after T
 *   inputs at ppm = 0, outputs 0 ... T - 17 exist.
 * dabgpu_clock_check, dabgpu_clock_step, dabgpu_clock_count, dabgpu_clock_out_max, dabgpu_clock_phase_taps,
 *   dabgpu_clock_inverse_ppm: host only, no context, no device; message via dabgpu_last_error(NULL).
 *   dabgpu_clock_inverse_ppm(ppm) = -ppm / (1 + ppm 1e-6): the setting that undoes delta, -delta / (1 + delta).
 * dabgpu_set_clock: installs ppm and implies dabgpu_clock_reset(0).  Ordered behind the calls queued before it (the step
 *   travels with each launch); the first one uploads the table.
 * dabgpu_clock_reset: T = position (at most 2^62) with a zero history: the next call starts at output M(position).
 * dabgpu_get_clock_position: T; waits for the most recent call, as dabgpu_get_channel_position does.
 * dabgpu_clock_dev: device pointers (aligned to a sample), out_cap in samples, asynchronous on `stream` (NULL: the
 *   context's own stream, behind every lane -- the calls stay on lane 0 in call order); at most two launches, no host round
 *   trip.  The calls carry stream state: the caller keeps them in order.  dabgpu_clock: the host-pointer form.
 * Refused with DABGPU_E_INVALID and a message before anything is queued (position, history and the output untouched): a ppm
 *   that is not finite or above 1000 in magnitude, a format other than the two, a null pointer or one not aligned to a
 *   sample, input and output ranges that overlap, n_in = 0 (or above 2^40), a position beyond 2^62, a call before any
 *   dabgpu_set_clock.  An out_cap below the call's count: DABGPU_E_CAPACITY, the count in *n_out, nothing queued.
 * Out of scope: a state blob or seed for the clock's history, tracking across calls, a time-varying offset, u8 / s8,
 *   dabmod_file options (an offset moves the frames across its batch boundaries, which takes the synchroniser across
 *   batches). */
#define DABGPU_CLOCK_TAPS 32
#define DABGPU_CLOCK_PHASES 512
#define DABGPU_CLOCK_HISTORY 31
DABGPU_API int dabgpu_clock_check(double ppm);
DABGPU_API int dabgpu_clock_step(double ppm, int64_t *step);
DABGPU_API int dabgpu_clock_count(double ppm, uint64_t T, uint64_t *M);
DABGPU_API size_t dabgpu_clock_out_max(size_t n_in);
DABGPU_API int dabgpu_clock_phase_taps(int p, float taps[32]);
DABGPU_API double dabgpu_clock_inverse_ppm(double ppm);
DABGPU_API int dabgpu_set_clock(dabgpu_ctx *ctx, double ppm);
DABGPU_API int dabgpu_clock_reset(dabgpu_ctx *ctx, uint64_t position);
DABGPU_API int dabgpu_get_clock_position(dabgpu_ctx *ctx, uint64_t *position);
DABGPU_API int dabgpu_clock_dev(dabgpu_ctx *ctx, const void *d_in, int in_format, size_t n_in, void *d_out, int out_format,
                                size_t out_cap, size_t *n_out, void *stream);
DABGPU_API int dabgpu_clock(dabgpu_ctx *ctx, const void *in, int in_format, size_t n_in, void *out, int out_format,
                            size_t out_cap, size_t *n_out);
/* Diagnostic: outputs per workgroup of the clock's kernel (at most 2048); 0 (the default) = 1024.  Same bytes for every
 * value; exists so that a test can walk the run geometry. */
DABGPU_API int dabgpu_debug_clock_run_samples(dabgpu_ctx *ctx, int samples);

/* The clock's estimator: the offset of whole frames from their data symbols, decision directed.  Input: whole transmission
 * frames at the native rate as dabgpu_demod* takes them (a chain's output, or dabgpu_sync_extract's), complexf or
 * DABGPU_FMT_S16; `early` as for dabgpu_demod*, refused the same way.  n_frames = 1 ... max_frames.
 * Per frame, over its data blocks b and the occupied carriers k: d_{b,k} = z_s conj(z_{s-1}) is exactly dabgpu_demod's product
 *   (s = b + 2), c its decided point, and in fp32
 *   e = d conj(c) = (|Re d| + |Im d|) / sqrt 2 + j (Im d sgn Re d - Re d sgn Im d) / sqrt 2,  sgn x = -1 where x < 0, else +1;
 *   |e| = sqrtf(fmaf(Re e, Re e, Im e Im e)).
 * Sums: A_hi = sum of e over the carriers k = 1 ... K/2, A_lo = over k = -K/2 ... -1, S = sum of |e|, each over all data
 *   blocks: float64 sums of the fp32 terms in a FIXED order -- per block the lane's carriers, a butterfly inside the wave, the
 *   waves in wave order; then (a second kernel) the blocks in index order -- so a record repeats byte for byte and does not
 *   depend on the run geometry (dabgpu_debug_demod_run_symbols sets it for this kernel too).
 * Derived, in float64 on the host: ppm = 1e6 arg(A_hi conj(A_lo)) / (2 pi (sym_size / spacing) (K/2 + 1)) -- a clock offset
 *   delta turns carrier k of d by 2 pi k delta sym_size / spacing, and with carriers of equal amplitude the two halves' mean
 *   phases lie (K/2 + 1) carriers apart; residual_cfo = arg(A_hi + A_lo) / (2 pi sym_size / spacing), in carrier spacings;
 *   quality = |A_hi + A_lo| / S; valid = (S > 0), and a frame that is not valid has every figure 0.
 * The sign convention is the resampler's delta: a capture made by dabgpu_set_clock(p) reads +p, and
 *   dabgpu_clock_inverse_ppm(estimate) is the setting that takes it off.  Working range: |2 pi (K/2) delta sym_size / spacing|
 *   < pi/4, where the edge carriers reach the decision boundary (about +-130 ppm in Mode I); the drift of the FFT window
 *   along the frame (delta x the frame's samples) must stay inside what `early` leaves of the cyclic prefix.  Amplitude slopes
 *   across the band (an echo, a filter's edge) bias the estimate multiplicatively -- the sums weigh a carrier by |d| -- so
 *   one estimate-and-correct pass leaves a residual of second order.
 * dabgpu_sco_dev: a device pointer aligned to a sample, asynchronous on `stream` (NULL: the context's own stream, behind
 *   every lane); two launches, no atomics, no host round trip.  dabgpu_sco: the host-pointer form.
 * dabgpu_get_sco: waits for the most recent call, as the other getters do; frame = 0 ... n_frames - 1, or -1: the figures
 *   from the sums over all valid frames, added in frame order.
 * Out of scope: tracking across calls, a time-varying offset, weighting by a channel estimate, u8 / s8. */
typedef struct dabgpu_sco_frame {
    double a_hi_re, a_hi_im, a_lo_re, a_lo_im, s;   /* the raw sums */
    double ppm, residual_cfo, quality;
    int32_t valid, reserved;
} dabgpu_sco_frame;
DABGPU_API int dabgpu_sco_dev(dabgpu_ctx *ctx, const void *d_iq, int format, size_t n_frames, int early, void *stream);
DABGPU_API int dabgpu_sco(dabgpu_ctx *ctx, const void *iq, int format, size_t n_frames, int early);
DABGPU_API int dabgpu_get_sco(dabgpu_ctx *ctx, int frame, dabgpu_sco_frame *out);

/* ---- the tuner: any capture rate and offset down to native-rate IQ -- mix, channel-filter, decimate ------------------------- *
 * Everything on the receive side takes IQ at 2.048 MS/s.  The tuner is the stage in front of it: a position-exact polyphase
 * rate converter L / M with a mixer in front, for the transmitter's own resampled output (dabgpu_set_resampler's chains) and for
 * the captures receivers make (2.4, 2.5, 2.56, 3.2, 10 MS/s ..., a wide capture with several blocks in it: one tuner each).
 * The reference has no such stage; these entries replace nothing of its flowgraph.  Every output is a function of the input
 * stream, the setting and its absolute index alone: a stream cut into calls of any lengths gives the bytes of one call.
 * Settings: dabgpu_tuner_config { in_rate_hz, selectivity, offset_hz }.
 * Ratio: g = gcd(2 048 000, in_rate_hz), L = 2 048 000 / g, M = in_rate_hz / g.  Accepted: in_rate_hz >= 2 048 000,
 *   L <= 512 (DABGPU_TUNER_MAX_L), M <= 8 L.  That covers 2.048 (1/1), 2.304 (8/9), 2.4 (64/75), 2.5 (512/625), 2.56 (4/5),
 *   3.072 (2/3), 3.2 (16/25), 4.096 (1/2), 6.144 (1/3), 8.192 (1/4), 10.0 (128/625) and 16.384 (1/8) MS/s.
 * Tap count: D = ceil(M / L) (1 at ratio 1); taps per output P = 32 D for selectivity 0 ("wide") and 96 D for 1 ("channel");
 *   at most 768 (DABGPU_TUNER_MAX_TAPS).
 * Mixer: r[n] = x[n] exp(2 pi j frac(n step / 2^64)), n the absolute input index, step = rint(-offset_hz / in_rate_hz 2^64)
 *   as an int64 (the quotient and the product in float64, from the left), the product n step modulo 2^64.  The phase is
 *   taken from the upper 32 bits of that product: the nearest quarter turn comes off in integers, the rest is rounded to fp32
 *   once.  Nothing accumulates.  |offset_hz| < in_rate_hz / 4.  A signal at +offset_hz in the capture comes out at 0.  With
 *   step = 0 the sample's bits pass: no multiply.  Otherwise, with w the phase's (cos, sin) in fp32:
 *   Re r = fmaf(Re x, Re w, -(Im x Im w)), Im r = fmaf(Re x, Im w, Im x Re w), the inner products rounded.
 * Position: for the absolute output index m >= 0: q = m M, i_m = q div L, p = q mod L, in integers; positions up to 2^50
 *   input samples.
 * Output: y[m] = sum_{j = 0 ... P - 1} T[p][j] r[i_m + j - (P/2 - 1)], r[.] the mixed input stream counted from the last
 *   reset's position, zero before the reset.
 * Taps: T[p][j] = fp32(h_j / sum_j h_j + 0), h and the sum (in the order j = 0 ... P - 1) in float64, with
 *   t = j - (P/2 - 1) - p / L, c = min(1, B / in_rate_hz), B = 2 048 000 for wide (-6 dB at 1024 kHz) and 1 712 000 for channel
 *   (-6 dB at 856 kHz, halfway between the block's edge at 768 kHz and the neighbour's at 944 kHz), and
 *   h = c sinc(c t) I0(10 sqrt(1 - (t / (P/2))^2)) / I0(10) for |t| <= P/2, else 0.
 *   sinc(x) = 1 at x = 0, else (-1)^n sin(pi (x - n)) / (pi x) with n = x rounded to the nearest integer (ties to even), so that
 *   it is exactly 0 at every other integer; I0(x) = sum_k ((x/2)^k / k!)^2, the terms formed by term *= (x / 2k)(x / 2k),
 *   added from k = 0 until one is below 1e-18 of the sum.  At 2.048 MS/s wide every row is the unit impulse at tap 15.
 * Sum, in fp32, the ONE order of every instantiation: re = im = +0; for j = 0, 1, ... P - 1 in this order
 *   re = fmaf(T[p][j], Re r, re), im = fmaf(T[p][j], Im r, im).
 * Formats: input complexf (format 0), DABGPU_FMT_S16, DABGPU_FMT_U8 (byte - 128) or DABGPU_FMT_S8, as dabgpu_spectrum* loads
 *   them (a value becomes its float on load); output complexf or DABGPU_FMT_S16 -- dabgpu_format_process's conversion of the
 *   complexf result byte for byte (saturating, toward zero), without a clip count.  Calls may mix the formats.
 * State: T, the absolute number of input samples received (the reset's position included), and the last P - 1 input samples,
 *   kept as floats (not mixed) in two buffers that take turns.  M(T) = the number of m >= 0 with i_m + P/2 <= T - 1: the
 *   outputs all of whose taps have arrived (= ceil((T - P/2) L / M), 0 for T <= P/2).  A call that brings n_in samples writes
 *   the outputs M(T) ... M(T + n_in) - 1 and returns their count in *n_out (it may be 0).  The count is integer arithmetic on
 *   the host, before anything is queued: no device round trip.  dabgpu_tuner_count gives M, dabgpu_tuner_out_max(cfg, n_in) =
 *   ceil(n_in L / M) + 1 bounds the count of any call of n_in samples (0 for a setting that is refused).  The output trails
 *   the input by P/2 input samples: at 2.048 MS/s wide and offset 0 it is the input's bytes, trailing by 16 (a negative zero
 *   comes out positive).
 * dabgpu_tuner_check, dabgpu_tuner_geometry, dabgpu_tuner_taps (row p = 0 ... L - 1, P floats), dabgpu_tuner_count,
 *   dabgpu_tuner_out_max: host only, no context, no device; message via dabgpu_last_error(NULL).
 * dabgpu_set_tuner: installs a setting and implies dabgpu_tuner_reset(0); uploads the tap table when rate or selectivity
 *   change, after the tuner's queued calls have finished.
 * dabgpu_tuner_reset: T = position (at most 2^50) with a zero history: the next call starts at output M(position).
 * dabgpu_get_tuner_position: T; waits for the most recent call, as dabgpu_get_clock_position does.
 * dabgpu_tuner_dev: device pointers (aligned to a sample of their format), out_cap in samples, asynchronous on `stream` (NULL:
 *   the context's own stream, behind every lane -- the calls stay on lane 0 in call order); at most two launches, no host
 *   round trip.  The calls carry stream state: the caller keeps them in order.  dabgpu_tuner: the host-pointer form.
 * Refused with DABGPU_E_INVALID and a message before anything is queued (position, history and the output untouched): a rate
 *   below 2 048 000 or with L above 512 or M above 8 L, a selectivity other than 0 and 1, an offset that is not finite or not
 *   below in_rate_hz / 4 in magnitude, an input format other than the four or an output format other than the two, a null
 *   pointer or one not aligned to a sample, input and output ranges that overlap, n_in = 0 (or above 2^40), a position beyond
 *   2^50, a call before any dabgpu_set_tuner.  An out_cap below the call's count: DABGPU_E_CAPACITY, the count in *n_out,
 *   nothing queued.
 * Out of scope: input rates below 2.048 MS/s, a time-varying offset, a state blob or seed for the history, dabmod_file
 *   options (the resampler's delay moves the frames across its batch boundaries), and the monitor on resampled chains
 *   (dabgpu_set_monitor still refuses them). */
#define DABGPU_TUNER_MAX_L 512
#define DABGPU_TUNER_MAX_TAPS 768
typedef struct dabgpu_tuner_config {
    uint32_t in_rate_hz;
    int selectivity;          /* 0: wide (32 D taps), 1: channel (96 D taps) */
    double offset_hz;
} dabgpu_tuner_config;
DABGPU_API int dabgpu_tuner_check(const dabgpu_tuner_config *cfg);
DABGPU_API int dabgpu_tuner_geometry(const dabgpu_tuner_config *cfg, int *L, int *M, int *P);
DABGPU_API int dabgpu_tuner_taps(const dabgpu_tuner_config *cfg, int p, float *taps);
DABGPU_API int dabgpu_tuner_count(const dabgpu_tuner_config *cfg, uint64_t T, uint64_t *M_out);
DABGPU_API size_t dabgpu_tuner_out_max(const dabgpu_tuner_config *cfg, size_t n_in);
DABGPU_API int dabgpu_set_tuner(dabgpu_ctx *ctx, const dabgpu_tuner_config *cfg);
DABGPU_API int dabgpu_tuner_reset(dabgpu_ctx *ctx, uint64_t position);
DABGPU_API int dabgpu_get_tuner_position(dabgpu_ctx *ctx, uint64_t *position);
DABGPU_API int dabgpu_tuner_dev(dabgpu_ctx *ctx, const void *d_in, int in_format, size_t n_in, void *d_out, int out_format,
                                size_t out_cap, size_t *n_out, void *stream);
DABGPU_API int dabgpu_tuner(dabgpu_ctx *ctx, const void *in, int in_format, size_t n_in, void *out, int out_format,
                            size_t out_cap, size_t *n_out);
/* Diagnostic: outputs per workgroup of the tuner's kernels (at most what the staged span holds, 2048 at most); 0 (the
 * default) = chosen from the setting.  Same bytes for every value; exists so that a test can walk the run geometry. */
DABGPU_API int dabgpu_debug_tuner_run_samples(dabgpu_ctx *ctx, int samples);

/* ---- the TII analyser: transmitters, levels and delays from the null symbols of whole frames -------------------------------- *
 * Reads what dabgpu_set_tii puts into a signal: which (comb, pattern) the null symbols carry, how strong every comb is and
 * when it arrives -- of one transmitter, or of the several of a single-frequency network in one monitoring capture.  The
 * reference has no receiver; these entries replace nothing of its flowgraph.
 * Input: n_frames whole transmission frames at the native rate, each tf_samples long and starting at its frame start -- what a
 * chain call without the Resampler writes, or dabgpu_sync_extract* -- complexf (format 0) or DABGPU_FMT_S16 (a value becomes
 * its float on load).  Modes I and II only (no other carries TII), 2 <= n_frames <= max_frames.
 * With N = spacing, K = carriers, null = null_size, P[k] the phase reference symbol on carrier k, carrier k on bin k mod N, and
 * `early` as dabgpu_demod* means it (the window ends `early` samples before the end of the null symbol; 0 ... null - N):
 *   Cells      (c, b), c = 0 ... 23 (the comb), b = 0 ... 7 (the pattern bit), cell index 8 c + b.  First carriers, EN 300 401
 *              14.8.1 as carrier numbers of the standard: Mode I  k(c, b, g) = {-768, -384, 1, 385}[g] + 2 c + 48 b, g = 0 ... 3;
 *              Mode II  k(c, b) = -192 + 2 c + 48 b for b < 4 and -191 + 2 c + 48 b for b >= 4 (one g).  Every first carrier has
 *              its pair carrier k + 1.  Pattern p is row p of a_b(p): the 70 eight-bit words of weight four in ascending
 *              order, b = 0 the most significant bit.
 *   Per frame  R = DFT_N(x[null - early - N ... null - early)) on the cells' carriers, in float64: R[k] = sum_n x[n]
 *              e^{-j 2 pi ((k n) mod N) / N}, n in order, fused multiply-adds, the twiddles float64 (a clean capture's unset
 *              cells are 1e-14 of the set ones: an fp32 transform's own rounding would be the floor).  In float64, g in order:
 *              E_f(c, b) = sum_g (|R[k]|^2 + |R[k + 1]|^2),  G_f(c, b) = sum_g R[k + 1] conj(R[k]) conj(q_k),
 *              q_k = 1 (new variant) or P[k + 1] conj(P[k]) (old variant).
 *   Parity     total[p] = sum over the cells of (sum of E_f over the frames f = p mod 2, in frame order);  parity = 0 if
 *              total[0] >= total[1], else 1.  Only the n_used frames f = parity mod 2 are used: E(c, b) and G(c, b) are the
 *              sums of E_f and G_f over them, in frame order.
 *   Floor      floor = the 96th smallest of the 192 E(c, b) (a cell's rank: the cells smaller, or equal with a lower index).
 *   Decision   thr = max(min_ratio floor, min_rel max E), in float64;  cell (c, b) is set when E >= thr and E > 0.  A comb with
 *              at least one set cell is an entry; entries are in comb order.  mask = the set bits, b as 0x80 >> b;  n_set;
 *              pattern = the table index of mask when n_set = 4, else -1 (two transmitters on one comb, or a faint one, report
 *              the mask only);  energy = (sum of the set cells' E, b in order) / n_used.
 *   Coarse     tau1 = -arg(sum over the set b of G(c, b), b in order) N / 2 pi (float64 atan2), in samples from the window;
 *              delay_coarse = tau1 - early.  Unambiguous within +-N / 2.
 *   Fine       s = N / 16384 samples (1/8 in Mode I, 1/32 in Mode II);  u_j = rint(tau1 / s) + j, j = -128 ... 127;
 *              H_f[k] = R_f[k] conj(T[k]) (R_f rounded to fp32) on the carriers of the entry's set cells, T[k] = P[k] on a first carrier and on its
 *              pair carrier T[k + 1] = P[k] (new variant) or P[k + 1] (old variant);
 *              S_j = sum_f |sum_k H_f[k] e^{j 2 pi ((k u_j) mod 16384) / 16384}|^2, the inner sum in fp32 (fused multiply-adds,
 *              the phase an exact integer turn) over the carriers in ascending k, the outer in float64 over the used frames in
 *              order;  j* = the first j with the largest S;  delay = u_j* s - early;
 *              runner_up = (the largest S_j with |j - j*| > 16384 / N) / S_j*, 0 when S_j* = 0.
 *              A comb's carriers lie on a lattice of 48 carriers, so S repeats almost unchanged every N / 48 samples; only the
 *              pair carriers resolve that, and coarsely: hence the two stages and the window of +-N / 128 samples.
 * delay = 0: the useful part of the null symbol starts at sample null - N of the frame.  A chain with FIRFilter reads -22 (its
 *   look-ahead, the 22 samples dabgpu_sync* reports as well).  Delays of two entries differ by the transmitters' distance in time.
 * As emitted -- bit-exact to the reference -- a Mode II signal configured with pattern p reads here, by the standard, as the
 *   pattern with bits b and b + 4 exchanged (comb 3, pattern 5 reads as comb 3, pattern 32); Mode I reads as configured.
 *   INTEGRATION.md F has the cause.
 * Every sum and search runs in a fixed order (the lane's own terms in index order, an xor butterfly in the wave, the waves in
 *   wave order; ties go to the first index; no floating-point atomics): a call on the same samples gives the same bytes.
 * dabgpu_tii_scan_dev: device pointer (aligned to a sample), asynchronous on `stream` (NULL: the context's own stream, behind
 *   every lane); three launches, no host round trip.  dabgpu_tii_scan: the host-pointer form.
 * dabgpu_get_tii_scan: waits for the most recent of them, as dabgpu_get_sync_result does; the head, and min(cap, 24) entry
 *   slots to `out`.  The result has a fixed layout: the head (40 bytes), then 24 slots of 48 bytes, zeros behind n_entries.
 * Refused with DABGPU_E_INVALID and a message before anything is queued (the previous result stays): Mode III or IV,
 *   n_frames < 2 or > max_frames, early outside 0 ... null - N, min_ratio not finite or < 1, min_rel outside [0, 1), a format
 *   other than 0 / DABGPU_FMT_S16, a null or misaligned pointer.
 * dabgpu_tii_scan_check: host only, no context, no device: the refusals of mode (1..4; 0 = IV), n_frames (>= 2; max_frames is
 *   the context's) and the settings, message via dabgpu_last_error(NULL).
 * Out of scope: coherent accumulation across frames, more than one pattern per comb resolved, sampling-clock offset (since built: the clock), u8 / s8,
 *   resampled captures. */
typedef struct dabgpu_tii_scan_config { int early, old_variant; float min_ratio, min_rel; } dabgpu_tii_scan_config;
typedef struct dabgpu_tii_scan_head   { int n_used, parity, n_entries, reserved; double floor, total[2]; } dabgpu_tii_scan_head;
typedef struct dabgpu_tii_entry       { int comb, pattern, mask, n_set; double energy, delay_coarse, delay, runner_up; } dabgpu_tii_entry;
DABGPU_API int dabgpu_tii_scan_dev(dabgpu_ctx *ctx, const void *d_frames, int format, size_t n_frames,
                                   const dabgpu_tii_scan_config *cfg, void *stream);
DABGPU_API int dabgpu_tii_scan(dabgpu_ctx *ctx, const void *frames, int format, size_t n_frames, const dabgpu_tii_scan_config *cfg);
DABGPU_API int dabgpu_get_tii_scan(dabgpu_ctx *ctx, dabgpu_tii_scan_head *head, dabgpu_tii_entry *out, size_t cap);
DABGPU_API int dabgpu_tii_scan_check(int mode, size_t n_frames, const dabgpu_tii_scan_config *cfg);

/* ---- the channel estimator: impulse response and echoes from the phase reference symbols of whole frames ------------------- *
 * Reads what dabgpu_set_channel puts into a signal, or what a single-frequency network and the air do: the paths a capture went
 * through, their levels and delays, how much arrives later than the guard interval, and the response on every carrier.  The
 * reference has no receiver; these entries replace nothing of its flowgraph.
 * Input: n_frames whole transmission frames at the native rate, each tf_samples long and starting at its frame start -- what a
 * chain call without the Resampler writes, or dabgpu_sync_extract* -- complexf (format 0) or DABGPU_FMT_S16 (a value becomes
 * its float on load).  All four modes, 1 <= n_frames <= max_frames.
 * With N = spacing, K = carriers, null = null_size, sym = sym_size, CP = sym - N, P[k] the phase reference symbol on carrier k,
 * carrier k on bin k mod N, `early` in 0 ... CP and `window` 0 (rectangular) or 1 (Hann):
 *   Transform  per frame f:  R_f = DFT_N(x_f[w0 ... w0 + N)), w0 = null + CP - early; the samples become float64 on load and the
 *              transform runs in float64 (the profile's floor lies at 1e-6 ... 1e-5 of its peak: an fp32 transform's own
 *              rounding would show in it).
 *   Channel    H_f[k] = R_f[k mod N] conj(P[k]) on the occupied carriers k = -K/2 ... -1, 1 ... K/2, 0 elsewhere.
 *   Weights    i = the position of k in ascending carrier order (k = -K/2 -> 0, k = -1 -> K/2 - 1, k = 1 -> K/2, k = K/2 ->
 *              K - 1);  w_i = 1 (window 0) or 0.5 - 0.5 cos(2 pi (i + 0.5) / K) (window 1), in float64;  S_w = sum_i w_i.
 *   Response   h_f[l] = (1 / S_w) sum_k w H_f[k] e^{+j 2 pi k l / N}, l = 0 ... N - 1, in float64.
 *   Profile    pdp[l] = (1 / n_frames) sum_f |h_f[l]|^2, the frames in order -- non-coherent across frames: residual carrier
 *              offset and Doppler turn the taps from frame to frame.  resp[b] = (1 / n_frames) sum_f |H_f[k]|^2 at bin
 *              b = k mod N, unweighted, 0 on the unoccupied bins.
 *   Floor      floor = the pdp value of rank N/2 - 1, zero-based (a value's rank: the values smaller, or equal with a lower
 *              index).  peak = the largest pdp, peak_index = its first index.
 *   Decision   threshold = max(min_ratio floor, min_rel peak).  Tap l is a peak when pdp[l] > 0, pdp[l] >= threshold,
 *              pdp[l] > pdp[(l - 1) mod N] and pdp[l] >= pdp[(l + 1) mod N].  n_peaks counts them all.
 *   Paths      the DABGPU_CIR_MAX_PATHS = 16 strongest peaks in descending power, a lower index first among equals.  index = l;
 *              delay = (l, or l - N from N/2 on) - early;  fine = 0.5 (a - c) / (a - 2 b + c) with a, b, c = pdp at l - 1, l,
 *              l + 1 (mod N), 0 when the denominator is 0;  power = b.
 *   Figures    over the reported paths in their order, float64, d_i = delay_i + fine_i:  path_power = sum p_i;  mean_delay =
 *              sum p_i d_i / sum p_i;  delay_spread = sqrt(sum p_i (d_i - mean_delay)^2 / sum p_i);  first_delay = the smallest
 *              delay_i;  outside_guard = the share of path_power on paths with delay_i - first_delay > CP (all 0 without a
 *              path).  total = sum_l pdp[l] in index order.  resp_mean (sum / K), resp_min, resp_max over the occupied bins in
 *              ascending bin order, resp_min_bin / resp_max_bin the first bin of each extreme.
 *              A zero input (peak = 0) gives zero everywhere, the two bins included, and no path.
 * delay = 0: a path whose phase reference symbol's useful part starts at sample null + CP of the frame.  A chain with FIRFilter
 *   reads -22 (its look-ahead, the 22 samples dabgpu_sync* and dabgpu_tii_scan* report as well); behind dabgpu_sync_extract* the
 *   strongest path reads 0.  A delay is unambiguous within +-N / 2.
 * Resolution: with the Hann weights two paths closer than about 3 N / K samples merge; with the rectangular ones every path
 *   shows its side lobes, from -13 dB down, as peaks of their own.  With one frame a noise tap exceeds min_ratio floor with
 *   probability about e^{-0.69 min_ratio} (|h|^2 of noise is exponentially distributed and the floor is its median): 1e-6 at
 *   min_ratio 20, per tap -- hence 20 as the wrappers' default, and more where one frame is all there is.
 * Every sum and search runs in a fixed order (the frames in order, total and the response's sum in index order, searches as an
 *   xor butterfly in the wave and the waves in wave order; ties go to the first index; no floating-point atomics): a call on
 *   the same samples gives the same bytes.
 * dabgpu_cir_dev: device pointer (aligned to a sample), asynchronous on `stream` (NULL: the context's own stream, behind every
 *   lane); two launches, no host round trip.  dabgpu_cir: the host-pointer form.
 * dabgpu_get_cir: waits for the most recent of them, as dabgpu_get_tii_scan does; the head, and min(cap, 16) path slots to
 *   `out`.  The result has a fixed layout, the same in every mode: the head (128 bytes), then 16 slots of 32 bytes, zeros behind
 *   n_paths: 640 bytes.  dabgpu_get_cir_profile: pdp and resp of the same call, N doubles each; either may be NULL.
 * Refused with DABGPU_E_INVALID and a message before anything is queued (the previous result stays): n_frames < 1 or >
 *   max_frames, early outside 0 ... CP, window other than 0 / 1, min_ratio not finite or < 1, min_rel outside [0, 1), a format
 *   other than 0 / DABGPU_FMT_S16, a null or misaligned pointer; a get before any call.
 * dabgpu_cir_check: host only, no context, no device: the refusals of mode (1..4; 0 = IV), n_frames (>= 1; max_frames is the
 *   context's) and the settings, message via dabgpu_last_error(NULL).
 * Out of scope: coherent averaging across frames, Doppler per path, a delay finer than the three-point `fine`, sampling-clock
 *   offset (since built: the clock), u8 / s8, resampled captures, and weighting the soft metrics with resp (this measures what that would need). */
#define DABGPU_CIR_MAX_PATHS 16
typedef struct dabgpu_cir_config { int early, window; float min_ratio, min_rel; } dabgpu_cir_config;
typedef struct dabgpu_cir_head {
    int n_frames, n_peaks, n_paths, window, peak_index, resp_min_bin, resp_max_bin, reserved;
    double floor, threshold, peak, total, path_power, mean_delay, delay_spread, first_delay, outside_guard, resp_mean, resp_min,
        resp_max;
} dabgpu_cir_head;                                                                                  /* 128 bytes */
typedef struct dabgpu_cir_path { int index, reserved; double delay, fine, power; } dabgpu_cir_path; /* 32 bytes */
DABGPU_API int dabgpu_cir_dev(dabgpu_ctx *ctx, const void *d_frames, int format, size_t n_frames, const dabgpu_cir_config *cfg,
                              void *stream);
DABGPU_API int dabgpu_cir(dabgpu_ctx *ctx, const void *frames, int format, size_t n_frames, const dabgpu_cir_config *cfg);
DABGPU_API int dabgpu_get_cir(dabgpu_ctx *ctx, dabgpu_cir_head *head, dabgpu_cir_path *out, size_t cap);
DABGPU_API int dabgpu_get_cir_profile(dabgpu_ctx *ctx, double *pdp, double *resp);
DABGPU_API int dabgpu_cir_check(int mode, size_t n_frames, const dabgpu_cir_config *cfg);

/* ---- the FIC reader: FIB CRCs, FIG 0/0, 0/1, 0/2, 1/0, 1/1, and a decoder that configures itself from them ------------------ *
 * dabgpu_decode* reads the tables dabgpu_frontend_configure uploads from a raw ETI frame's FC / STC words.  A capture that did
 * not come from this modulator has no ETI frame: its layout is written down in the Fast Information Channel only.  These
 * entries read it on the device and build the ETI header the decoder is configured with.  What the reference has of this is
 * on the CPU (FICDecoder, src/FigParser.cpp:94-321,650-713); nothing here replaces a plugin of its flowgraph.
 * Input: n_images images of 6144 bytes on the device, four-byte aligned: what dabgpu_decode* writes (the FIC at the configured
 *   layout's fic_offset, zeros in the headers), or raw ETI(NI) frames.  fic_offset says where the FIC lies in every image;
 *   DABGPU_FIC_OFFSET_CONFIGURED: at the configured layout's fic_offset.  The FIC is the 96 bytes (128 in Mode III) of the
 *   context's mode: 3 or 4 FIBs of 32 bytes per image.  FIB index = image x FIBs per image + i: stream order.
 * Per FIB, one dabgpu_fic_record (288 bytes):
 *   CRC      CRC-16, x^16 + x^12 + x^5 + 1, register 0xFFFF at the start, result complemented, over bytes 0 ... 29, compared big
 *            endian with bytes 30 ... 31 (EN 300 401 5.2.1; "123456789" gives 0xD64E).  flags: DABGPU_FIC_CRC_OK.  A FIB of 32
 *            zero bytes fails it (30 zero bytes give 0xD5BA) and is flagged DABGPU_FIC_ZERO: what the decoder's fifteen
 *            lead-in outputs hold, counted as fibs_zero, not as fibs_bad.  A FIB that fails carries nothing but its flags.
 *   Walk     only when the CRC holds, over bytes 0 ... 29, to the end marker 0xFF: type (3 bits) | length (5 bits), then
 *            `length` bytes.  A FIG whose length runs past byte 29 ends the walk: figs_truncated, DABGPU_FIC_TRUNCATED, the FIG
 *            is not counted.  An entry cut off by the end of its FIG is dropped with what follows it in that FIG.  No byte
 *            outside the FIB's 32 is ever read.  (FICDecoder trusts the lengths and reads on: the deliberate deviation.)
 *            figs_type[t]: FIGs of type t;  fig0_ext[e]: FIGs 0/e (length >= 1), whatever their flags.
 *   FIG 0    header C/N | OE | P/D | extension (5 bits).  Extensions 0, 1, 2 are read only with C/N = OE = P/D = 0, as the
 *            reference does (fig0_skipped counts those that were not); every other extension is counted only.
 *   FIG 0/0  (>= 4 field bytes) EId, change flags (2 bits), alarm flag, CIF count (5 + 8 bits).  eid_first / eid: the first and
 *            the last EId of the FIB, eid_seen how many, eid_changes how often one differed from the one before.
 *   FIG 0/1  per entry SubChId (6 bits), start address (10 bits), then the short form (0, table switch, 6-bit table index: 3
 *            bytes) or the long form (1, option (3 bits), protection level (2 bits), size (10 bits): 4 bytes).  sub[]: raw = the
 *            entry's 3 or 4 bytes, first byte highest, zero behind a short entry;  form;  sw_option = table switch or option;
 *            index_level = table index or the level field (0 ... 3);  size (0 in the short form).  At most 9 per FIB.
 *   FIG 0/2  (P/D = 0) SId (16 bits), info = local flag | CAId (3 bits) | number of components (4 bits), then per component two
 *            bytes: TMId (2 bits); ASCTy / DSCTy (6 bits; `type`, 0 for TMId 3); SubChId (6 bits) or, for TMId 3, SCId (12 bits)
 *            (`id`); P/S (`primary`); CA flag.  4 services and 8 components are kept per FIB, a service with all of its
 *            components or not at all: services_dropped, components_dropped.
 *   FIG 1    header charset (4 bits) | OE | extension (3 bits).  1/0 (kind 1, id = EId) and 1/1 (kind 2, id = SId) with OE = 0
 *            and exactly 2 + 16 + 2 field bytes: 16 label bytes and the 16-bit character flag.  The first label of a FIB is
 *            kept, later ones are counted (labels_dropped).
 * Over the call, dabgpu_fic_result: the sums of the above (fibs = fibs_ok + fibs_bad + fibs_zero), and per SubChId 0 ... 63 and
 *   for the EId what one pass over the FIBs in stream order, entries in walk order, gives: seen = sightings, changes = how often
 *   the raw word differed from the sighting before, first_fib / last_fib, raw = the last word.  Formed without atomics in a fixed
 *   order, from per-run summaries whose combination is associative: the same bytes for the same input, whatever the grid.
 *   sub[0 ... n_subch - 1]: the SubChIds seen, ascending; the rest is zero.  Derived on the host from the last raw word:
 *   short form: table_switch = 0 is supported: index_option = the table index, row i of the standard's 64-row table (EN 300 401
 *     table 6: ascending bit rate, level 5 down to 1) built from the UEP profiles of host/protection_tables.inc -> bitrate,
 *     level 1 ... 5, size_cu;  tpl = level - 1.
 *   long form: index_option = option, level = the level field + 1.  Option 0 (EEP-A): bitrate = size / {12, 8, 6, 4}[level - 1]
 *     x 8;  option 1 (EEP-B): bitrate = size / {27, 21, 18, 15}[level - 1] x 32;  supported when the option is 0 or 1 and the
 *     size a non-zero multiple of its factor;  tpl = 0x20 | option << 2 | (level - 1);  size_cu = size.
 *   stl = 3 x bitrate / 8 (64-bit words per 24 ms).  supported = 0: bitrate, level (short form), tpl, stl are 0.
 * dabgpu_fic_scan_dev: asynchronous on `stream` (NULL: the context's own, behind every lane); three launches, no host round
 *   trip.  dabgpu_fic_scan: the host-pointer form.  A result is per call; the getters wait for the most recent one.
 *   Refused with DABGPU_E_INVALID and a message before anything is queued (the previous result stays): n_images = 0 or above
 *   2^22; a null or misaligned pointer; an offset that is not a multiple of 4 or with fic_offset + fic_bytes > 6144;
 *   DABGPU_FIC_OFFSET_CONFIGURED on a context whose front-end is not configured; a get before any call.
 * dabgpu_get_fic_records: min(cap, n) records to `out`, *n = FIBs of the call.  dabgpu_get_fic_services: merged on the host
 *   from the records (a few hundred bytes per call's worth of 16-bit identifiers): services in order of first appearance (in
 *   a FIG 0/2, or as the id of a FIG 1/1; within one FIB the FIG 0/2 entries come first), sightings = FIG 0/2 entries, the
 *   components in order of first appearance ((TMId, id) names one; the latest type / primary / ca), at most
 *   DABGPU_FIC_MAX_COMPONENTS, the latest label.  min(cap, n) services to `out`, *n = services found; `ensemble` (may be NULL):
 *   the latest FIG 1/0, kind 0 when none was seen.
 * Host only -- no context, no device, message via dabgpu_last_error(NULL):
 *   dabgpu_fic_bootstrap_frame: the ETI header of an ensemble with FICF = 1 and NST = 0 in `mode` (1 ... 4).
 *     dabgpu_frontend_configure on it leaves a decoder that decodes the FIC alone: the FIC's puncturing depends on the mode only.
 *   dabgpu_fic_make_header: from a result, the ETI frame dabgpu_frontend_configure wants: SYNC, FC (FCT 0, FICF 1, NST, FP 0, MID,
 *     FL), one STC word per sub-channel in ascending SubChId (SCId = SubChId, SAD, TPL, STL), EOH zero, zero payload, EOF 00 00 FF
 *     FF, TIST FF FF FF FF, 0x55 behind it.  Refused: n_subch = 0 (no FIG 0/1 seen is not an empty ensemble); n_subch above 64; a
 *     sub-channel with changes > 0 (a reconfiguration inside the capture); a sub-channel with supported = 0.  Then whatever
 *     dabgpu_frontend_describe and dabgpu_decode_check_layout refuse (overlap, beyond CU 864), with their message.
 * dabgpu_decode_configure_from_fic: dabgpu_fic_make_header on the most recent result in the context's mode, then
 *   dabgpu_frontend_configure -- which zeroes the histories of front-end and decoder.
 * The blind loop: coded bits of a capture -> a context configured with dabgpu_fic_bootstrap_frame -> dabgpu_decode_dev ->
 *   dabgpu_fic_scan_dev on its output (past the fifteen lead-in images, or with them: they count as fibs_zero) ->
 *   dabgpu_decode_configure_from_fic -> dabgpu_decode_dev on the same coded bits again.  The FIC leaves the decoder fifteen ETI
 *   frames late, like every unit: A CAPTURE MUST HOLD MORE THAN 15 ETI FRAMES BEFORE ANYTHING CAN BE READ.  A FIC path
 *   without the delay line is out of scope; so are the other FIG 0 extensions, FIG 1/4 ... and FIG 2, and CRC-less recovery. */
#define DABGPU_FIC_OFFSET_CONFIGURED (~(size_t)0)
#define DABGPU_FIC_CRC_OK 1u
#define DABGPU_FIC_ZERO 2u
#define DABGPU_FIC_TRUNCATED 4u
#define DABGPU_FIC_REC_SUBCH 9
#define DABGPU_FIC_REC_SERVICES 4
#define DABGPU_FIC_REC_COMPONENTS 8
#define DABGPU_FIC_MAX_COMPONENTS 12
typedef struct dabgpu_fic_sub_entry {
    uint32_t raw;
    uint16_t sad, size;
    uint8_t subchid, form, sw_option, index_level;
} dabgpu_fic_sub_entry;                                                                              /* 12 bytes */
typedef struct dabgpu_fic_service_entry { uint16_t sid; uint8_t info, first_comp; } dabgpu_fic_service_entry;
typedef struct dabgpu_fic_component { uint16_t id; uint8_t tmid, type, primary, ca, service, reserved; } dabgpu_fic_component;
typedef struct dabgpu_fic_label { uint8_t kind, charset; uint16_t id, flag; uint8_t text[16]; uint16_t reserved; } dabgpu_fic_label;
typedef struct dabgpu_fic_record {
    uint32_t flags;
    uint16_t eid_first, eid;
    uint8_t eid_seen, eid_changes, change, alarm;
    uint8_t cif_hi, cif_lo, n_sub, n_svc;
    uint8_t n_comp, services_dropped, components_dropped, labels_dropped;
    uint8_t figs_truncated, fig0_skipped, reserved[2];
    uint8_t figs_type[8];
    uint8_t fig0_ext[32];
    dabgpu_fic_sub_entry sub[DABGPU_FIC_REC_SUBCH];
    dabgpu_fic_service_entry svc[DABGPU_FIC_REC_SERVICES];
    dabgpu_fic_component comp[DABGPU_FIC_REC_COMPONENTS]; /* `service`: index into svc[] */
    dabgpu_fic_label label;
    uint8_t pad[12];
} dabgpu_fic_record;                                                                                 /* 288 bytes */
typedef struct dabgpu_fic_subch {
    uint32_t subchid, sad, size_cu, form, index_option, level, bitrate, tpl, stl, supported, seen, changes, first_fib, last_fib, raw;
    uint32_t table_switch;
} dabgpu_fic_subch;                                                                                  /* 64 bytes */
typedef struct dabgpu_fic_result {
    uint32_t fibs, fibs_ok, fibs_bad, fibs_zero, figs_truncated, fig0_skipped, services_dropped, components_dropped, labels_dropped;
    uint32_t eid, eid_seen, eid_changes, eid_first_fib, eid_last_fib, n_subch, reserved;
    uint32_t figs_type[8], fig0_ext[32];
    dabgpu_fic_subch sub[64];
} dabgpu_fic_result;                                                                                 /* 4320 bytes */
typedef struct dabgpu_fic_service {
    uint32_t sid, n_components, sightings, components_dropped;
    dabgpu_fic_component comp[DABGPU_FIC_MAX_COMPONENTS]; /* `service` is 0 here */
    dabgpu_fic_label label;                               /* kind 0: no FIG 1/1 seen */
} dabgpu_fic_service;                                                                                /* 136 bytes */
DABGPU_API int dabgpu_fic_scan_dev(dabgpu_ctx *ctx, const void *d_images, size_t n_images, size_t fic_offset, void *stream);
DABGPU_API int dabgpu_fic_scan(dabgpu_ctx *ctx, const uint8_t *images, size_t n_images, size_t fic_offset);
DABGPU_API int dabgpu_get_fic_result(dabgpu_ctx *ctx, dabgpu_fic_result *out);
DABGPU_API int dabgpu_get_fic_records(dabgpu_ctx *ctx, dabgpu_fic_record *out, size_t cap, size_t *n);
DABGPU_API int dabgpu_get_fic_services(dabgpu_ctx *ctx, dabgpu_fic_service *out, size_t cap, size_t *n, dabgpu_fic_label *ensemble);
DABGPU_API int dabgpu_fic_bootstrap_frame(int mode, uint8_t frame[6144]);
DABGPU_API int dabgpu_fic_make_header(const dabgpu_fic_result *result, int mode, uint8_t frame[6144]);
DABGPU_API int dabgpu_decode_configure_from_fic(dabgpu_ctx *ctx);

/* ---- the superframe reader: DAB+ Fire code, RS(120,110) and AU CRCs of one sub-channel ------------------------------------- *
 * What a receiver judges a DAB+ sub-channel by (ETSI TS 102 563 5.2-5.4, 6): whether the superframes are found, how many bytes the
 * outer code had to correct and how many words it could not, and whether the access units pass their CRC.  These figures need no
 * reference ETI: they are the ground truth a capture carries itself.  The reference sends superframes and reads none; the outer
 * code is checked against its lib/fec (decode_rs_char), set up as init_rs_char(8, 0x11d, 0, 1, 10, 135).
 * Input: n_images images of 6144 bytes on the device, four-byte aligned: what dabgpu_decode* writes, or raw ETI(NI) frames; one
 *   sub-channel as (offset, framesize), the fields dabgpu_frontend_describe gives.  framesize = 24 s, s = bitrate / 8 in 1 ... 24.
 * Candidate f (0 ... n_images - 5): the 120 s bytes of the sub-channel in images f ... f + 4.  EVERY alignment is decoded, n_images - 4
 *   candidates per call: nothing depends on an earlier candidate and the device never waits for a host decision.  The fivefold
 *   work is deliberate (profiles/superframe.txt has its cost).
 * Per candidate, one dabgpu_sf_record (64 bytes):
 *   RS       codeword i (i < s) is bytes i, i + s, ..., i + 119 s: 110 data bytes, 10 parity bytes.  GF(2^8) with x^8 + x^4 + x^3 +
 *            x^2 + 1, g(x) = prod_{i = 0 ... 9} (x + alpha^i), shortened from (255,245).  Syndromes, Berlekamp-Massey, a Chien search
 *            over the 120 real positions, Forney.  cw_errors[i]: bytes corrected in word i; DABGPU_SF_WORD_FAILED for a word that
 *            is uncorrectable -- the locator has fewer roots among the 120 real positions than its degree, which covers a degree
 *            above 5 and a root in the 135 padding positions -- and whose bytes stay as received; 0 behind s.  (lib/fec applies
 *            the in-range part of a locator with a root in the padding and reports success: the deliberate deviation.)
 *            rs_corrected: bytes over the candidate; rs_failed: words; rs_max: the most corrections in one word;
 *            DABGPU_SF_RS_FAILED: rs_failed > 0.  No erasure decoding.
 *   Fire     on the corrected bytes: CRC-16 with x^16 + x^14 + x^13 + x^12 + x^11 + x^5 + x^3 + x^2 + x + 1 (0x782F), register 0 at the
 *            start, not complemented, over bytes 2 ... 10 (fire_crc), compared big endian with bytes 0 ... 1: DABGPU_SF_FIRE_OK.
 *            Eleven zero bytes pass it -- and are what the decoder's fifteen lead-in images hold: DABGPU_SF_ZERO, never accepted.
 *   Header   byte 2 (`header`): rfa | dac_rate | sbr_flag | aac_channel_mode | ps_flag | mpeg_surround_config (3 bits).
 *            (dac_rate, sbr_flag) -> (num_aus, au_start[0]): (0,1) -> (2, 5); (1,1) -> (3, 6); (0,0) -> (4, 8); (1,0) -> (6, 11).
 *            au_start[1 ... num_aus - 1]: 12-bit big-endian fields packed from byte 3; au_start[num_aus] = 110 s; 0 behind it.
 *            DABGPU_SF_HEADER_VALID: every AU is at least 3 bytes long (so the starts ascend and the last lies below 110 s).
 *            The fields are written whatever the Fire code says.
 *   AU CRC   the FIB's CRC (0x1021, register 0xFFFF, complemented) over an AU without its last two bytes, compared big endian with
 *            them; au_ok: bit k = AU k passes.  Computed only for an ACCEPTED candidate: FIRE_OK, not ZERO, HEADER_VALID.
 * Output bytes: candidate f at f x 110 s of d_out: its data bytes after correction, in superframe order (uncorrectable words
 *   contribute their received bytes).  *out_bytes = (n_images - 4) x 110 s.
 * Over the call, dabgpu_sf_result: formed on the host by the getter from the records.  Walk f from 0; an accepted candidate
 *   counts and f += 5, any other f += 1.  Stateless: no lock, no hysteresis.  candidates; superframes; first: the first
 *   accepted candidate, -1 if none; phase_changes: accepted candidates whose f mod 5 differs from the one before; over the
 *   accepted candidates aus, aus_ok, aus_bad, rs_corrected, rs_failed, rs_max; `accepted` receives min(cap, superframes) of
 *   their indices (may be NULL with cap 0).
 * THERE IS NO STREAM STATE.  A superframe that straddles two calls is the caller's business: hand the last four images of one
 *   call in again in front of the next (the decoder keeps its history of fifteen rows itself; this stage keeps nothing).
 * dabgpu_superframe_dev: asynchronous on `stream` (NULL: the context's own, behind every lane); one launch, one workgroup per
 *   candidate, no atomics: the same records and bytes for the same images, whatever the split into calls.  dabgpu_superframe:
 *   the host-pointer form.  A result is per call; the getters wait for the most recent one.
 *   Refused before anything is queued (the previous result stays), DABGPU_E_INVALID and a message: n_images below 5 or above 2^22;
 *   a null or misaligned pointer; a framesize that is not 24 s with s in 1 ... 24; an offset that is not a multiple of 4 or with
 *   offset + framesize > 6144; a get before any call.  DABGPU_E_CAPACITY: out_cap too small (*out_bytes receives the size).
 * dabgpu_get_superframe_records: min(cap, n) records to `out`, *n = candidates of the call.
 * dabgpu_superframe_check: the shape refusals alone -- host only, no context, message via dabgpu_last_error(NULL).
 * Out of scope: erasure decoding from the soft metrics; AAC, PAD; DAB (MP2) frames; packet mode. */
#define DABGPU_SF_FIRE_OK 1u
#define DABGPU_SF_ZERO 2u
#define DABGPU_SF_HEADER_VALID 4u
#define DABGPU_SF_RS_FAILED 8u
#define DABGPU_SF_WORD_FAILED 0xFFu
#define DABGPU_SF_MAX_WORDS 24
typedef struct dabgpu_sf_record {
    uint32_t flags;
    uint16_t rs_corrected, rs_failed;
    uint8_t rs_max, num_aus, au_ok, header;
    uint8_t rfa, dac_rate, sbr_flag, aac_channel_mode, ps_flag, mpeg_surround_config, reserved0[2];
    uint16_t au_start[7];
    uint16_t fire_crc;
    uint8_t cw_errors[DABGPU_SF_MAX_WORDS];
    uint32_t reserved1;
} dabgpu_sf_record;                                                                                  /* 64 bytes */
typedef struct dabgpu_sf_result {
    uint32_t candidates, superframes;
    int32_t first;
    uint32_t phase_changes, aus, aus_ok, aus_bad, rs_failed, rs_max, reserved;
    uint64_t rs_corrected;
} dabgpu_sf_result;                                                                                  /* 48 bytes */
DABGPU_API int dabgpu_superframe_dev(dabgpu_ctx *ctx, const void *d_images, size_t n_images, size_t offset, size_t framesize,
                                     void *d_out, size_t out_cap, size_t *out_bytes, void *stream);
DABGPU_API int dabgpu_superframe(dabgpu_ctx *ctx, const uint8_t *images, size_t n_images, size_t offset, size_t framesize,
                                 uint8_t *out, size_t out_cap, size_t *out_bytes);
DABGPU_API int dabgpu_get_superframe_result(dabgpu_ctx *ctx, dabgpu_sf_result *out, uint32_t *accepted, size_t cap);
DABGPU_API int dabgpu_get_superframe_records(dabgpu_ctx *ctx, dabgpu_sf_record *out, size_t cap, size_t *n);
DABGPU_API int dabgpu_superframe_check(size_t n_images, size_t offset, size_t framesize);

/* wait for everything queued on the context's own stream(s): every lane */
DABGPU_API int dabgpu_synchronize(dabgpu_ctx *ctx);

#ifdef __cplusplus
}
#endif
#endif
