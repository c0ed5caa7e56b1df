// dabgpu_ctx.h -- the device context behind the C-ABI of include/dabgpu.h and the helpers its translation units share:
//   api_context.hip   context, settings, device tables (apply_settings), setters, diagnostics
//   api_chain.hip     the chain dispatch: which kernels a stage mask runs and which scratch they take, decided once per call
//                     (plan_chain -> ChainPlan) and carried out (run_native / run_chain), chain entry points
//   api_lanes.hip     batches in flight inside one context: lanes (chosen from the plan's scratch total), their ordering,
//                     submit / collect
//   api_stages.hip    one host-buffer entry point per reference plugin, FormatConverter, CFR statistics
//   api_state.hip     the stream state (resampler halo, TII frame parity): read, installed, computed from a lead-in frame
//                     of coded bits or, with the front-end's, from the ETI frames in front of a chunk
//   api_demod.hip     the receiver (demod.hip): IQ -> coded bits and per-frame quality figures, stand-alone and as the monitor
//                     that rides on a chain call
//   api_spectrum.hip  the spectrum monitor (spectrum.hip): Welch power spectrum of any sample buffer, stand-alone and behind a
//                     chain call; the window tables and the mask check (host only)
//   api_dpd.hip       the DPD measurement (dpd.hip): cross-spectrum and aligned amplitude-bin statistics of a tx / feedback
//                     pair; alignment solve, delay taps and polynomial fit (host only)
//   api_decode.hip    the channel decoder (decode.hip): coded bits -> ETI payload, its history of fifteen received rows, the
//                     per-unit figures; the layout check (host only)
//   api_sync.hip      the synchroniser (sync.hip): frame starts and carrier offset of a capture, the frames extracted for the
//                     receiver; the shape check (host only)
//   api_channel.hip   the channel emulator (channel.hip): paths, Doppler and seeded noise on a sample stream, its history and
//                     position; the settings check (host only)
//   api_clock.hip     the clock's resampler (clock.hip): a sampling-clock offset put on a sample stream or taken off it, its
//                     history and position; step, counts and the tap table (host only); the clock's estimator: the offset
//                     of whole frames from their data symbols
//   api_tuner.hip     the tuner (tuner.hip): mixer, channel filter and decimator from any accepted capture rate and offset to
//                     the native rate, its history and position; ratio, tap rows and counts (host only)
//   api_tii_scan.hip  the TII analyser (tii_scan.hip): transmitters, levels and delays from the null symbols of whole frames;
//                     the settings check (host only)
//   api_cir.hip       the channel estimator (cir.hip): impulse response, echoes and the response on the carriers from the
//                     phase reference symbols of whole frames; the settings check (host only)
//   api_fic.hip       the FIC reader (fic.hip): FIB CRCs and FIG 0/0, 0/1, 0/2, 1/0, 1/1 of decoded images or ETI frames, the
//                     sub-channel table of a call; the short-form table, the derived fields, the ETI header made from a
//                     result and the bootstrap frame (host only); the decoder configured from a result
//   api_superframe.hip the superframe reader (superframe.hip): Fire code, RS(120,110) and AU CRCs of one DAB+ sub-channel of
//                     decoded images or ETI frames, a record per alignment of five images; the greedy walk over a call's
//                     records and the shape check (host only)
//   api_frontend.hip  the front-end on the device: layout of an ETI frame (host), configure / reset, ETI -> coded bits -> IQ,
//                     its own stream state (the time interleaver's history): read, installed, computed from lead-in frames
// In this order: Settings, TraceScope; the receive-side stages' state, one struct each (the streamed stages' on StreamStage);
// dabgpu_ctx with one member of each beside the chain's own; what the translation units export to each other; what entry
// points are built from (HostIO ... capture_from_host for the capture stages, StreamRules ... stream_run_samples for the
// streamed ones).  Device memory is DevBuf's (devbuf.h): a context's buffers free themselves when it is deleted.
#pragma once
#include "dabgpu.h"
#include "dabgpu_internal.h"
#include "devbuf.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <tuple>
#include <vector>

namespace dabgpu_api {
using namespace dabgpu;

struct Settings {
    int gain_mode = DABGPU_GAIN_VAR;      // src/ConfigParser.h:60-91 defaults
    float digital = 1.0f, normalise = 1.0f, var_variance = 4.0f;
    bool gain_reference_rounding = false;  // dabgpu_set_gain_rounding: chain calls replay the reference's variance recurrence
    std::vector<float> taps;
    size_t overlap = 0;
    size_t rs_in = 2048000, rs_out = 2048000;
    bool poly_is_lut = false;
    float am[5] = {1, 0, 0, 0, 0}, pm[5] = {0, 0, 0, 0, 0};
    float lut_scale = 0.f, lut[32] = {0};
    bool cfr_enable = false;               // src/ConfigParser.h: enableCfr / cfrClip / cfrErrorClip
    float cfr_clip = 1.0f, cfr_errclip = 1.0f;
    int out_format = 0;                    // 0 = complexf, else DABGPU_FMT_*: FormatConverter as the chain's last step
    bool tii_enable = false, tii_old_variant = false;   // src/TII.h:42-69 (tii_config_t)
    int tii_comb = 0, tii_pattern = 0;
    size_t cic_spacing = 0;                // dabgpu_set_cic_equalizer: CicEqualizer(carriers, spacing, R) between cifSig and
    int cic_R = 0;                         // cifOfdm of every chain call (src/DabModulator.cpp:155-176,399); 0 / 0 = off
    bool monitor = false;                  // dabgpu_set_monitor: every native-rate chain call is demodulated against its own bits
    int monitor_early = -1;                //   the FFT window's lead in samples; < 0: from the call's filter and window
    bool spectrum = false;                 // dabgpu_set_spectrum_monitor: every chain call's output goes into the Welch sums
    int spectrum_window = 2;               //   the window table (dabgpu_spectrum_window)
    unsigned long long epoch = 1;  // bumped by every setter
    bool resampler_reset = true;

    // What each group of device data is a function of.  apply_settings_groups compares these keys, never single fields: a
    // setting that starts to feed a table is added to that table's key HERE, next to its declaration.
    //   the fused FIR's tap table, its frequency response and the inverse filter of the equalised-boundary variant
    auto fir_key() const { return std::tie(taps); }
    //   the raised-cosine window of the guard interval
    auto window_key() const { return std::tie(overlap); }
    //   the predistorter's coefficient block (polynomial and LUT share it; the selector and the LUT scale are kernel arguments)
    bool coef_equal(const Settings &o) const
    {
        return poly_is_lut == o.poly_is_lut && lut_scale == o.lut_scale && !std::memcmp(am, o.am, sizeof am) &&
               !std::memcmp(pm, o.pm, sizeof pm) && !std::memcmp(lut, o.lut, sizeof lut);
    }
    //   the chain's table of CicEqualizer factors
    auto cic_key() const { return std::tie(cic_spacing, cic_R); }
    bool cic_on() const { return cic_spacing != 0 && cic_R > 0; }
    //   the resampler's window, twiddles and geometry
    auto resampler_key() const { return std::tie(rs_in, rs_out); }
    //   the cached unit-gain TII segment (TII symbol -> IFFT -> [CFR] -> guard [window] -> [FIR]); gain scales it at use
    auto tii_segment_key() const
    {
        return std::tie(taps, overlap, tii_comb, tii_pattern, tii_old_variant, cfr_enable, cfr_clip, cfr_errclip);
    }
};


// names the kernels of one chain call into ctx->last_variant (the sink is a thread-local of api_context.hip)
std::string *&trace_sink_ref();
struct TraceScope {
    std::string *prev;
    // (sink == nullptr: tracing is off for this context -- nothing is installed, a launch costs one pointer test)
    explicit TraceScope(std::string *sink) : prev(trace_sink_ref())
    {
        if (sink) sink->clear();
        trace_sink_ref() = sink;
    }
    ~TraceScope() { trace_sink_ref() = prev; }
};

// ---- the state of the receive-side stages: one struct each, one member each in dabgpu_ctx.  `stream` is the stream the
// most recent result is complete on (nullptr: none yet -- wait_result).  Every DevBuf frees itself with the context.

// The receiver (api_demod.hip): the records of the most recent dabgpu_demod* call or monitored chain call and the staging
// of the host-pointer entries (the capture itself is staged in the chain's d_out).  Monitored calls stay on lane 0: one set.
struct DemodState {
    DevBuf stats, bits, ref, soft;
    size_t frames = 0;
    bool has_ref = false;
    hipStream_t stream = nullptr;
    int run_symbols = 0;                  // dabgpu_debug_demod_run_symbols: symbols per workgroup, 0 = by the batch size
};

// The carrier state (api_demod.hip, dabgpu_demod_csi* / dabgpu_demod_carrier_state*): the integer sums and the weights of
// the most recent such call, sized by the largest call.
struct CsiState {
    DevBuf sums, weights;
    size_t frames = 0;
    hipStream_t stream = nullptr;
    bool unit_weights = false;            // dabgpu_debug_csi_unit_weights
};

// The spectrum monitor (api_spectrum.hip): the three window tables, the rows of one launch, the sums (2048 float64 and the
// segment count) and the host-pointer entry's staging.  One accumulator: monitored calls stay on lane 0.  window: the window
// the sums were formed with, -1 = none yet.
struct SpectrumState {
    DevBuf win, rows, acc, in;
    bool ready = false;
    int window = -1;
    double rate_hz = 0.0;
    hipStream_t stream = nullptr;
    int run_segments = 0;                 // dabgpu_debug_spectrum_run_segments: segments per workgroup, 0 = by the input size
};

// The DPD measurement (api_dpd.hip): the cross-spectrum's rows and sums (4 x 2048 float64 and the segment count), the
// statistics' integer sums (256 bins x 6 figures, overflow, samples used), the squared bin edges and the host-pointer entries'
// staging.  peak / bins: what the sums were formed with (0: none yet); offered: samples offered since they started over (the
// cap).
struct DpdState {
    DevBuf rows, xacc, sums, edge, tx, rx;
    bool ready = false;
    float peak = 0.f;
    int bins = 0;
    unsigned long long offered = 0;
    hipStream_t stream = nullptr;
    int run_segments = 0;                 // dabgpu_debug_dpd_run_segments
    int tile = 0;                         // dabgpu_debug_dpd_tile
};

// The channel decoder (api_decode.hip, decode.hip).  One DecodeStream per metric width: the hard decoder's rows hold one byte
// per received bit, the soft decoder's eight int8 metrics.  rows is the stream state: [15 + n][width x (fic_out + 6912)]
// received rows, punctured FIC | CIF of one ETI frame each, rows 0 ... 14 = the last fifteen of the stream (zero after
// configure / reset: zero_pending asks the next call to zero them).  pos: rows received since then (outputs before row 15
// are the lead-in).  tmp: where the last fifteen rows pass through when they overlap their place at the front.  stats,
// frames, first_valid, stream: the records of the most recent call; in: the host-pointer entry's staging.
struct DecodeStream {
    size_t width;                         // bytes per received bit: 1 (coded bits) or 8 (soft metrics)
    DevBuf rows, tmp, stats, in;
    unsigned long long pos = 0;
    bool zero_pending = true;
    size_t frames = 0, first_valid = 0;
    hipStream_t stream = nullptr;
};
// What both streams share (both stay on lane 0): slot -- where each unit's survivor words start inside one output's share
// of surv -- with its device copy, the survivor scratch, and the host-pointer entries' output and reference staging.
struct DecodeState {
    DecodeStream hard{1}, soft{8};
    DevBuf slot_dev, surv, out, ref;
    std::vector<uint32_t> slot;
    std::string refusal;                  // not empty: the configured layout is not decoded (two sub-channels on one capacity unit)
};

// The synchroniser (api_sync.hip, sync.hip): head and frame records of the most recent dabgpu_sync* call (what
// dabgpu_sync_extract* reads, straight from device memory), the block powers, what the call was given (n = 0 samples: none
// yet) and the host-pointer entries' staging.
struct SyncState {
    DevBuf result, power, in, out;
    size_t n = 0, slots = 0;
    hipStream_t stream = nullptr;
};

// What the streamed stages share (channel emulator, clock's resampler, tuner): a call takes the next n samples of a stream and
// reads a few samples of history in front of them.  hist: two histories of float samples, the stream state (kChMaxDelay,
// kClkHist, kTunMaxHist samples each); hist_cur: the one the next call reads (a call writes the other and swaps).
// zero_pending: the next call zeroes it first (before the first call, after the stage's setter -- the channel's keeps the
// stream -- and after its reset).  position: input samples the stream has taken (the reset's position included).  in, out:
// the host-pointer entry's staging.  run_samples: dabgpu_debug_*_run_samples, samples or outputs per workgroup, 0 = chosen.
struct StreamStage {
    DevBuf hist, in, out;
    bool configured = false, zero_pending = true;
    int hist_cur = 0;
    unsigned long long position = 0;
    hipStream_t stream = nullptr;
    int run_samples = 0;
};

// The channel emulator (api_channel.hip, channel.hip).  args: the installed configuration as the kernel takes it (paths that
// do not rotate first, either group in the given order).
struct ChannelState : StreamStage {
    dabgpu::ChannelArgs args{};
};

// The clock's resampler (api_clock.hip, clock.hip).  step: the installed offset as the kernel takes it.  tab: the tap table,
// uploaded by the first dabgpu_set_clock.
struct ClockState : StreamStage {
    DevBuf tab;
    long long step = 0;
};

// The clock's estimator (api_clock.hip, clock.hip).  rows: every block's sums (scratch); sums: the frames' sums of the most
// recent dabgpu_sco* call, `frames` of them (0: no call yet); in: the host-pointer entry's staging.
struct ScoState {
    DevBuf rows, sums, in;
    size_t frames = 0;
    hipStream_t stream = nullptr;
};

// The tuner (api_tuner.hip, tuner.hip).  Of a history's kTunMaxHist samples the first P - 1 are in use.  cfg, L, M, P, step: the
// installed setting and what follows from it.  tab: the tap table [L][P] of (tab_rate, tab_selectivity), uploaded by the
// dabgpu_set_tuner that changes either.
struct TunerState : StreamStage {
    DevBuf tab;
    unsigned long long step = 0;
    dabgpu_tuner_config cfg{};
    int L = 1, M = 1, P = 32;
    uint32_t tab_rate = 0;
    int tab_selectivity = -1;
};

// The TII analyser (api_tii_scan.hip, tii_scan.hip).  result: head, 24 entry slots and the entries' grid centres of the most
// recent dabgpu_tii_scan* call; rows / bins: per-frame cell sums and occupied bins (scratch); in: the host-pointer entry's
// staging; done: a call has been queued.
struct TiiScanState {
    DevBuf result, rows, bins, in;
    bool done = false;
    hipStream_t stream = nullptr;
};

// The channel estimator (api_cir.hip, cir.hip).  result: head, 16 path slots, then the profile and the response (N doubles
// each) of the most recent dabgpu_cir* call; rows: per-frame taps and bins (scratch, max_frames of them); in: the
// host-pointer entry's staging; done: a call has been queued.
struct CirState {
    DevBuf result, rows, in;
    bool done = false;
    hipStream_t stream = nullptr;
};

// The FIC reader (api_fic.hip, fic.hip).  rec: one record per FIB of the most recent dabgpu_fic_scan* call, `fibs` of them;
// partial: one summary per 256 FIBs (scratch); result: the call's summary; in: the host-pointer entry's staging; done: a call
// has been queued.
struct FicState {
    DevBuf rec, partial, result, in;
    size_t fibs = 0;
    bool done = false;
    hipStream_t stream = nullptr;
};

// The superframe reader (api_superframe.hip, superframe.hip).  rec: one record per candidate of the most recent
// dabgpu_superframe* call, `candidates` of them; in, out: the host-pointer entry's staging; done: a call has been queued.
// No stream state: a candidate is five images of the call.
struct SuperframeState {
    DevBuf rec, in, out;
    size_t candidates = 0;
    bool done = false;
    hipStream_t stream = nullptr;
};
}  // namespace dabgpu_api

struct dabgpu_ctx {
    std::string last_variant;             // dabgpu_debug_last_variant: the kernels the most recent chain call launched
    bool trace_enabled = false;           // dabgpu_debug_trace: off by default (names are formatted per launch when on)
    dabgpu::Geometry g{};
    int device = 0;
    int max_frames = 1;
    int chunks_cfg = 0;
    hipStream_t stream = nullptr;
    std::string err;

    // constant tables
    dabgpu_api::DevBuf d_twiddle, d_src, d_dst, d_phq, d_mag, d_taps, d_firh, d_window, d_coef, d_eqg;
    bool use_eq = true;                   // dabgpu_set_fir_boundary_mode: false = always the packed dual transform
    bool eq_ok = false;                   // d_eqg holds a well-conditioned inverse of the current taps (TF_EQ may be used)
    double eq_fit = 0.0;                  // max |G H - 1| over the occupied bins
    // resampler
    dabgpu_api::DevBuf d_rs_window, d_rs_tw_in, d_rs_tw_out, d_rs_halo, d_rs_tw_s, d_rs_tw_l;
    int rs_nin = 0, rs_nout = 0;
    int rs_halo_cur = 0;                  // which of the two halo buffers holds the state the next call reads
    size_t rs_L = 1, rs_M = 1;
    float rs_factor = 1.f;
    int rs_last_hops = 0;                 // dabgpu_debug_resampler_last_launch: the most recent resampler launch of this context
    unsigned rs_last_grid = 0;
    int rs_run_hops = 0;                  // dabgpu_debug_resampler_run_hops: hops per workgroup, 0 = by the call size
    // scratch
    dabgpu_api::DevBuf d_a, d_b, d_c, d_in, d_out, d_count, d_fmt, d_clip;
    dabgpu_api::DevBuf d_car;             // CIC equaliser on: the carriers between the front kernel and the from-carriers chain
    // dabgpu_chain_seed: the lead-in frame's coded bits, through two pinned staging frames in turn (the host never waits
    // for the seed before the last one)
    dabgpu_api::DevBuf d_seed;
    void *h_seed[2] = {nullptr, nullptr};
    hipEvent_t seed_ev[2] = {nullptr, nullptr};
    unsigned long long seed_seq = 0;
    // The front-end on the device (api_frontend.hip, frontend.hip).  d_fe_hist is the stream state: [15 + n_eti][6912] punctured,
    // not yet time-interleaved CIF rows, rows 0 ... 14 = the last fifteen frames of the stream (zero after configure / reset).
    bool fe_configured = false;
    dabgpu_fe_layout fe_layout{};
    int fe_units = 0;                     // FIC + sub-channels: workgroups per ETI frame of the encode kernel
    int fe_cifs = 1, fe_fic_out = 288;    // ETI frames per transmission frame; punctured FIC bytes per ETI frame
    std::vector<uint8_t> fe_header;       // bytes 5 ... 8 + 4 NST of the frame the layout was read from (byte 6: MID bits only)
    dabgpu_api::DevBuf d_fe_prbs, d_fe_units, d_fe_owner, d_fe_hist, d_fe_tmp, d_fe_fic, d_fe_eti;
    dabgpu_api::DevBuf d_fe_seed;          // dabgpu_chain_seed_eti: the coded bits of the lead-in transmission frame
    dabgpu_api::DevBuf d_phase;                        // tool builds only (-DDABGPU_PHASE_TIMING): the frame kernel's per-phase cycle counters
    hipStream_t clip_stream = nullptr;     // stream of the most recent chain call that converted its output
    // TII (f-4): carrier set, the one-frame carrier image and its native-rate response, gain of symbol 1
    dabgpu_api::DevBuf d_acp, d_tii_car, d_tii_frame, d_gain1, d_cic;
    dabgpu_api::DevBuf d_gains;           // gain rounding REFERENCE: the multipliers of a call's symbols
    size_t cic_spacing = 0;               // what d_cic was built for (CicEqualizer, a12: the STAGE entry's table)
    int cic_R = 0;
    // the chain's own CicEqualizer table (a setting: uploaded by apply_settings for cur.cic_key(), never touched by the stage
    // entry) and the TII carrier set the carriers kernel reads (rewritten after the lanes have drained: ensure_carrier_acp)
    dabgpu_api::DevBuf d_cic_chain, d_car_acp;
    int car_acp_comb = -1, car_acp_pattern = -1;
    // CFR statistics (f-3) of the most recent chain / OfdmGenerator call, and a scratch set for internal runs
    dabgpu_api::DevBuf d_cfr_counts, d_cfr_mer, d_cfr_papr, d_cfr_tmp;
    int cfr_mer_index = 0;                // myMERCalcIndex (src/OfdmGenerator.h:109): advances once per frame
    int cfr_last_base = 0;
    size_t cfr_last_frames = 0;
    hipStream_t cfr_last_stream = nullptr;
    // the receive-side stages (a new one adds its struct above and its member here)
    dabgpu_api::DemodState demod;
    dabgpu_api::CsiState csi;
    dabgpu_api::SpectrumState spectrum;
    dabgpu_api::DpdState dpd;
    dabgpu_api::DevBuf welch_tw;          // the 2048-entry twiddle table of both in modes II - IV (welch_twiddle)
    dabgpu_api::DecodeState decode;
    dabgpu_api::SyncState sync;
    dabgpu_api::ChannelState channel;
    dabgpu_api::ClockState clock;
    dabgpu_api::ScoState sco;
    dabgpu_api::TunerState tuner;
    dabgpu_api::TiiScanState tii_scan;
    dabgpu_api::CirState cir;
    dabgpu_api::FicState fic;
    dabgpu_api::SuperframeState superframe;
    bool tii_insert = true;               // TII::m_insert (src/TII.h:112): this frame of the stream carries TII
    bool tables_valid = false;            // apply_settings has uploaded every table group once
    unsigned long long tii_seg_epoch = 0; // 1 while the cached segment matches the settings (apply_settings zeroes it), and its stage mask
    unsigned tii_seg_mask = ~0u;
    int tii_seg_len = 0;

    // Batches in flight inside ONE context (the idiom of PipelinedModCodec, src/ModPlugin.cpp:90-154: the caller hands over
    // batch i + 1 while batch i is still being worked on).  A chain call on the context's own stream (stream argument NULL)
    // goes to one of n_lanes internal HIP streams in turn; every lane has its own per-call scratch, so the kernels of
    // consecutive calls overlap where one launch alone cannot fill the chip.  Lane 0 is `stream` and the scratch members
    // above; LaneScope swaps another lane's buffers in for the duration of a call.  Calls with the Resampler stay on lane 0
    // (its state runs from frame to frame).
    struct Lane {
        hipStream_t stream = nullptr;
        hipEvent_t ev = nullptr;
        dabgpu_api::DevBuf d_a, d_b, d_fmt, d_clip, d_gain1, d_gains, d_cfr_counts, d_cfr_mer, d_cfr_papr, d_cfr_tmp, d_car;
    };
    enum { kMaxLanes = 4, kLaneMaxFrames = 2048, kLaneScratchBytes = 256 << 20 };
    Lane lane[kMaxLanes];                 // (entry 0: only `ev` is used)
    bool lane_own_queue[kMaxLanes] = {true, false, false, false};   // the probe found the lane a hardware queue of its own
    int n_lanes = 3;
    int call_lanes = 1;                   // lanes the CURRENT chain call rotates over (1: an explicit stream, lane 0 only)
    unsigned long long lane_seq = 0;
    int clip_lane = 0, cfr_last_lane = 0; // whose scratch holds the clip count / the CFR statistics of the most recent call
    // Ordering between the lanes and the context's own stream for the NULL-stream entry points that do NOT rotate
    // (dabgpu_format_process_dev, dabgpu_post_process_dev): they queue on `stream` behind everything the lanes hold
    // (lane_dirty: the lane has work `stream` has not been ordered behind yet), and a later chain call that goes to
    // another lane is ordered behind them (own_epoch / lane_seen_epoch).
    bool lane_dirty[kMaxLanes] = {false, false, false, false};
    unsigned long long own_epoch = 0, lane_seen_epoch[kMaxLanes] = {0, 0, 0, 0};
    hipEvent_t own_ev = nullptr;
    // The native-rate stream between FIRFilter and Resampler (src/DabModulator.cpp:403-406) in pieces of this many frames
    // through a two-piece ring that stays cache-resident, produced on lane 1's stream while the consumer works on the
    // piece before (dabgpu_set_handover_frames; 0 = one piece, the whole batch through memory)
    int handover_frames = 0;
    hipEvent_t ho_prod[2] = {nullptr, nullptr}, ho_cons[2] = {nullptr, nullptr}, ho_start = nullptr, ho_join = nullptr;

    std::mutex mu;
    dabgpu_api::Settings set;                    // guarded by mu
    dabgpu_api::Settings cur;                    // snapshot used by the processing thread
    unsigned long long applied_epoch = 0;


    // asynchronous host path (dabgpu_chain_submit / dabgpu_chain_collect): two batches in flight,
    // pinned staging on both sides, device->host copies on their own stream
    struct Slot {
        void *h_in = nullptr;                          // pinned (hipHostMalloc)
        size_t h_in_cap = 0, out_bytes = 0;
        int h_out_index = 0;                           // which of the three pinned output buffers this batch lands in
        unsigned long long *h_clip = nullptr;          // pinned: this batch's clipped-component count (output formats)
        dabgpu_api::DevBuf d_in, d_out;
        dabgpu_api::DevBuf d_eti;                      // dabgpu_chain_submit_eti: the batch's ETI frames (d_in then holds the coded bits)
        hipEvent_t computed = nullptr, copied = nullptr;
        hipStream_t stream = nullptr;                  // the lane this batch's kernels were queued on
        bool busy = false;
        int out_format = 0;                            // the output format this batch was submitted with
    } slot[2];
    // Pinned output buffers, THREE for two batches in flight: submit n copies into buffer n mod 3, so the
    // buffer handed out by collect() of batch n is next written by submit n + 3 -- after the collect at the
    // latest the second next submit.  (With one buffer per slot the very next submit overwrote it.)
    void *h_out[3] = {nullptr, nullptr, nullptr};
    size_t h_out_cap[3] = {0, 0, 0};
    unsigned long long submit_seq = 0;
    bool clip_from_collect = false;        // dabgpu_get_num_clipped answers for the batch collect() returned last
    bool clip_valid = false;               // the most recent chain call converted its output (d_clip holds ITS count)
    size_t collected_clipped = 0;
    hipStream_t copy_stream = nullptr;
    int slot_head = 0, slot_count = 0;                 // oldest batch in flight, number in flight
};

namespace dabgpu_api {

int fail(dabgpu_ctx *c, int code, const std::string &msg);
int hip_fail(dabgpu_ctx *c, hipError_t e, const char *what);

#define HIPCHK(ctx, expr)                                                                      \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess) return hip_fail(ctx, e_, #expr);                                 \
    } while (0)


// ---- api_lanes.hip
int lane_stream(dabgpu_ctx *c, int i, hipStream_t *out);          // the stream of lane i (created on first use)
int own_stream_joins_lanes(dabgpu_ctx *c);                         // a NULL-stream call on the context's own stream: behind every lane
int lane_joins_own_stream(dabgpu_ctx *c, int i);                   // a chain call that goes to lane i: behind such work
int drain_lanes(dabgpu_ctx *c);                                    // every stream of the context idle
int chain_dev(dabgpu_ctx *c, const void *d_in, bool from_bits, size_t n_frames, unsigned mask, void *d_iq, size_t out_cap,
              size_t *out_bytes, void *stream);

// lane i's per-call scratch in place of the context's for the lifetime of the object
struct LaneScope {
    dabgpu_ctx *c;
    int i;
    LaneScope(dabgpu_ctx *ctx, int lane) : c(ctx), i(lane) { swap(); }
    ~LaneScope() { swap(); }
    LaneScope(const LaneScope &) = delete;
    LaneScope &operator=(const LaneScope &) = delete;
    void swap()
    {
        if (i == 0) return;
        dabgpu_ctx::Lane &l = c->lane[i];
        std::swap(c->d_a, l.d_a); std::swap(c->d_b, l.d_b); std::swap(c->d_fmt, l.d_fmt); std::swap(c->d_clip, l.d_clip);
        std::swap(c->d_gain1, l.d_gain1); std::swap(c->d_gains, l.d_gains); std::swap(c->d_cfr_counts, l.d_cfr_counts); std::swap(c->d_cfr_mer, l.d_cfr_mer);
        std::swap(c->d_cfr_papr, l.d_cfr_papr); std::swap(c->d_cfr_tmp, l.d_cfr_tmp); std::swap(c->d_car, l.d_car);
    }
};


// ---- api_frontend.hip
// the host-pointer checks of an ETI batch against the configured layout (nothing queued, nothing changed when it fails)
int frontend_check_host(dabgpu_ctx *c, const uint8_t *eti, size_t n_eti);
// shape checks every entry shares (configured, whole transmission frames, max_frames); *n_tf: transmission frames
int frontend_check_shape(dabgpu_ctx *c, size_t n_eti, size_t *n_tf);
// the two launches and the history's move to the front, on `s`; d_bits receives n_eti / cifs-per-frame x tf_input_bytes
int run_frontend(dabgpu_ctx *c, const void *d_eti, size_t n_eti, void *d_bits, hipStream_t s);
// the layout half of frontend_check_host: FICF / NST, the MID bits and the STC words of every frame
int frontend_check_layout(dabgpu_ctx *c, const uint8_t *eti, size_t n_eti);
// The seeds (dabgpu_frontend_seed, dabgpu_chain_seed_eti).  _check: configured, e on a transmission frame, n_leadin =
// min(e, reach); _check_leadin_host: the layout of the lead-in frames and the frame phase of the last one; _rows: the
// history in front of a frame from the m <= 15 ETI frames before it (device memory), on `s` -- a memset of the rows that
// lie before the start of the stream and the encode launch's seed form, nothing else
int frontend_seed_check(dabgpu_ctx *c, size_t n_leadin, uint64_t e, size_t reach);
int frontend_check_leadin_host(dabgpu_ctx *c, const uint8_t *eti, size_t n_leadin);
int frontend_seed_rows(dabgpu_ctx *c, const void *d_eti, size_t m, hipStream_t s);

// ---- api_lanes.hip (the streaming host path; eti: `src` holds ETI frames, n_frames still counts transmission frames)
int chain_submit(dabgpu_ctx *c, const uint8_t *src, size_t n_frames, unsigned mask, bool eti);

// ---- api_context.hip
extern const float kDefaultTaps[45];
extern const char *const kCicBadParameters;          // the refusal of the stage entry and of the setter
bool mode_geometry(int mode, Geometry *g);
size_t tf_in_bytes(const Geometry &g);
size_t tf_samples(const Geometry &g);
template <typename T> hipError_t upload(DevBuf &b, const std::vector<T> &v, hipStream_t s)
{
    hipError_t e = b.reserve(std::max<size_t>(v.size() * sizeof(T), 16));
    if (e != hipSuccess) return e;
    e = hipMemcpyAsync(b.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, s);
    if (e != hipSuccess) return e;
    return hipStreamSynchronize(s);  // v may be a temporary
}

bool design_inverse_filter(const std::vector<float> &taps, int N, int K, std::vector<float> &g_out, double *fit_out);
// least squares by Householder QR in float64 (A: m x n column-major; A and b are overwritten)
bool householder_lstsq(std::vector<double> &A, std::vector<double> &b, int m, int n, std::vector<double> &x,
                       double *rmin = nullptr, double *rmax = nullptr);
int apply_settings(dabgpu_ctx *c);
Tables tables_of(dabgpu_ctx *c);
GainParams gain_of(const dabgpu_ctx *c);

// ---- api_chain.hip
// What one chain call runs and reserves: decided once, by plan_chain; run_chain / run_native do what it says.
struct ChainPlan {
    const char *error = nullptr;          // the request cannot run (DABGPU_E_INVALID, this text); only the sizes below are set then
    bool from_bits = false, keep_stats = true;
    size_t n_frames = 0;
    unsigned mask = 0;                    // normalised: RESAMPLE dropped when the rates are equal
    int fmt = 0;                          // the integer format of the call's output (0: complexf)
    size_t per = 0, native = 0;           // samples per frame of the output / of the native-rate stream
    size_t out_bytes = 0;
    // the native-rate part: one frame kernel (TF_WINDOW in tf_flags: it windows the guard interval itself), or frame kernel
    // -> guard / FIRFilter kernel, the latter with the reference's gain recurrence in between
    enum Form { ONE_KERNEL, UNFUSED, GAIN_REPLAY } form = ONE_KERNEL;
    // Carriers first (the CIC equaliser is on): a kernel in front leaves the equalised carriers in d_car and everything above
    // describes the from-carriers chain that runs on them (from_bits = false, no TII of its own: it is in the carriers).
    // FRONT_BITS: the call's input is coded bits (carriers_from_bits_kernel, which also advances the TII parity);
    // FRONT_CIC: it is the caller's carriers (cic_kernel).
    enum Front { FRONT_NONE, FRONT_BITS, FRONT_CIC } front = FRONT_NONE;
    unsigned tf_flags = 0;                // the frame kernel's final TF_* flags
    int ntaps = 0, chunks_per_frame = 1, syms_per_chunk = 1;
    bool tii = false, tii_inside = false; // the call adds the TII null symbol; the frame kernel does it itself
    bool fuse_native = false, fuse_post = false;   // the integer format is stored by the frame kernel / by the resampler
    bool fuse_poly = false;               // the predistorter rides in the resampler's store
    size_t piece = 0;                     // the hand-over FIRFilter -> Resampler runs in pieces of this many frames (0: one piece)
    // bytes of each per-lane scratch buffer the call reserves (the CFR statistics: the caller's set, or cfr_tmp for an
    // internal run), and their sum
    struct Scratch {
        size_t d_a = 0, d_b = 0, d_fmt = 0, d_gains = 0, d_gain1 = 0, cfr_counts = 0, cfr_mer = 0, cfr_papr = 0, cfr_tmp = 0;
        size_t d_car = 0;
    } scratch;
    size_t scratch_bytes = 0;
};
// (cic: the call is a chain entry point's and the context's CIC equaliser applies -- chain_cic(c); the stage entries and the
// chain's internal runs that borrow the dispatch never equalise)
ChainPlan plan_chain(const dabgpu_ctx *c, bool from_bits, size_t n_frames, unsigned mask, bool apply_format = true,
                     bool keep_stats = true, bool cic = false);
inline bool chain_cic(const dabgpu_ctx *c) { return c->cur.cic_on(); }
// the front kernel of a carriers-first plan, or dabgpu_carriers_process: coded bits -> carriers with the context's TII and CIC
// settings (cic: apply the equaliser), from the TII parity as it stands; does NOT advance the parity
int run_carriers(dabgpu_ctx *c, const void *d_bits, size_t n_frames, float2 *d_car, bool cic, hipStream_t s);
std::vector<float> cic_filter(size_t K, size_t spacing, int R);
unsigned normalised_mask(const Settings &st, unsigned mask);
int auto_chunks(const dabgpu_ctx *c, size_t n_frames);
bool is_pow2(size_t x);
const char *resampler_ratio_error(int N, size_t in_rate, size_t out_rate);
int check_resampler(dabgpu_ctx *c);
int run_resampler(dabgpu_ctx *c, const float2 *d_in, size_t total, float2 *d_out, hipStream_t s, bool fuse_poly = false,
                  unsigned long long *s16_clipped = nullptr);
int run_poly(dabgpu_ctx *c, const float2 *d_in, size_t n, float2 *d_out, hipStream_t s);
int tii_carrier_set(int mode, int comb, int pattern, std::vector<uint8_t> &acp);
int run_native_tii(dabgpu_ctx *c, const ChainPlan &p, const void *d_in, float2 *native_out, hipStream_t s);
int run_front(dabgpu_ctx *c, const ChainPlan &p, const void **d_in, hipStream_t s);
int run_chain(dabgpu_ctx *c, const ChainPlan &p, const void *d_in, void *d_out_v, size_t out_cap, size_t *out_bytes,
              hipStream_t s, bool apply_format = true, int lane = 0);

// ---- api_demod.hip
// The monitor (dabgpu_set_monitor) on a chain call from coded bits.  monitor_refusal: the message when the monitor is on and
// the planned call cannot be demodulated (nullptr: off, or fine) -- asked before anything is queued.  run_monitor: behind
// run_chain on the same stream, the call's output against the call's own bits; nothing when the monitor is off.
const char *monitor_refusal(const dabgpu_ctx *c, const ChainPlan &p);
extern const char *const kMonitorNoSubmit;
int run_monitor(dabgpu_ctx *c, const ChainPlan &p, const void *d_bits, const void *d_iq, hipStream_t s);
// the arguments every walk over the data symbols of whole frames shares (DemodArgs, ScoArgs), at the context's run geometry
void fill_rx_symbols(dabgpu_ctx *c, const void *d_iq, int format, size_t n_frames, int early, RxSymbolArgs &a);

// ---- api_decode.hip
// dabgpu_frontend_configure's last step: the decoder's view of the new layout (survivor slots, the overlap refusal) and a zero
// history; the context is idle
int decode_configure(dabgpu_ctx *c);

// ---- api_spectrum.hip
// The spectrum monitor (dabgpu_set_spectrum_monitor) on a chain call from coded bits: behind run_chain (and run_monitor) on
// the same stream, over the samples the call wrote; nothing when it is off.
extern const char *const kSpectrumNoSubmit;
int run_spectrum_monitor(dabgpu_ctx *c, const ChainPlan &p, const void *d_iq, hipStream_t s);

// host-pointer stage wrapper: H2D, launch, D2H on the context stream
struct HostIO {
    dabgpu_ctx *c;
    explicit HostIO(dabgpu_ctx *ctx) : c(ctx) {}
    int in(DevBuf &b, const void *h, size_t n)
    {
        HIPCHK(c, b.reserve(std::max<size_t>(n, 16)));
        if (n) HIPCHK(c, hipMemcpyAsync(b.p, h, n, hipMemcpyHostToDevice, c->stream));
        return DABGPU_OK;
    }
    int out(void *h, const void *d, size_t n)
    {
        if (n) HIPCHK(c, hipMemcpyAsync(h, d, n, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return DABGPU_OK;
    }
};

inline int check_out(dabgpu_ctx *c, size_t need, size_t cap, size_t *out_bytes)
{
    if (out_bytes) *out_bytes = need;
    if (need > cap) return fail(c, DABGPU_E_CAPACITY, "output buffer too small");
    return DABGPU_OK;
}

#define CTXCHK(c)                                                                              \
    do {                                                                                       \
        if (!(c)) return DABGPU_E_INVALID;                                                     \
        hipError_t e_ = hipSetDevice((c)->device);                                             \
        if (e_ != hipSuccess) return hip_fail((c), e_, "hipSetDevice");                        \
    } while (0)

// ---- what the entry points of the receive-side stages are built from
// bytes of one complex sample: complexf, DABGPU_FMT_S16, u8 / s8
inline size_t sample_bytes(int format) { return format == 0 ? sizeof(float2) : format == DABGPU_FMT_S16 ? 4 : 2; }

// A capture argument, in this order: the format is complexf or s16, the pointer is not null, a device pointer is aligned to
// a sample.  `stage` starts the messages.  An entry whose order or wording differs uses the pieces, or its own lines.
inline int check_capture_format(dabgpu_ctx *c, const char *stage, int format)
{
    if (format == 0 || format == DABGPU_FMT_S16) return DABGPU_OK;
    return fail(c, DABGPU_E_INVALID, std::string(stage) + ": input format is complexf (0) or DABGPU_FMT_S16");
}
inline bool sample_aligned(const void *p, int format) { return ((uintptr_t)p & (sample_bytes(format) - 1)) == 0; }
inline int fail_misaligned(dabgpu_ctx *c, const char *stage)
{
    return fail(c, DABGPU_E_INVALID, std::string(stage) + ": buffers must be aligned to a sample (eight bytes complexf, four bytes s16)");
}
inline int check_capture(dabgpu_ctx *c, const char *stage, const void *p, int format, bool device)
{
    if (int rc = check_capture_format(c, stage, format)) return rc;
    if (!p) return fail(c, DABGPU_E_INVALID, "null argument");
    if (device && !sample_aligned(p, format)) return fail_misaligned(c, stage);
    return DABGPU_OK;
}

// The prologue of a device call: the stream it goes to -- the caller's, or the context's own behind every lane (the input
// may be a chain call's output on any lane) -- and the trace scope.  rc is not DABGPU_OK when the lanes could not be
// joined: the entry returns it.
struct DevCall {
    hipStream_t s;
    int rc;
    TraceScope trace;
    DevCall(dabgpu_ctx *c, void *stream)
        : s(stream ? (hipStream_t)stream : c->stream), rc(stream ? DABGPU_OK : own_stream_joins_lanes(c)),
          trace(rc == DABGPU_OK && c->trace_enabled ? &c->last_variant : nullptr) {}
};

// waits for a result that is complete on `result_stream` (nullptr: nothing was queued elsewhere -- the context's own)
inline hipError_t wait_result(dabgpu_ctx *c, hipStream_t result_stream)
{
    return hipStreamSynchronize(result_stream ? result_stream : c->stream);
}

// ---- what the two Welch measurements (the spectrum monitor, the DPD cross-spectrum) share on the host
// The 2048-entry twiddle table: the context's own in Mode I, else a buffer built on first use -- written once, and the context's
// stream has been waited for (upload) before this returns, so a call on any stream may read it.
inline int welch_twiddle(dabgpu_ctx *c, const float2 **table)
{
    if (c->g.N != SPECTRUM_NFFT && !c->welch_tw.p) {
        std::vector<float2> tw(SPECTRUM_NFFT);
        for (int m = 0; m < SPECTRUM_NFFT; ++m) {
            const double a = 2.0 * M_PI * (double)m / (double)SPECTRUM_NFFT;
            tw[m] = make_float2((float)std::cos(a), (float)std::sin(a));
        }
        DevBuf b;
        HIPCHK(c, upload(b, tw, c->stream));
        c->welch_tw = std::move(b);
    }
    *table = (const float2 *)(c->g.N == SPECTRUM_NFFT ? c->d_twiddle.p : c->welch_tw.p);
    return DABGPU_OK;
}
// `width` float64 sums and the segment count behind them (acc, complete on `result_stream`); zeros when nothing has run (ready
// false)
inline int fetch_welch_sums(dabgpu_ctx *c, bool ready, const DevBuf &acc, hipStream_t result_stream, size_t width, std::vector<double> &sums,
                            unsigned long long *segments)
{
    sums.assign(width + 1, 0.0);
    if (ready) {
        HIPCHK(c, wait_result(c, result_stream));
        HIPCHK(c, hipMemcpy(sums.data(), acc.p, sums.size() * sizeof(double), hipMemcpyDeviceToHost));
    }
    std::memcpy(segments, &sums[width], sizeof *segments);
    return DABGPU_OK;
}

// The host-pointer form of a capture stage, after its checks: the context idle, the capture in `staging`, the stage's _dev
// entry on the context's stream (dev(d_capture) -> rc), the result complete.
template <typename DevEntry> int capture_from_host(dabgpu_ctx *c, DevBuf &staging, const void *capture, size_t bytes, DevEntry dev)
{
    int rc = dabgpu_synchronize(c);
    if (rc) return rc;
    HostIO io(c);
    if ((rc = io.in(staging, capture, bytes))) return rc;
    if ((rc = dev(staging.p))) return rc;
    return io.out(nullptr, nullptr, 0);
}

// ---- what the entry points of the streamed stages (StreamStage) are built from.  What differs between them in a refusal:
struct StreamRules {
    const char *stage;                    // starts the messages
    const char *n_name;                   // the call's sample count in the header: n_samples, n_in
    const char *unit;                     // what dabgpu_debug_*_run_samples counts per workgroup: samples, outputs
    const char *misaligned;               // the stage's own alignment refusal; nullptr: fail_misaligned's
    unsigned long long max_position;      // the stream's position at most; 0: any
    const char *bad_position;             // ... and its refusal
};

// A call's buffers, after the stage's own lines (configured, formats), in this order: not null, aligned to a sample, n not 0
// and at most 2^40, the position bound, the capacity (*n_out = count first: what the caller has to offer), no overlap.
// count: the outputs the call makes (the channel's: n, with out_cap = n and an n_out of its own).
inline int check_stream_call(dabgpu_ctx *c, const StreamStage &st, const StreamRules &r, const void *in, int in_format, size_t n,
                             const void *out, int out_format, unsigned long long count, size_t out_cap, size_t *n_out)
{
    const std::string stage = std::string(r.stage) + ": ";
    if (!in || !out || !n_out) return fail(c, DABGPU_E_INVALID, "null argument");
    if (!sample_aligned(in, in_format) || !sample_aligned(out, out_format))
        return r.misaligned ? fail(c, DABGPU_E_INVALID, r.misaligned) : fail_misaligned(c, r.stage);
    if (n == 0) return fail(c, DABGPU_E_INVALID, stage + r.n_name + " must not be 0");
    if (n > ((size_t)1 << 40)) return fail(c, DABGPU_E_INVALID, stage + r.n_name + " must not exceed 2^40");
    if (r.max_position && st.position + n > r.max_position) return fail(c, DABGPU_E_INVALID, r.bad_position);
    if (count > out_cap) {
        *n_out = (size_t)count;
        return fail(c, DABGPU_E_CAPACITY, stage + "output buffer too small");
    }
    const uintptr_t i0 = (uintptr_t)in, i1 = i0 + n * sample_bytes(in_format);
    const uintptr_t o0 = (uintptr_t)out, o1 = o0 + (size_t)count * sample_bytes(out_format);
    if (i0 < o1 && o0 < i1) return fail(c, DABGPU_E_INVALID, stage + "input and output must not overlap");
    return DABGPU_OK;
}

// The history hand-over of a streamed _dev call on stream s.  begin, in front of the stage's kernels: the two histories of
// `capacity` samples, cur (what this call reads, zeroed first where that is pending) and next.  end, behind them: the call's
// last H <= capacity inputs into next, which the next call reads; the position moves on; the result is complete on s.
struct StreamHistory {
    float2 *cur = nullptr, *next = nullptr;
    int capacity = 0;
    int begin(dabgpu_ctx *c, StreamStage &st, int capacity_, hipStream_t s)
    {
        capacity = capacity_;
        const size_t bytes = (size_t)capacity * sizeof(float2);
        HIPCHK(c, st.hist.reserve(2 * bytes));
        cur = (float2 *)((char *)st.hist.p + (size_t)st.hist_cur * bytes);
        next = (float2 *)((char *)st.hist.p + (size_t)(st.hist_cur ^ 1) * bytes);
        if (st.zero_pending) {
            HIPCHK(c, hipMemsetAsync(cur, 0, bytes, s));
            st.zero_pending = false;
        }
        return DABGPU_OK;
    }
    int end(dabgpu_ctx *c, StreamStage &st, const void *d_in, int in_format, size_t n, int H, hipStream_t s)
    {
        HIPCHK(c, H <= capacity ? launch_stream_history(d_in, in_format, (long long)n, H, cur, next, s) : hipErrorInvalidValue);
        st.hist_cur ^= 1;
        st.position += n;
        st.stream = s;
        return DABGPU_OK;
    }
};

// The host-pointer form of a streamed stage, after its checks: the context idle, the input in st.in, room for the output in
// st.out, the stage's _dev entry on the context's stream (dev(d_in, d_out) -> rc), the output copied out and complete.
template <typename DevEntry>
int stream_from_host(dabgpu_ctx *c, StreamStage &st, const void *in, size_t in_bytes, void *out, size_t out_bytes, DevEntry dev)
{
    int rc = dabgpu_synchronize(c);
    if (rc) return rc;
    HostIO io(c);
    if ((rc = io.in(st.in, in, in_bytes))) return rc;
    HIPCHK(c, st.out.reserve(std::max<size_t>(out_bytes, 16)));
    if ((rc = dev(st.in.p, st.out.p))) return rc;
    return io.out(out, st.out.p, out_bytes);
}

// the bodies of dabgpu_*_reset, dabgpu_get_*_position and dabgpu_debug_*_run_samples, behind the entry's CTXCHK
inline int stream_reset(dabgpu_ctx *c, StreamStage &st, const StreamRules &r, uint64_t position)
{
    if (r.max_position && position > r.max_position) return fail(c, DABGPU_E_INVALID, r.bad_position);
    st.zero_pending = true;               // (the next call zeroes the history on its own stream, in front of its kernels)
    st.position = position;
    return DABGPU_OK;
}
inline int stream_position(dabgpu_ctx *c, const StreamStage &st, uint64_t *position)
{
    if (!position) return fail(c, DABGPU_E_INVALID, "null argument");
    HIPCHK(c, wait_result(c, st.stream));
    *position = st.position;
    return DABGPU_OK;
}
inline int stream_run_samples(dabgpu_ctx *c, StreamStage &st, const StreamRules &r, int samples)
{
    if (samples < 0)
        return fail(c, DABGPU_E_INVALID, std::string(r.stage) + ": " + r.unit + " per workgroup must not be negative (0 = chosen)");
    st.run_samples = samples;
    return DABGPU_OK;
}

}  // namespace dabgpu_api
