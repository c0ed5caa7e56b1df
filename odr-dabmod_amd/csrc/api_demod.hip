// api_demod.hip -- the receiver of demod.hip behind the C-ABI: native-rate IQ -> coded bits and per-frame quality figures, as
// entries of their own (dabgpu_demod / _dev) and as the monitor that rides on a chain call (dabgpu_set_monitor).  The reference
// has no receiver: nothing here replaces a plugin of its flowgraph, which is why no entry is named *_process.
#include "dabgpu_ctx.h"

using namespace dabgpu;
using namespace dabgpu_api;

namespace dabgpu_api {
const char *const kMonitorNoSubmit =
    "monitor: dabgpu_chain_submit* is not monitored (statistics per streaming slot are not kept); turn the monitor off";

void fill_rx_symbols(dabgpu_ctx *c, const void *d_iq, int format, size_t n_frames, int early, RxSymbolArgs &a)
{
    a.g = c->g;
    a.t = tables_of(c);
    a.iq = d_iq;
    a.fmt = format;                      // (0 or DABGPU_FMT_S16: the entries refuse the rest, the launchers check again)
    a.frame_stride = tf_samples(c->g);
    a.n_frames = (int)n_frames;
    demod_runs(c->g, n_frames, c->demod.run_symbols, &a.runs_per_frame, &a.syms_per_run);
    a.early = early;
}

namespace {
const char *const kEarlyRange = "demod: early must lie inside the cyclic prefix (0 ... sym_size - spacing)";

// zero records, one launch; on `s`.  d_iq: n_frames x tf_samples samples of `format` (0 = cf32, DABGPU_FMT_S16).
// d_soft: nullptr (the hard kernel), or n_frames x 8 tf_input_bytes int8 (the soft kernel: the same bits and sums besides).
// weights: nullptr, or n_frames x K fp32 (with d_soft: the weighted soft kernel)
int queue_demod(dabgpu_ctx *c, const void *d_iq, int format, size_t n_frames, int early, void *d_bits_out, const void *d_ref,
                hipStream_t s, void *d_soft = nullptr, const float *weights = nullptr)
{
    HIPCHK(c, c->demod.stats.reserve(std::max<size_t>(n_frames, 1) * sizeof(DemodFrameStats)));
    HIPCHK(c, hipMemsetAsync(c->demod.stats.p, 0, n_frames * sizeof(DemodFrameStats), s));
    DemodArgs a{};
    fill_rx_symbols(c, d_iq, format, n_frames, early, a);
    a.csi_w = weights;
    a.bits_out = (uint8_t *)d_bits_out;
    a.ref_bits = (const uint8_t *)d_ref;
    a.stats = (DemodFrameStats *)c->demod.stats.p;
    a.soft_out = (int8_t *)d_soft;
    HIPCHK(c, launch_demod(a, s));
    c->demod.frames = n_frames;
    c->demod.has_ref = d_ref != nullptr;
    c->demod.stream = s;
    return DABGPU_OK;
}

// The carrier state of n_frames frames and their weights, on `s`: zero sums, the state pass, the weights kernel.
int queue_carrier_state(dabgpu_ctx *c, const void *d_iq, int format, size_t n_frames, int early, hipStream_t s)
{
    const size_t K = (size_t)c->g.K;
    HIPCHK(c, c->csi.sums.reserve(std::max<size_t>(n_frames, 1) * 2 * K * sizeof(unsigned long long)));
    HIPCHK(c, c->csi.weights.reserve(std::max<size_t>(n_frames, 1) * K * sizeof(float)));
    HIPCHK(c, hipMemsetAsync(c->csi.sums.p, 0, n_frames * 2 * K * sizeof(unsigned long long), s));
    DemodArgs a{};
    fill_rx_symbols(c, d_iq, format, n_frames, early, a);
    a.csi_sums = (unsigned long long *)c->csi.sums.p;
    HIPCHK(c, launch_demod(a, s));
    HIPCHK(c, launch_csi_weights(a.csi_sums, (float *)c->csi.weights.p, c->g.K, (int)n_frames, c->csi.unit_weights, s));
    c->csi.frames = n_frames;
    c->csi.stream = s;
    return DABGPU_OK;
}

int check_demod(dabgpu_ctx *c, const void *iq, int format, size_t n_frames, int early, const void *bits_out, const void *ref)
{
    if (int rc = check_capture_format(c, "demod", format)) return rc;
    if (early < 0 || early > c->g.sym_size - c->g.N) return fail(c, DABGPU_E_INVALID, kEarlyRange);
    if (n_frames > (size_t)c->max_frames) return fail(c, DABGPU_E_CAPACITY, "n_frames exceeds max_frames of the context");
    if (n_frames && !iq) return fail(c, DABGPU_E_INVALID, "null argument");
    if (((uintptr_t)iq | (uintptr_t)bits_out | (uintptr_t)ref) & 3u)
        return fail(c, DABGPU_E_INVALID, "demod: buffers must be aligned to four bytes");
    return DABGPU_OK;
}
}  // namespace

const char *monitor_refusal(const dabgpu_ctx *c, const ChainPlan &p)
{
    if (!c->cur.monitor || (!p.from_bits && p.front != ChainPlan::FRONT_BITS)) return nullptr;
    if (p.mask & DABGPU_STAGE_RESAMPLE)
        return "monitor: a chain with the Resampler is not monitored (the receiver takes the native rate); turn the monitor off";
    if (p.mask & DABGPU_STAGE_NOGUARD)
        return "monitor: a chain without the guard interval is not monitored; turn the monitor off";
    if (p.fmt != 0 && p.fmt != DABGPU_FMT_S16)
        return "monitor: u8 / s8 output is not monitored (the receiver takes complexf or s16); turn the monitor off";
    int early = c->cur.monitor_early;
    if (early < 0)
        early = ((p.mask & DABGPU_STAGE_FIR) ? (int)c->cur.taps.size() - 1 : 0) + (int)c->cur.overlap;
    if (early > c->g.sym_size - c->g.N) return kEarlyRange;
    return nullptr;
}

int run_monitor(dabgpu_ctx *c, const ChainPlan &p, const void *d_bits, const void *d_iq, hipStream_t s)
{
    if (!c->cur.monitor || p.n_frames == 0) return DABGPU_OK;
    int early = c->cur.monitor_early;
    if (early < 0)
        early = ((p.mask & DABGPU_STAGE_FIR) ? (int)c->cur.taps.size() - 1 : 0) + (int)c->cur.overlap;
    return queue_demod(c, d_iq, p.fmt, p.n_frames, early, nullptr, d_bits, s);
}
}  // namespace dabgpu_api

namespace {
enum { HARD = 0, SOFT = 1, CSI = 2 };     // the three forms of the call (CSI: SOFT behind the carrier state and its weights)

// the device-pointer entry of every form: soft takes d_soft_out (n_frames x 8 tf_input_bytes int8), hard passes nullptr
int demod_dev(dabgpu_ctx *c, int soft, const void *d_iq, int format, size_t n_frames, int early, void *d_soft_out, void *d_bits_out,
              const void *d_ref_bits, void *stream)
{
    CTXCHK(c);
    int rc = apply_settings(c);
    if (rc) return rc;
    if ((rc = check_demod(c, d_iq, format, n_frames, early, d_bits_out, d_ref_bits))) return rc;
    if (soft && !d_soft_out) return fail(c, DABGPU_E_INVALID, "null argument");
    if ((uintptr_t)d_soft_out & 3u) return fail(c, DABGPU_E_INVALID, "demod: buffers must be aligned to four bytes");
    DevCall call(c, stream);
    if (call.rc) return call.rc;
    if (soft == CSI) {
        if ((rc = queue_carrier_state(c, d_iq, format, n_frames, early, call.s))) return rc;
        return queue_demod(c, d_iq, format, n_frames, early, d_bits_out, d_ref_bits, call.s, d_soft_out, (const float *)c->csi.weights.p);
    }
    return queue_demod(c, d_iq, format, n_frames, early, d_bits_out, d_ref_bits, call.s, d_soft_out);
}

// the host-pointer entry of every form
int demod_host(dabgpu_ctx *c, int soft, const void *iq, int format, size_t n_frames, int early, int8_t *soft_out, uint8_t *bits_out,
               const uint8_t *ref_bits)
{
    CTXCHK(c);
    int rc = check_demod(c, iq, format, n_frames, early, nullptr, nullptr);
    if (rc) return rc;
    if (soft && !soft_out) return fail(c, DABGPU_E_INVALID, "null argument");
    if ((rc = dabgpu_synchronize(c))) return rc;                      // (d_out is the synchronous host path's)
    const size_t iq_bytes = n_frames * tf_samples(c->g) * sample_bytes(format);
    const size_t bit_bytes = n_frames * tf_in_bytes(c->g);
    HostIO io(c);
    if ((rc = io.in(c->d_out, iq, iq_bytes))) return rc;
    if (ref_bits && (rc = io.in(c->demod.ref, ref_bits, bit_bytes))) return rc;
    if (bits_out) HIPCHK(c, c->demod.bits.reserve(std::max<size_t>(bit_bytes, 16)));
    if (soft) HIPCHK(c, c->demod.soft.reserve(std::max<size_t>(8 * bit_bytes, 16)));
    if ((rc = demod_dev(c, soft, c->d_out.p, format, n_frames, early, soft ? c->demod.soft.p : nullptr,
                        bits_out ? c->demod.bits.p : nullptr, ref_bits ? c->demod.ref.p : nullptr, c->stream)))
        return rc;
    if (soft && n_frames && (rc = io.out(soft_out, c->demod.soft.p, 8 * bit_bytes))) return rc;
    return io.out(bits_out, c->demod.bits.p, bits_out ? bit_bytes : 0);
}
}  // namespace

extern "C" {
int dabgpu_demod_dev(dabgpu_ctx *c, const void *d_iq, int format, size_t n_frames, int early, void *d_bits_out,
                     const void *d_ref_bits, void *stream)
{
    return demod_dev(c, HARD, d_iq, format, n_frames, early, nullptr, d_bits_out, d_ref_bits, stream);
}

int dabgpu_demod(dabgpu_ctx *c, const void *iq, int format, size_t n_frames, int early, uint8_t *bits_out,
                 const uint8_t *ref_bits)
{
    return demod_host(c, HARD, iq, format, n_frames, early, nullptr, bits_out, ref_bits);
}

int dabgpu_demod_soft_dev(dabgpu_ctx *c, const void *d_iq, int format, size_t n_frames, int early, void *d_soft_out,
                          void *d_bits_out, const void *d_ref_bits, void *stream)
{
    return demod_dev(c, SOFT, d_iq, format, n_frames, early, d_soft_out, d_bits_out, d_ref_bits, stream);
}

int dabgpu_demod_soft(dabgpu_ctx *c, const void *iq, int format, size_t n_frames, int early, int8_t *soft_out, uint8_t *bits_out,
                      const uint8_t *ref_bits)
{
    return demod_host(c, SOFT, iq, format, n_frames, early, soft_out, bits_out, ref_bits);
}

int dabgpu_demod_csi_dev(dabgpu_ctx *c, const void *d_iq, int format, size_t n_frames, int early, void *d_soft_out,
                         void *d_bits_out, const void *d_ref_bits, void *stream)
{
    return demod_dev(c, CSI, d_iq, format, n_frames, early, d_soft_out, d_bits_out, d_ref_bits, stream);
}

int dabgpu_demod_csi(dabgpu_ctx *c, const void *iq, int format, size_t n_frames, int early, int8_t *soft_out, uint8_t *bits_out,
                     const uint8_t *ref_bits)
{
    return demod_host(c, CSI, iq, format, n_frames, early, soft_out, bits_out, ref_bits);
}

int dabgpu_demod_carrier_state_dev(dabgpu_ctx *c, const void *d_iq, int format, size_t n_frames, int early, void *stream)
{
    CTXCHK(c);
    int rc = apply_settings(c);
    if (rc) return rc;
    if ((rc = check_demod(c, d_iq, format, n_frames, early, nullptr, nullptr))) return rc;
    DevCall call(c, stream);
    if (call.rc) return call.rc;
    return queue_carrier_state(c, d_iq, format, n_frames, early, call.s);
}

int dabgpu_demod_carrier_state(dabgpu_ctx *c, const void *iq, int format, size_t n_frames, int early)
{
    CTXCHK(c);
    int rc = check_demod(c, iq, format, n_frames, early, nullptr, nullptr);
    if (rc) return rc;
    if ((rc = dabgpu_synchronize(c))) return rc;                      // (d_out is the synchronous host path's)
    HostIO io(c);
    if ((rc = io.in(c->d_out, iq, n_frames * tf_samples(c->g) * sample_bytes(format)))) return rc;
    if ((rc = dabgpu_demod_carrier_state_dev(c, c->d_out.p, format, n_frames, early, c->stream))) return rc;
    return io.out(nullptr, nullptr, 0);
}

int dabgpu_get_carrier_state(dabgpu_ctx *c, size_t frame, int64_t *A, int64_t *V, float *w)
{
    CTXCHK(c);
    if (frame >= c->csi.frames)
        return fail(c, DABGPU_E_INVALID, "no carrier state for this frame (no call yet, or frame index out of range)");
    HIPCHK(c, wait_result(c, c->csi.stream));
    const size_t K = (size_t)c->g.K;
    if (A || V) {
        std::vector<int64_t> both(2 * K);
        HIPCHK(c, hipMemcpy(both.data(), (const int64_t *)c->csi.sums.p + frame * 2 * K, 2 * K * sizeof(int64_t), hipMemcpyDeviceToHost));
        for (size_t k = 0; k < K; ++k) {
            if (A) A[k] = both[2 * k];
            if (V) V[k] = both[2 * k + 1];
        }
    }
    if (w) HIPCHK(c, hipMemcpy(w, (const float *)c->csi.weights.p + frame * K, K * sizeof(float), hipMemcpyDeviceToHost));
    return DABGPU_OK;
}

int dabgpu_debug_csi_unit_weights(dabgpu_ctx *c, int enable)
{
    if (!c) return DABGPU_E_INVALID;
    c->csi.unit_weights = enable != 0;
    return DABGPU_OK;
}

int dabgpu_get_demod_stats(dabgpu_ctx *c, size_t frame, dabgpu_demod_stats *out)
{
    CTXCHK(c);
    if (!out) return fail(c, DABGPU_E_INVALID, "null argument");
    if (frame >= c->demod.frames)
        return fail(c, DABGPU_E_INVALID, "no demodulator statistics for this frame (no call yet, or frame index out of range)");
    HIPCHK(c, wait_result(c, c->demod.stream));
    DemodFrameStats st;
    HIPCHK(c, hipMemcpy(&st, (const DemodFrameStats *)c->demod.stats.p + frame, sizeof st, hipMemcpyDeviceToHost));
    std::memset(out, 0, sizeof *out);
    out->sum_signal = st.sum_signal;
    out->sum_quadrature = st.sum_quadrature;
    out->bit_errors = st.bit_errors;
    out->n_bits = c->demod.has_ref ? 8 * (uint64_t)tf_in_bytes(c->g) : 0;
    const unsigned mbits = ~st.min_margin_inv;
    float m;
    std::memcpy(&m, &mbits, sizeof m);
    out->min_margin = st.min_margin_inv ? (double)m : 0.0;
    return DABGPU_OK;
}

int dabgpu_demod_check_early(int mode, int early)
{
    Geometry g;
    if (!mode_geometry(mode, &g)) return fail(nullptr, DABGPU_E_INVALID, "demod: transmission mode not valid");
    if (early < 0 || early > g.sym_size - g.N) return fail(nullptr, DABGPU_E_INVALID, kEarlyRange);
    return DABGPU_OK;
}

int dabgpu_set_monitor(dabgpu_ctx *c, int enable, int early)
{
    if (!c) return DABGPU_E_INVALID;
    if (enable && early > c->g.sym_size - c->g.N) return fail(c, DABGPU_E_INVALID, kEarlyRange);
    std::lock_guard<std::mutex> lk(c->mu);
    const int e = early < 0 ? -1 : early;
    if (c->set.monitor == (enable != 0) && c->set.monitor_early == e) return DABGPU_OK;
    c->set.monitor = enable != 0;
    c->set.monitor_early = e;
    ++c->set.epoch;
    return DABGPU_OK;
}

int dabgpu_debug_demod_run_symbols(dabgpu_ctx *c, int symbols)
{
    if (!c) return DABGPU_E_INVALID;
    if (symbols < 0) return fail(c, DABGPU_E_INVALID, "demod: symbols per run: a positive number, or 0 = by the batch size");
    c->demod.run_symbols = symbols;
    return DABGPU_OK;
}

}  // extern "C"
