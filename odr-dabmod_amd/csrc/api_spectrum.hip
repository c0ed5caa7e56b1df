// api_spectrum.hip -- the spectrum monitor of spectrum.hip behind the C-ABI: the Welch power spectrum of a sample buffer as
// entries of their own (dabgpu_spectrum / _dev), as the monitor that rides on a chain call (dabgpu_set_spectrum_monitor), the
// window tables and the mask check (host only).  The reference has no such stage: no entry is named *_process.
#include "dabgpu_ctx.h"

using namespace dabgpu;
using namespace dabgpu_api;

namespace dabgpu_api {
const char *const kSpectrumNoSubmit =
    "spectrum monitor: dabgpu_chain_submit* is not monitored (two batches in flight would race on one set of sums); turn the "
    "spectrum monitor off";

namespace {
enum { kWindows = 3 };
const char *const kBadWindow = "spectrum: window is 0 (rectangular), 1 (Hann) or 2 (Blackman-Harris)";
const char *const kBadFormat = "spectrum: input format is complexf (0), DABGPU_FMT_S16, DABGPU_FMT_U8 or DABGPU_FMT_S8";

// periodic form, float64, one rounding to fp32
bool window_table(int window, float *out)
{
    const int N = SPECTRUM_NFFT;
    for (int k = 0; k < N; ++k) {
        const double x = 2.0 * M_PI * (double)k / (double)N;
        double w;
        switch (window) {
        case 0: w = 1.0; break;
        case 1: w = 0.5 - 0.5 * std::cos(x); break;
        case 2: w = 0.35875 - 0.48829 * std::cos(x) + 0.14128 * std::cos(2.0 * x) - 0.01168 * std::cos(3.0 * x); break;
        default: return false;
        }
        out[k] = (float)w;
    }
    return true;
}

double window_sum_w2(int window)
{
    std::vector<float> w(SPECTRUM_NFFT);
    if (!window_table(window, w.data())) return 0.0;
    double s = 0.0;
    for (float x : w) s += (double)x * (double)x;
    return s;
}

// tables and sums on first use: written once, never rewritten, so that a call on any stream may read them
int spectrum_ready(dabgpu_ctx *c)
{
    if (c->spectrum.ready) return DABGPU_OK;
    std::vector<float> win(kWindows * SPECTRUM_NFFT);
    for (int w = 0; w < kWindows; ++w) window_table(w, win.data() + (size_t)w * SPECTRUM_NFFT);
    HIPCHK(c, upload(c->spectrum.win, win, c->stream));
    HIPCHK(c, c->spectrum.acc.reserve((SPECTRUM_NFFT + 1) * sizeof(double)));
    HIPCHK(c, hipMemsetAsync(c->spectrum.acc.p, 0, (SPECTRUM_NFFT + 1) * sizeof(double), c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->spectrum.ready = true;
    return DABGPU_OK;
}

int check_spectrum(dabgpu_ctx *c, const void *iq, int format, size_t n_samples, int window, int accumulate)
{
    if (format != 0 && format != DABGPU_FMT_S16 && format != DABGPU_FMT_U8 && format != DABGPU_FMT_S8)
        return fail(c, DABGPU_E_INVALID, kBadFormat);
    if (window < 0 || window >= kWindows) return fail(c, DABGPU_E_INVALID, kBadWindow);
    if (n_samples && !iq) return fail(c, DABGPU_E_INVALID, "null argument");
    if ((uintptr_t)iq & (sample_bytes(format) - 1))
        return fail(c, DABGPU_E_INVALID, "spectrum: the buffer must be aligned to the sample size (8 / 4 / 2 / 2 bytes)");
    if (accumulate && c->spectrum.window >= 0 && c->spectrum.window != window)
        return fail(c, DABGPU_E_INVALID, "spectrum: the sums were formed with another window; dabgpu_reset_spectrum first");
    return DABGPU_OK;
}

// the two launches on `s` (the reduce kernel alone when a call that starts over has no segment; nothing when an accumulating
// one has none)
int queue_spectrum(dabgpu_ctx *c, const void *d_iq, int format, size_t n_samples, int window, bool accumulate, double rate_hz,
                   hipStream_t s)
{
    SpectrumArgs a{};
    int rc = spectrum_ready(c);
    if (!rc) rc = welch_twiddle(c, &a.twiddle);
    if (rc) return rc;
    a.iq = d_iq;
    a.fmt = format;
    a.n_segments = welch_n_segments(n_samples);
    spectrum_runs(a.n_segments, c->spectrum.run_segments, kSpectrumMaxRuns, &a.n_runs, &a.segs_per_run);
    a.window = (const float *)c->spectrum.win.p + (size_t)window * SPECTRUM_NFFT;
    a.acc = (double *)c->spectrum.acc.p;
    a.accumulate = accumulate ? 1 : 0;
    if (a.n_segments > 0 || !accumulate) {
        HIPCHK(c, c->spectrum.rows.reserve(std::max<size_t>((size_t)a.n_runs, 1) * SPECTRUM_NFFT * sizeof(double)));
        a.rows = (double *)c->spectrum.rows.p;
        HIPCHK(c, launch_spectrum(a, s));
        c->spectrum.window = window;           // (only what was queued binds the sums to a window and a rate)
        c->spectrum.rate_hz = rate_hz;
        c->spectrum.stream = s;
    }
    return DABGPU_OK;
}
}  // namespace

int run_spectrum_monitor(dabgpu_ctx *c, const ChainPlan &p, const void *d_iq, hipStream_t s)
{
    if (!c->cur.spectrum || p.n_frames == 0) return DABGPU_OK;
    const int window = c->cur.spectrum_window;
    const double rate = (p.mask & DABGPU_STAGE_RESAMPLE) ? 2048000.0 * (double)c->cur.rs_out / (double)c->cur.rs_in : 2048000.0;
    // the sums go on while window and rate are theirs; a change starts them over (two frequency axes do not add)
    const bool accumulate = c->spectrum.window == window && c->spectrum.rate_hz == rate;
    return queue_spectrum(c, d_iq, p.fmt, p.out_bytes / sample_bytes(p.fmt), window, accumulate, rate, s);
}
}  // namespace dabgpu_api

extern "C" {
int dabgpu_spectrum_window(int window, float *out2048)
{
    if (!out2048) return fail(nullptr, DABGPU_E_INVALID, "null argument");
    if (!window_table(window, out2048)) return fail(nullptr, DABGPU_E_INVALID, kBadWindow);
    return DABGPU_OK;
}

int dabgpu_spectrum_dev(dabgpu_ctx *c, const void *d_iq, int format, size_t n_samples, int window, int accumulate, void *stream)
{
    CTXCHK(c);
    int rc = apply_settings(c);
    if (rc) return rc;
    if ((rc = check_spectrum(c, d_iq, format, n_samples, window, accumulate))) return rc;
    DevCall call(c, stream);
    if (call.rc) return call.rc;
    // (a stand-alone call does not know the rate: 0, unless it adds to sums that have one)
    return queue_spectrum(c, d_iq, format, n_samples, window, accumulate != 0, accumulate ? c->spectrum.rate_hz : 0.0, call.s);
}

int dabgpu_spectrum(dabgpu_ctx *c, const void *iq, int format, size_t n_samples, int window, int accumulate)
{
    CTXCHK(c);
    int rc = check_spectrum(c, iq, format, n_samples, window, accumulate);
    if (rc) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));                        // (the staging buffer may still be read by the call before)
    HostIO io(c);
    if ((rc = io.in(c->spectrum.in, iq, n_samples * sample_bytes(format)))) return rc;
    if ((rc = dabgpu_spectrum_dev(c, c->spectrum.in.p, format, n_samples, window, accumulate, c->stream))) return rc;
    return io.out(nullptr, nullptr, 0);
}

int dabgpu_get_spectrum(dabgpu_ctx *c, double *raw2048, dabgpu_spectrum_info *info)
{
    CTXCHK(c);
    std::vector<double> host;
    unsigned long long n;
    if (int rc = fetch_welch_sums(c, c->spectrum.ready, c->spectrum.acc, c->spectrum.stream, SPECTRUM_NFFT, host, &n)) return rc;
    if (raw2048) std::memcpy(raw2048, host.data(), SPECTRUM_NFFT * sizeof(double));
    if (info) {
        std::memset(info, 0, sizeof *info);
        info->segments = n;
        info->nfft = SPECTRUM_NFFT;
        info->window = c->spectrum.window;
        info->sum_w2 = c->spectrum.window >= 0 ? window_sum_w2(c->spectrum.window) : 0.0;
        info->rate_hz = c->spectrum.rate_hz;
    }
    return DABGPU_OK;
}

int dabgpu_reset_spectrum(dabgpu_ctx *c)
{
    CTXCHK(c);
    if (c->spectrum.ready) {
        HIPCHK(c, wait_result(c, c->spectrum.stream));
        HIPCHK(c, hipMemset(c->spectrum.acc.p, 0, (SPECTRUM_NFFT + 1) * sizeof(double)));
    }
    c->spectrum.window = -1;
    c->spectrum.rate_hz = 0.0;
    return DABGPU_OK;
}

int dabgpu_set_spectrum_monitor(dabgpu_ctx *c, int enable, int window)
{
    if (!c) return DABGPU_E_INVALID;
    if (window < 0 || window >= kWindows) return fail(c, DABGPU_E_INVALID, kBadWindow);
    std::lock_guard<std::mutex> lk(c->mu);
    if (c->set.spectrum == (enable != 0) && c->set.spectrum_window == window) return DABGPU_OK;
    c->set.spectrum = enable != 0;
    c->set.spectrum_window = window;
    ++c->set.epoch;
    return DABGPU_OK;
}

int dabgpu_debug_spectrum_run_segments(dabgpu_ctx *c, int segments)
{
    if (!c) return DABGPU_E_INVALID;
    if (segments < 0) return fail(c, DABGPU_E_INVALID, "spectrum: segments per run: a positive number, or 0 = by the input size");
    c->spectrum.run_segments = segments;
    return DABGPU_OK;
}

int dabgpu_spectrum_check_mask(const double *raw, int nfft, double rate_hz, const double *offs_hz, const double *limit_db,
                               int n_points, double oob_from_hz, dabgpu_mask_result *out)
{
    if (!raw || !out || nfft < 2 || n_points < 0 || (n_points && (!offs_hz || !limit_db)))
        return fail(nullptr, DABGPU_E_INVALID, "check_mask: null argument, or nfft / n_points not valid");
    if (!(rate_hz > 0.0) || !std::isfinite(rate_hz)) return fail(nullptr, DABGPU_E_INVALID, "check_mask: rate_hz must be positive");
    for (int i = 0; i < n_points; ++i)
        if (!std::isfinite(offs_hz[i]) || !std::isfinite(limit_db[i]) || (i && !(offs_hz[i] > offs_hz[i - 1])))
            return fail(nullptr, DABGPU_E_INVALID, "check_mask: mask offsets must be finite and strictly increasing");
    const double band = 768000.0;
    auto freq = [&](int k) { return (double)(k < nfft / 2 ? k : k - nfft) * rate_hz / (double)nfft; };
    double sum = 0.0;
    int in_band = 0;
    for (int k = 0; k < nfft; ++k) {
        const double f = std::fabs(freq(k));
        if (f > 0.0 && f <= band) { sum += raw[k]; ++in_band; }
    }
    if (!in_band) return fail(nullptr, DABGPU_E_INVALID, "check_mask: no bin lies in the occupied band (+-768 kHz) at this rate_hz");
    const double ref = sum / (double)in_band;
    if (!(ref > 0.0) || !std::isfinite(ref))
        return fail(nullptr, DABGPU_E_INVALID, "check_mask: the mean power in the occupied band is zero or not finite");
    dabgpu_mask_result r{};
    r.ref = ref;
    r.oob_max_db = -INFINITY;
    bool any = false, oob_any = false;
    for (int k = 0; k < nfft; ++k) {
        const double f = freq(k), af = std::fabs(f);
        const double level = 10.0 * std::log10(raw[k] / ref);
        if (af >= oob_from_hz && (!oob_any || level > r.oob_max_db)) {
            r.oob_max_db = level;
            r.oob_freq_hz = f;
            oob_any = true;
        }
        if (!n_points || af < offs_hz[0]) continue;
        double limit = limit_db[n_points - 1];
        for (int i = 1; i < n_points; ++i)
            if (af < offs_hz[i]) {
                limit = limit_db[i - 1] + (limit_db[i] - limit_db[i - 1]) * (af - offs_hz[i - 1]) / (offs_hz[i] - offs_hz[i - 1]);
                break;
            }
        const double margin = limit - level;
        ++r.n_checked;
        if (level > limit) ++r.n_violations;
        if (!any || margin < r.worst_margin_db) {
            r.worst_margin_db = margin;
            r.worst_freq_hz = f;
            any = true;
        }
    }
    *out = r;
    return DABGPU_OK;
}

}  // extern "C"
