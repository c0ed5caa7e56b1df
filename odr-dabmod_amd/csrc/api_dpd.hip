// api_dpd.hip -- the DPD measurement of dpd.hip behind the C-ABI: the cross-spectrum of a tx / feedback pair, the alignment
// it gives (host), the aligned amplitude-bin statistics, and the host-only pieces that need no device: the alignment solve, the
// fractional-delay taps and the polynomial fit.  The reference does all of this outside the modulator: no entry is named
// *_process.
#include "dabgpu_ctx.h"

using namespace dabgpu;
using namespace dabgpu_api;

namespace {
enum { kXN = SPECTRUM_NFFT, kXAcc = 4 * SPECTRUM_NFFT + 1, kSums = DPD_MAX_BINS * DPD_FIGURES + 2 };
const unsigned long long kDpdSampleCap = 1ull << 31;
const char *const kBadTxFormat = "dpd: tx is complexf (format 0) or DABGPU_FMT_S16; rx is complexf";

size_t tx_bytes(int format) { return format == 0 ? sizeof(float2) : 4; }

int dpd_ready(dabgpu_ctx *c)
{
    if (c->dpd.ready) return DABGPU_OK;
    HIPCHK(c, c->dpd.xacc.reserve(kXAcc * sizeof(double)));
    HIPCHK(c, c->dpd.sums.reserve(kSums * sizeof(unsigned long long)));
    HIPCHK(c, c->dpd.edge.reserve((DPD_MAX_BINS + 1) * sizeof(float)));
    HIPCHK(c, hipMemsetAsync(c->dpd.xacc.p, 0, kXAcc * sizeof(double), c->stream));
    HIPCHK(c, hipMemsetAsync(c->dpd.sums.p, 0, kSums * sizeof(unsigned long long), c->stream));
    HIPCHK(c, hipMemsetAsync(c->dpd.edge.p, 0, (DPD_MAX_BINS + 1) * sizeof(float), c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->dpd.ready = true;
    return DABGPU_OK;
}

int check_pair(dabgpu_ctx *c, const void *tx, int format, const void *rx, size_t n)
{
    if (format != 0 && format != DABGPU_FMT_S16) return fail(c, DABGPU_E_INVALID, kBadTxFormat);
    if (n && (!tx || !rx)) return fail(c, DABGPU_E_INVALID, "null argument");
    if (((uintptr_t)tx & (tx_bytes(format) - 1)) || ((uintptr_t)rx & (sizeof(float2) - 1)))
        return fail(c, DABGPU_E_INVALID, "dpd: the buffers must be aligned to the sample size (tx 8 / 4 bytes, rx 8)");
    if (n > ((size_t)1 << 40)) return fail(c, DABGPU_E_INVALID, "dpd: more than 2^40 samples");
    return DABGPU_OK;
}

int queue_xspectrum(dabgpu_ctx *c, const void *d_tx, int format, const void *d_rx, size_t n, long long rx_offset, hipStream_t s)
{
    DpdXspecArgs a{};
    int rc = dpd_ready(c);
    if (!rc) rc = welch_twiddle(c, &a.twiddle);
    if (rc) return rc;
    a.tx = d_tx;
    a.fmt = format;
    a.rx = (const float2 *)d_rx;
    a.rx_offset = rx_offset;
    dpd_segments(n, rx_offset, &a.seg_first, &a.n_segments);
    spectrum_runs(a.n_segments, c->dpd.run_segments, kDpdMaxRuns, &a.n_runs, &a.segs_per_run);
    HIPCHK(c, c->dpd.rows.reserve(std::max<size_t>((size_t)a.n_runs, 1) * 4 * kXN * sizeof(double)));
    a.rows = (double *)c->dpd.rows.p;
    a.acc = (double *)c->dpd.xacc.p;
    HIPCHK(c, launch_dpd_xspectrum(a, n, s));
    c->dpd.stream = s;
    return DABGPU_OK;
}

int fetch_xspectrum(dabgpu_ctx *c, std::vector<double> &host, unsigned long long *segments = nullptr)
{
    unsigned long long n;
    return fetch_welch_sums(c, c->dpd.ready, c->dpd.xacc, c->dpd.stream, 4 * kXN, host, segments ? segments : &n);
}

// S as the C-ABI hands it out: re / im interleaved
void interleave_s(const std::vector<double> &host, double *s2)
{
    for (int k = 0; k < kXN; ++k) {
        s2[2 * k] = host[k];
        s2[2 * k + 1] = host[kXN + k];
    }
}

int check_alignment(dabgpu_ctx *c, const dabgpu_dpd_alignment *al)
{
    if (!al) return DABGPU_OK;
    if (al->lag > DABGPU_DPD_MAX_LAG || al->lag < -DABGPU_DPD_MAX_LAG)
        return fail(c, DABGPU_E_INVALID, "dpd: |lag| exceeds DABGPU_DPD_MAX_LAG (1000 samples)");
    if (!(std::fabs(al->tau) < 1.0)) return fail(c, DABGPU_E_INVALID, "dpd: tau must lie in (-1, 1)");
    if (!std::isfinite(al->gain_re) || !std::isfinite(al->gain_im)) return fail(c, DABGPU_E_INVALID, "dpd: the gain is not finite");
    return DABGPU_OK;
}

int check_measure(dabgpu_ctx *c, const void *tx, int format, const void *rx, size_t n, const dabgpu_dpd_alignment *al, float peak,
                  int n_bins, int accumulate)
{
    // (the sample cap first: nothing below may look at a buffer that a refused n describes)
    const unsigned long long held = accumulate ? c->dpd.offered : 0ull;
    if ((unsigned long long)n > kDpdSampleCap || held + (unsigned long long)n > kDpdSampleCap)
        return fail(c, DABGPU_E_INVALID, "dpd: the sums hold at most 2^31 samples; dabgpu_reset_dpd, or accumulate = 0, first");
    int rc = check_pair(c, tx, format, rx, n);
    if (rc) return rc;
    if (n_bins < 1 || n_bins > DABGPU_DPD_MAX_BINS) return fail(c, DABGPU_E_INVALID, "dpd: n_bins is 1 ... 256");
    if (!(peak > 0.f) || !std::isfinite(peak)) return fail(c, DABGPU_E_INVALID, "dpd: peak must be positive and finite");
    if (accumulate && c->dpd.bins && (c->dpd.peak != peak || c->dpd.bins != n_bins))
        return fail(c, DABGPU_E_INVALID, "dpd: the sums were formed with another peak or n_bins; dabgpu_reset_dpd first");
    return check_alignment(c, al);
}

// |sum_k conj(S[k]) e^{j w_k d}|^2 and its derivative in d
struct Correlation {
    const double *s2;
    void at(double d, double *re, double *im, double *dre, double *dim) const
    {
        double ar = 0.0, ai = 0.0, br = 0.0, bi = 0.0;
        for (int k = 0; k < kXN; ++k) {
            const double w = 2.0 * M_PI * (double)(k < kXN / 2 ? k : k - kXN) / (double)kXN;
            const double cs = std::cos(w * d), sn = std::sin(w * d);
            const double xr = s2[2 * k], xi = -s2[2 * k + 1];              // conj(S)
            const double pr = xr * cs - xi * sn, pi = xr * sn + xi * cs;
            ar += pr;
            ai += pi;
            br += -w * pi;                                                 // d/dd: j w (pr + j pi)
            bi += w * pr;
        }
        *re = ar; *im = ai; *dre = br; *dim = bi;
    }
    double power(double d) const
    {
        double ar, ai, br, bi;
        at(d, &ar, &ai, &br, &bi);
        return ar * ar + ai * ai;
    }
    double slope(double d) const
    {
        double ar, ai, br, bi;
        at(d, &ar, &ai, &br, &bi);
        return 2.0 * (ar * br + ai * bi);
    }
};

// min |A c - b| with rows scaled by wt; A: m x 5 column-major.  Returns false when the system is singular.
bool solve5(std::vector<double> A, std::vector<double> b, int m, double *c5, double *cond, double *resid)
{
    std::vector<double> x;
    double lo = 0.0, hi = 0.0;
    if (!householder_lstsq(A, b, m, 5, x, &lo, &hi)) return false;
    for (int i = 0; i < 5; ++i) c5[i] = x[i];
    *cond = hi / lo;
    double r2 = 0.0;
    for (int i = 5; i < m; ++i) r2 += b[i] * b[i];
    *resid = std::sqrt(r2 / (double)m);
    return true;
}

// The host-pointer form of an entry on a tx / feedback pair, after its checks: the pair staged behind whatever still reads
// the staging buffers, the _dev entry on the context's stream (dev(d_tx, d_rx) -> rc), the result complete.
template <typename DevEntry> int pair_from_host(dabgpu_ctx *c, const void *tx, int tx_format, const void *rx, size_t n_samples, DevEntry dev)
{
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HostIO io(c);
    int rc = io.in(c->dpd.tx, tx, n_samples * tx_bytes(tx_format));
    if (!rc) rc = io.in(c->dpd.rx, rx, n_samples * sizeof(float2));
    if (!rc) rc = dev(c->dpd.tx.p, c->dpd.rx.p);
    return rc ? rc : io.out(nullptr, nullptr, 0);
}
}  // namespace

extern "C" {
int dabgpu_dpd_xspectrum_dev(dabgpu_ctx *c, const void *d_tx, int tx_format, const void *d_rx, size_t n_samples, long long rx_offset,
                             void *stream)
{
    CTXCHK(c);
    int rc = apply_settings(c);
    if (rc) return rc;
    if ((rc = check_pair(c, d_tx, tx_format, d_rx, n_samples))) return rc;
    if (rx_offset > (1ll << 40) || rx_offset < -(1ll << 40)) return fail(c, DABGPU_E_INVALID, "dpd: |rx_offset| exceeds 2^40");
    DevCall call(c, stream);
    if (call.rc) return call.rc;
    return queue_xspectrum(c, d_tx, tx_format, d_rx, n_samples, rx_offset, call.s);
}

int dabgpu_dpd_xspectrum(dabgpu_ctx *c, const void *tx, int tx_format, const void *rx, size_t n_samples, long long rx_offset)
{
    CTXCHK(c);
    if (int rc = check_pair(c, tx, tx_format, rx, n_samples)) return rc;
    return pair_from_host(c, tx, tx_format, rx, n_samples, [&](const void *d_tx, const void *d_rx) {
        return dabgpu_dpd_xspectrum_dev(c, d_tx, tx_format, d_rx, n_samples, rx_offset, c->stream);
    });
}

int dabgpu_get_dpd_xspectrum(dabgpu_ctx *c, double *s2048x2, double *p_tx2048, double *p_rx2048, uint64_t *segments)
{
    CTXCHK(c);
    std::vector<double> host;
    unsigned long long n;
    int rc = fetch_xspectrum(c, host, &n);
    if (rc) return rc;
    if (s2048x2) interleave_s(host, s2048x2);
    if (p_tx2048) std::memcpy(p_tx2048, &host[2 * kXN], kXN * sizeof(double));
    if (p_rx2048) std::memcpy(p_rx2048, &host[3 * kXN], kXN * sizeof(double));
    if (segments) *segments = n;
    return DABGPU_OK;
}

int dabgpu_dpd_solve_alignment(const double *s2, const double *p_tx, const double *p_rx, dabgpu_dpd_alignment *out)
{
    if (!s2 || !p_tx || !p_rx || !out) return fail(nullptr, DABGPU_E_INVALID, "null argument");
    double sum_tx = 0.0, sum_rx = 0.0;
    for (int k = 0; k < kXN; ++k) {
        if (!std::isfinite(s2[2 * k]) || !std::isfinite(s2[2 * k + 1]) || !std::isfinite(p_tx[k]) || !std::isfinite(p_rx[k]))
            return fail(nullptr, DABGPU_E_INVALID, "dpd: the cross-spectrum is not finite");
        sum_tx += p_tx[k];
        sum_rx += p_rx[k];
    }
    if (!(sum_tx > 0.0) || !(sum_rx > 0.0)) return fail(nullptr, DABGPU_E_INVALID, "dpd: the cross-spectrum holds no power (no segment?)");
    // c[l] = sum_k conj(S[k]) e^{+2 pi j k l / N}: the circular cross-correlation, largest where rx[i + l] matches tx[i]
    std::vector<double> cs(kXN), sn(kXN);
    for (int m = 0; m < kXN; ++m) {
        cs[m] = std::cos(2.0 * M_PI * (double)m / (double)kXN);
        sn[m] = std::sin(2.0 * M_PI * (double)m / (double)kXN);
    }
    int best_l = 0;
    double best = -1.0;
    for (int l = 0; l < kXN; ++l) {
        double re = 0.0, im = 0.0;
        for (int k = 0; k < kXN; ++k) {
            const int m = (k * l) & (kXN - 1);
            const double xr = s2[2 * k], xi = -s2[2 * k + 1];
            re += xr * cs[m] - xi * sn[m];
            im += xr * sn[m] + xi * cs[m];
        }
        const double p = re * re + im * im;
        if (p > best) { best = p; best_l = l; }
    }
    const int lag = best_l < kXN / 2 ? best_l : best_l - kXN;
    // tau: a scan at 1/32 sample, then bisection on the derivative of the power inside the best point's two neighbours
    const Correlation f{s2};
    const double step = 1.0 / 32.0;
    int bi = 0;
    double bp = -1.0;
    for (int i = -31; i <= 31; ++i) {
        const double p = f.power((double)lag + step * (double)i);
        if (p > bp) { bp = p; bi = i; }
    }
    double lo = step * (double)(bi - 1), hi = step * (double)(bi + 1), tau;
    if (!(f.slope((double)lag + lo) > 0.0)) tau = lo;                  // (the maximum lies at or beyond the bracket's end)
    else if (!(f.slope((double)lag + hi) < 0.0)) tau = hi;
    else {
        for (int it = 0; it < 60 && hi - lo > 1e-13; ++it) {
            const double mid = 0.5 * (lo + hi);
            if (f.slope((double)lag + mid) > 0.0) lo = mid; else hi = mid;
        }
        tau = 0.5 * (lo + hi);
    }
    const double lim = 1.0 - 1e-9;
    tau = std::max(-lim, std::min(lim, tau));
    double ar, ai, br, bim;
    f.at((double)lag + tau, &ar, &ai, &br, &bim);                      // sum conj(S) e^{+jwd}: its conjugate is sum S e^{-jwd}
    out->lag = lag;
    out->tau = tau;
    out->gain_re = ar / sum_rx;
    out->gain_im = -ai / sum_rx;
    out->coherence = (ar * ar + ai * ai) / (sum_tx * sum_rx);
    return DABGPU_OK;
}

int dabgpu_dpd_align_dev(dabgpu_ctx *c, const void *d_tx, int tx_format, const void *d_rx, size_t n_samples, dabgpu_dpd_alignment *out,
                         void *stream)
{
    CTXCHK(c);
    if (!out) return fail(c, DABGPU_E_INVALID, "null argument");
    int rc = apply_settings(c);
    if (rc) return rc;
    if ((rc = check_pair(c, d_tx, tx_format, d_rx, n_samples))) return rc;
    if (n_samples < (size_t)kXN) return fail(c, DABGPU_E_INVALID, "dpd: alignment needs 2048 samples or more");
    DevCall call(c, stream);
    if (call.rc) return call.rc;
    std::vector<double> host, s2(2 * kXN);
    dabgpu_dpd_alignment a1{}, a2{};
    if ((rc = queue_xspectrum(c, d_tx, tx_format, d_rx, n_samples, 0, call.s))) return rc;
    if ((rc = fetch_xspectrum(c, host))) return rc;
    interleave_s(host, s2.data());
    if (dabgpu_dpd_solve_alignment(s2.data(), &host[2 * kXN], &host[3 * kXN], &a1)) return fail(c, DABGPU_E_INVALID, dabgpu_last_error(nullptr));
    if ((rc = check_alignment(c, &a1))) return rc;
    if ((rc = queue_xspectrum(c, d_tx, tx_format, d_rx, n_samples, a1.lag, call.s))) return rc;
    if ((rc = fetch_xspectrum(c, host))) return rc;
    interleave_s(host, s2.data());
    if (dabgpu_dpd_solve_alignment(s2.data(), &host[2 * kXN], &host[3 * kXN], &a2)) return fail(c, DABGPU_E_INVALID, dabgpu_last_error(nullptr));
    a2.lag += a1.lag;
    if ((rc = check_alignment(c, &a2))) return rc;
    *out = a2;
    return DABGPU_OK;
}

int dabgpu_dpd_align(dabgpu_ctx *c, const void *tx, int tx_format, const void *rx, size_t n_samples, dabgpu_dpd_alignment *out)
{
    CTXCHK(c);
    if (int rc = check_pair(c, tx, tx_format, rx, n_samples)) return rc;
    return pair_from_host(c, tx, tx_format, rx, n_samples, [&](const void *d_tx, const void *d_rx) {
        return dabgpu_dpd_align_dev(c, d_tx, tx_format, d_rx, n_samples, out, c->stream);
    });
}

int dabgpu_dpd_delay_taps(double tau, float taps[32])
{
    if (!taps) return fail(nullptr, DABGPU_E_INVALID, "null argument");
    if (!(std::fabs(tau) < 1.0)) return fail(nullptr, DABGPU_E_INVALID, "dpd: tau must lie in (-1, 1)");
    auto bessel_i0 = [](double x) {
        double term = 1.0, sum = 1.0;
        for (int k = 1; k < 64; ++k) {
            term *= (x / (2.0 * (double)k)) * (x / (2.0 * (double)k));
            sum += term;
            if (term < 1e-18 * sum) break;
        }
        return sum;
    };
    const double beta = 10.0, half = 16.0, i0b = bessel_i0(beta);
    const double st = std::sin(M_PI * tau);                            // sin(pi (m - tau)) = -(-1)^m sin(pi tau): exactly 0 at tau = 0
    for (int j = 0; j < DPD_TAPS; ++j) {
        const int m = j - DPD_TAP_CENTRE;
        const double x = (double)m - tau;
        double v;
        if (x == 0.0) v = 1.0;
        else {
            const double sinc = ((m & 1) ? st : -st) / (M_PI * x);
            const double u = x / half;
            v = u * u < 1.0 ? sinc * bessel_i0(beta * std::sqrt(1.0 - u * u)) / i0b : 0.0;
        }
        taps[j] = (float)(v + 0.0);                                    // (no negative zero: tau = 0 is the impulse bit for bit)
    }
    return DABGPU_OK;
}

int dabgpu_dpd_measure_dev(dabgpu_ctx *c, const void *d_tx, int tx_format, const void *d_rx, size_t n_samples,
                           const dabgpu_dpd_alignment *al, float peak, int n_bins, int accumulate, void *stream)
{
    CTXCHK(c);
    int rc = check_measure(c, d_tx, tx_format, d_rx, n_samples, al, peak, n_bins, accumulate);
    if (rc) return rc;
    if ((rc = apply_settings(c))) return rc;
    DevCall call(c, stream);
    if (call.rc) return call.rc;
    if ((rc = dpd_ready(c))) return rc;
    if (c->dpd.peak != peak || c->dpd.bins != n_bins) {
        std::vector<float> edge(DPD_MAX_BINS + 1, 0.f);
        for (int j = 0; j <= n_bins; ++j) {
            const double e = (double)j * (double)peak / (double)n_bins;
            edge[j] = (float)(e * e);
        }
        HIPCHK(c, hipMemcpyAsync(c->dpd.edge.p, edge.data(), edge.size() * sizeof(float), hipMemcpyHostToDevice, call.s));
        HIPCHK(c, hipStreamSynchronize(call.s));                       // (edge is a temporary)
    }
    if (!accumulate) {
        HIPCHK(c, hipMemsetAsync(c->dpd.sums.p, 0, kSums * sizeof(unsigned long long), call.s));
        c->dpd.offered = 0;
    }
    c->dpd.peak = peak;
    c->dpd.bins = n_bins;
    c->dpd.offered += (unsigned long long)n_samples;
    c->dpd.stream = call.s;
    DpdStatsArgs a{};
    a.tx = d_tx;
    a.fmt = tx_format;
    a.rx = (const float2 *)d_rx;
    a.n = (long long)n_samples;
    a.lag = al ? al->lag : 0;
    float taps[DPD_TAPS];
    dabgpu_dpd_delay_taps(al ? al->tau : 0.0, taps);
    std::memcpy(a.h, taps, sizeof taps);
    a.g_re = al ? (float)al->gain_re : 1.f;
    a.g_im = al ? (float)al->gain_im : 0.f;
    a.peak = peak;
    a.n_bins = n_bins;
    a.edge2 = (const float *)c->dpd.edge.p;
    a.tile = c->dpd.tile ? c->dpd.tile : DPD_TILE_MAX;
    a.sums = (unsigned long long *)c->dpd.sums.p;
    HIPCHK(c, launch_dpd_stats(a, call.s));
    return DABGPU_OK;
}

int dabgpu_dpd_measure(dabgpu_ctx *c, const void *tx, int tx_format, const void *rx, size_t n_samples, const dabgpu_dpd_alignment *al,
                       float peak, int n_bins, int accumulate)
{
    CTXCHK(c);
    if (int rc = check_measure(c, tx, tx_format, rx, n_samples, al, peak, n_bins, accumulate)) return rc;
    return pair_from_host(c, tx, tx_format, rx, n_samples, [&](const void *d_tx, const void *d_rx) {
        return dabgpu_dpd_measure_dev(c, d_tx, tx_format, d_rx, n_samples, al, peak, n_bins, accumulate, c->stream);
    });
}

int dabgpu_get_dpd_stats(dabgpu_ctx *c, dabgpu_dpd_stats *out)
{
    CTXCHK(c);
    if (!out) return fail(c, DABGPU_E_INVALID, "null argument");
    std::vector<unsigned long long> host(kSums, 0ull);
    if (c->dpd.ready) {
        HIPCHK(c, wait_result(c, c->dpd.stream));
        HIPCHK(c, hipMemcpy(host.data(), c->dpd.sums.p, host.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    }
    std::memset(out, 0, sizeof *out);
    out->n_bins = c->dpd.bins;
    out->peak = c->dpd.peak;
    out->overflow = host[DPD_MAX_BINS * DPD_FIGURES];
    out->samples_used = host[DPD_MAX_BINS * DPD_FIGURES + 1];
    const double peak = (double)c->dpd.peak, q = 1.0 / 16777216.0;
    for (int b = 0; b < DPD_MAX_BINS; ++b) {
        const unsigned long long *r = &host[(size_t)b * DPD_FIGURES];
        for (int f = 0; f < DPD_FIGURES; ++f) out->raw[b][f] = (int64_t)r[f];
        out->count[b] = r[0];
        out->sum_tx[b] = (double)r[1] * q * peak;
        out->sum_rx[b] = (double)r[2] * q * peak;
        out->sum_phase[b] = (double)(int64_t)r[3] * q;
        out->sum_rx2[b] = (double)r[4] * q * peak * peak;
        out->sum_phase2[b] = (double)r[5] * q;
    }
    return DABGPU_OK;
}

int dabgpu_reset_dpd(dabgpu_ctx *c)
{
    CTXCHK(c);
    if (c->dpd.ready) {
        HIPCHK(c, wait_result(c, c->dpd.stream));
        HIPCHK(c, hipMemset(c->dpd.sums.p, 0, kSums * sizeof(unsigned long long)));
    }
    c->dpd.peak = 0.f;
    c->dpd.bins = 0;
    c->dpd.offered = 0;
    return DABGPU_OK;
}

int dabgpu_debug_dpd_run_segments(dabgpu_ctx *c, int segments)
{
    if (!c) return DABGPU_E_INVALID;
    if (segments < 0) return fail(c, DABGPU_E_INVALID, "dpd: segments per run: a positive number, or 0 = by the input size");
    c->dpd.run_segments = segments;
    return DABGPU_OK;
}

int dabgpu_debug_dpd_tile(dabgpu_ctx *c, int samples)
{
    if (!c) return DABGPU_E_INVALID;
    if (samples < 0 || samples > DPD_TILE_MAX || samples % 256)
        return fail(c, DABGPU_E_INVALID, "dpd: samples per workgroup: a multiple of 256 up to 2048, or 0 = 2048");
    c->dpd.tile = samples;
    return DABGPU_OK;
}

int dabgpu_dpd_fit_poly(const dabgpu_dpd_stats *st, int basis, uint64_t min_count, int weighted, double tx_min, const float prev_am[5],
                        const float prev_pm[5], double lr_am, double lr_pm, float am[5], float pm[5], dabgpu_dpd_fit_info *info)
{
    if (!st || !am || !pm) return fail(nullptr, DABGPU_E_INVALID, "null argument");
    if (basis != DABGPU_DPD_BASIS_MAGSQ && basis != DABGPU_DPD_BASIS_REFERENCE)
        return fail(nullptr, DABGPU_E_INVALID, "dpd: basis is DABGPU_DPD_BASIS_MAGSQ or DABGPU_DPD_BASIS_REFERENCE");
    if (st->n_bins < 1 || st->n_bins > DABGPU_DPD_MAX_BINS || !(st->peak > 0.f) || !std::isfinite(st->peak))
        return fail(nullptr, DABGPU_E_INVALID, "dpd: the statistics hold no measurement (n_bins 1 ... 256, peak > 0)");
    if (!std::isfinite(lr_am) || !std::isfinite(lr_pm) || !std::isfinite(tx_min))
        return fail(nullptr, DABGPU_E_INVALID, "dpd: learning rates and tx_min must be finite");
    if (min_count < 1) min_count = 1;
    const bool ref = basis == DABGPU_DPD_BASIS_REFERENCE;
    std::vector<double> t, r, p, wt;
    for (int b = 0; b < st->n_bins; ++b) {
        if (st->count[b] < min_count) {
            if (ref) break;                                            // (the leading run of bins)
            continue;
        }
        const double n = (double)st->count[b];
        double tb = st->sum_tx[b] / n, rb = st->sum_rx[b] / n, pb = st->sum_phase[b] / n;
        if (ref) {
            // Model_Poly's inputs are float32 arrays; tx is the bin centre, the phase is zero below tx_min
            tb = (double)(float)(((double)b + 0.5) * (double)st->peak / (double)st->n_bins);
            rb = (double)(float)rb;
            pb = tb < tx_min ? 0.0 : (double)(float)pb;
        }
        if (!std::isfinite(tb) || !std::isfinite(rb) || !std::isfinite(pb))
            return fail(nullptr, DABGPU_E_INVALID, "dpd: the statistics are not finite");
        t.push_back(tb);
        r.push_back(rb);
        p.push_back(pb);
        wt.push_back(weighted ? std::sqrt(n) : 1.0);
    }
    const int m = (int)t.size();
    if (m < 6) return fail(nullptr, DABGPU_E_INVALID, "dpd: fewer than six usable bins (n >= min_count)");
    // abscissae: AM/AM in r either way; AM/PM in r (MAGSQ) or in the bin centre (REFERENCE)
    const std::vector<double> &xa = r, &xp = ref ? t : r;
    double sa = 0.0, sp = 0.0;
    for (int i = 0; i < m; ++i) {
        sa = std::max(sa, std::fabs(xa[i]));
        sp = std::max(sp, std::fabs(xp[i]));
    }
    if (!(sa > 0.0) || !(sp > 0.0)) return fail(nullptr, DABGPU_E_INVALID, "dpd: every usable bin has amplitude zero");
    // powers: 2i + 1 and 2i of r in float64 (MAGSQ); i + 1 of rx and i of tx, each rounded to fp32 (REFERENCE: Model_Poly forms
    // `sig ** i` on float32 arrays -- the correctly rounded fp32 power is what numpy's scalar float32 power gives)
    auto power = [&](double x, int e) { return ref ? (double)(float)std::pow(x, e) : std::pow(x, e); };
    std::vector<double> A((size_t)m * 5), Bm((size_t)m * 5), ba(m), bp(m);
    int ea[5], ep[5];
    for (int i = 0; i < 5; ++i) {
        ea[i] = ref ? i + 1 : 2 * i + 1;
        ep[i] = ref ? i : 2 * i;
        for (int k = 0; k < m; ++k) {
            A[(size_t)i * m + k] = wt[k] * power(xa[k], ea[i]) / std::pow(sa, ea[i]);
            Bm[(size_t)i * m + k] = wt[k] * power(xp[k], ep[i]) / std::pow(sp, ep[i]);
        }
    }
    for (int k = 0; k < m; ++k) {
        ba[k] = wt[k] * t[k];
        bp[k] = wt[k] * p[k];
    }
    double ca[5], cp[5];
    dabgpu_dpd_fit_info fi{};
    fi.bins_used = m;
    if (!solve5(A, ba, m, ca, &fi.cond_am, &fi.resid_am) || !solve5(Bm, bp, m, cp, &fi.cond_pm, &fi.resid_pm))
        return fail(nullptr, DABGPU_E_INVALID, "dpd: the fit is singular (the usable bins do not span five powers)");
    for (int i = 0; i < 5; ++i) {
        const double fa = ca[i] / std::pow(sa, ea[i]), fp = cp[i] / std::pow(sp, ep[i]);
        const double pa = prev_am ? (double)prev_am[i] : (i == 0 ? 1.0 : 0.0), pp = prev_pm ? (double)prev_pm[i] : 0.0;
        am[i] = (float)(pa + lr_am * (fa - pa));
        pm[i] = (float)(pp + lr_pm * (fp - pp));
        if (!std::isfinite(am[i]) || !std::isfinite(pm[i])) return fail(nullptr, DABGPU_E_INVALID, "dpd: the fit is not finite");
    }
    if (info) *info = fi;
    return DABGPU_OK;
}

}  // extern "C"
