// api_tuner.hip -- the tuner of tuner.hip behind the C-ABI: a capture at any accepted rate and offset mixed, channel-filtered
// and decimated to the native rate (dabgpu_set_tuner, dabgpu_tuner / _dev), the stream's history and position
// (dabgpu_tuner_reset, dabgpu_get_tuner_position) and what needs neither context nor device: the setting's check, the ratio,
// the tap rows and the output counts.  The reference has no such stage: nothing here replaces a plugin of its flowgraph, which
// is why no entry is named *_process.
#include "dabgpu_ctx.h"

#include <numeric>

using namespace dabgpu;
using namespace dabgpu_api;

static_assert(DABGPU_TUNER_MAX_L == kTunMaxL && DABGPU_TUNER_MAX_TAPS == kTunMaxTaps, "the header's figures are the kernel's");

namespace {
constexpr uint32_t kNative = 2048000;
constexpr StreamRules kRules{"tuner", "n_in", "outputs",
                             "tuner: buffers must be aligned to a sample (eight bytes complexf, four bytes s16, two bytes u8 / s8)",
                             1ULL << 50, "tuner: the stream's position must not exceed 2^50"};

struct Ratio {
    int L, M, P;
    double c;                             // the filter's cutoff as a share of the input's Nyquist band
    long long step;
};

// the setting's refusal (nullptr: accepted, *r filled in)
const char *resolve(const dabgpu_tuner_config *cfg, Ratio *r)
{
    if (!cfg) return "null argument";
    if (cfg->in_rate_hz < kNative) return "tuner: in_rate_hz must not be below 2048000";
    const uint32_t g = std::gcd(kNative, cfg->in_rate_hz);
    const uint32_t L = kNative / g, M = cfg->in_rate_hz / g;
    if (L > (uint32_t)kTunMaxL) return "tuner: in_rate_hz / 2048000 = M / L in lowest terms needs L <= 512 (L too large)";
    if (M > 8 * L) return "tuner: in_rate_hz must not exceed 8 x 2048000 (M <= 8 L)";
    if (cfg->selectivity != 0 && cfg->selectivity != 1) return "tuner: selectivity is 0 (wide) or 1 (channel)";
    if (!std::isfinite(cfg->offset_hz)) return "tuner: offset_hz must be finite";
    if (!(std::fabs(cfg->offset_hz) < (double)cfg->in_rate_hz / 4.0)) return "tuner: |offset_hz| must be below in_rate_hz / 4";
    const int D = (int)((M + L - 1) / L);
    r->L = (int)L;
    r->M = (int)M;
    r->P = (cfg->selectivity ? 96 : 32) * D;
    r->c = std::min(1.0, (cfg->selectivity ? 1712000.0 : 2048000.0) / (double)cfg->in_rate_hz);
    r->step = std::llrint(-cfg->offset_hz / (double)cfg->in_rate_hz * 18446744073709551616.0);
    return nullptr;
}

double bessel_i0(double x)
{
    double term = 1.0, sum = 1.0;
    for (int k = 1; k < 256; ++k) {
        term *= (x / (2.0 * (double)k)) * (x / (2.0 * (double)k));
        sum += term;
        if (term < 1e-18 * sum) break;
    }
    return sum;
}

// 1 at 0, exactly 0 at every other integer
double sinc_exact(double x)
{
    if (x == 0.0) return 1.0;
    const double n = std::nearbyint(x);
    double s = std::sin(M_PI * (x - n));
    if (std::fmod(n, 2.0) != 0.0) s = -s;
    return s / (M_PI * x);
}

// row p of the table (include/dabgpu.h, "Taps")
void tap_row(const Ratio &r, int p, float *taps)
{
    const double half = (double)(r.P / 2), i0b = bessel_i0(10.0);
    std::vector<double> h((size_t)r.P);
    double sum = 0.0;
    for (int j = 0; j < r.P; ++j) {
        const double t = (double)(j - (r.P / 2 - 1)) - (double)p / (double)r.L;
        const double u = t / half;
        h[(size_t)j] = std::fabs(t) <= half ? r.c * sinc_exact(r.c * t) * bessel_i0(10.0 * std::sqrt(std::max(0.0, 1.0 - u * u))) / i0b : 0.0;
        sum += h[(size_t)j];
    }
    for (int j = 0; j < r.P; ++j) taps[j] = (float)(h[(size_t)j] / sum + 0.0);
}

// M(T): the outputs m >= 0 whose last tap, input i_m + P/2, lies in front of input T.  i_m = floor(m M / L) <= T - 1 - P/2
// exactly when m < (T - P/2) L / M
unsigned long long count_of(const Ratio &r, unsigned long long T)
{
    const unsigned long long half = (unsigned long long)(r.P / 2);
    if (T <= half) return 0;
    return ((T - half) * (unsigned long long)r.L + (unsigned long long)r.M - 1) / (unsigned long long)r.M;
}

int check_call(dabgpu_ctx *c, const void *in, int in_format, size_t n_in, const void *out, int out_format, size_t out_cap,
               size_t *n_out, unsigned long long *count)
{
    const TunerState &t = c->tuner;
    if (!t.configured) return fail(c, DABGPU_E_INVALID, "tuner: no setting (no dabgpu_set_tuner call yet)");
    if (in_format != 0 && in_format != DABGPU_FMT_S16 && in_format != DABGPU_FMT_U8 && in_format != DABGPU_FMT_S8)
        return fail(c, DABGPU_E_INVALID, "tuner: input format is complexf (0), DABGPU_FMT_S16, DABGPU_FMT_U8 or DABGPU_FMT_S8");
    if (out_format != 0 && out_format != DABGPU_FMT_S16)
        return fail(c, DABGPU_E_INVALID, "tuner: output format is complexf (0) or DABGPU_FMT_S16");
    // (unsigned arithmetic on any n_in: a count the checks below refuse is never used)
    const Ratio r{t.L, t.M, t.P, 0.0, 0};
    *count = count_of(r, t.position + n_in) - count_of(r, t.position);
    return check_stream_call(c, t, kRules, in, in_format, n_in, out, out_format, *count, out_cap, n_out);
}
}  // namespace

extern "C" {
int dabgpu_tuner_check(const dabgpu_tuner_config *cfg)
{
    Ratio r;
    if (const char *why = resolve(cfg, &r)) return fail(nullptr, DABGPU_E_INVALID, why);
    return DABGPU_OK;
}

int dabgpu_tuner_geometry(const dabgpu_tuner_config *cfg, int *L, int *M, int *P)
{
    Ratio r;
    if (!L || !M || !P) return fail(nullptr, DABGPU_E_INVALID, "null argument");
    if (const char *why = resolve(cfg, &r)) return fail(nullptr, DABGPU_E_INVALID, why);
    *L = r.L;
    *M = r.M;
    *P = r.P;
    return DABGPU_OK;
}

int dabgpu_tuner_taps(const dabgpu_tuner_config *cfg, int p, float *taps)
{
    Ratio r;
    if (!taps) return fail(nullptr, DABGPU_E_INVALID, "null argument");
    if (const char *why = resolve(cfg, &r)) return fail(nullptr, DABGPU_E_INVALID, why);
    if (p < 0 || p >= r.L) return fail(nullptr, DABGPU_E_INVALID, "tuner: the table's rows are 0 ... L - 1");
    tap_row(r, p, taps);
    return DABGPU_OK;
}

int dabgpu_tuner_count(const dabgpu_tuner_config *cfg, uint64_t T, uint64_t *M_out)
{
    Ratio r;
    if (!M_out) return fail(nullptr, DABGPU_E_INVALID, "null argument");
    if (const char *why = resolve(cfg, &r)) return fail(nullptr, DABGPU_E_INVALID, why);
    if (T > kRules.max_position) return fail(nullptr, DABGPU_E_INVALID, kRules.bad_position);
    *M_out = count_of(r, T);
    return DABGPU_OK;
}

size_t dabgpu_tuner_out_max(const dabgpu_tuner_config *cfg, size_t n_in)
{
    Ratio r;
    if (resolve(cfg, &r)) return 0;
    const unsigned __int128 up = ((unsigned __int128)n_in * (unsigned)r.L + (unsigned)r.M - 1) / (unsigned)r.M;
    return (size_t)up + 1;
}

int dabgpu_set_tuner(dabgpu_ctx *c, const dabgpu_tuner_config *cfg)
{
    CTXCHK(c);
    Ratio r;
    if (const char *why = resolve(cfg, &r)) return fail(c, DABGPU_E_INVALID, why);
    TunerState &t = c->tuner;
    if (!t.tab.p || t.tab_rate != cfg->in_rate_hz || t.tab_selectivity != cfg->selectivity) {
        std::vector<float> tab((size_t)r.L * (size_t)r.P);
        for (int p = 0; p < r.L; ++p) tap_row(r, p, &tab[(size_t)p * (size_t)r.P]);
        HIPCHK(c, wait_result(c, t.stream));                            // (a queued call may still read the table in place)
        t.tab_rate = 0;
        t.tab_selectivity = -1;
        t.configured = false;
        HIPCHK(c, upload(t.tab, tab, c->stream));
        t.tab_rate = cfg->in_rate_hz;
        t.tab_selectivity = cfg->selectivity;
    }
    t.cfg = *cfg;
    t.L = r.L;
    t.M = r.M;
    t.P = r.P;
    t.step = (unsigned long long)r.step;
    t.configured = true;
    t.zero_pending = true;
    t.position = 0;
    return DABGPU_OK;
}

int dabgpu_tuner_reset(dabgpu_ctx *c, uint64_t position)
{
    CTXCHK(c);
    return stream_reset(c, c->tuner, kRules, position);
}

int dabgpu_get_tuner_position(dabgpu_ctx *c, uint64_t *position)
{
    CTXCHK(c);
    return stream_position(c, c->tuner, position);
}

int dabgpu_debug_tuner_run_samples(dabgpu_ctx *c, int samples)
{
    CTXCHK(c);
    return stream_run_samples(c, c->tuner, kRules, samples);
}

int dabgpu_tuner_dev(dabgpu_ctx *c, const void *d_in, int in_format, size_t n_in, void *d_out, int out_format, size_t out_cap,
                     size_t *n_out, void *stream)
{
    CTXCHK(c);
    unsigned long long count = 0;
    int rc = check_call(c, d_in, in_format, n_in, d_out, out_format, out_cap, n_out, &count);
    if (rc) return rc;
    DevCall call(c, stream);
    if (call.rc) return call.rc;
    TunerState &t = c->tuner;
    StreamHistory h;
    if ((rc = h.begin(c, t, kTunMaxHist, call.s))) return rc;
    if (count) {
        const Ratio r{t.L, t.M, t.P, 0.0, 0};
        TunerArgs a{};
        a.in = d_in;
        a.out = d_out;
        a.hist = h.cur;
        a.tab = (const float *)t.tab.p;
        a.n = (long long)n_in;
        a.T = t.position;
        a.m0 = count_of(r, t.position);
        a.count = (long long)count;
        a.step = t.step;
        a.L = t.L;
        a.M = t.M;
        a.P = t.P;
        a.in_fmt = in_format;                                           // (DABGPU_FMT_S16, _U8, _S8 are 1, 2, 3)
        a.out_fmt = out_format ? 1 : 0;
        a.run = tuner_run(t.L, t.M, t.P, t.run_samples);
        HIPCHK(c, launch_tuner(a, call.s));
    }
    if ((rc = h.end(c, t, d_in, in_format, n_in, t.P - 1, call.s))) return rc;
    *n_out = (size_t)count;
    return DABGPU_OK;
}

int dabgpu_tuner(dabgpu_ctx *c, const void *in, int in_format, size_t n_in, void *out, int out_format, size_t out_cap, size_t *n_out)
{
    CTXCHK(c);
    unsigned long long count = 0;
    int rc = check_call(c, in, in_format, n_in, out, out_format, out_cap, n_out, &count);
    if (rc) return rc;
    return stream_from_host(c, c->tuner, in, n_in * sample_bytes(in_format), out, (size_t)count * sample_bytes(out_format),
                            [&](const void *d_in, void *d_out) {
                                return dabgpu_tuner_dev(c, d_in, in_format, n_in, d_out, out_format, (size_t)count, n_out, c->stream);
                            });
}

}  // extern "C"
