// api_clock.hip -- the clock's resampler of clock.hip behind the C-ABI: a sampling-clock offset put on a sample stream or, with
// the opposite sign, taken off it (dabgpu_set_clock, dabgpu_clock / _dev), the stream's history and position
// (dabgpu_clock_reset, dabgpu_get_clock_position) and what needs neither context nor device: the setting's check, the step, the
// output counts, the tap table and the setting that undoes another.  The reference has no such stage: nothing here replaces a
// plugin of its flowgraph, which is why no entry is named *_process.
#include "dabgpu_ctx.h"

using namespace dabgpu;
using namespace dabgpu_api;

static_assert(DABGPU_CLOCK_TAPS == kClkTaps && DABGPU_CLOCK_PHASES == kClkPhases && DABGPU_CLOCK_HISTORY == kClkHist,
              "the header's figures are the kernel's");

namespace {
constexpr StreamRules kRules{"clock", "n_in", "outputs", nullptr, 1ULL << 62, "clock: the stream's position must not exceed 2^62"};

const char *ppm_refusal(double ppm)
{
    if (!std::isfinite(ppm)) return "clock: ppm must be finite";
    if (std::fabs(ppm) > 1000.0) return "clock: |ppm| must not exceed 1000";
    return nullptr;
}

long long step_of(double ppm) { return std::llrint(ppm * 1e-6 * 18446744073709551616.0); }

// M(T): the outputs m >= 0 whose last tap, input i_m + 16, lies in front of input T.  i_m = floor(m W / 2^64) with
// W = 2^64 + step, so i_m <= T - 17 exactly when m < (T - 16) 2^64 / W
unsigned long long count_of(long long step, unsigned long long T)
{
    if (T <= 16) return 0;
    const unsigned __int128 w = (unsigned __int128)(((__int128)1 << 64) + step);
    const unsigned __int128 a = (unsigned __int128)(T - 16) << 64;
    return (unsigned long long)((a + w - 1) / w);
}

// row p of the table: dabgpu_dpd_delay_taps at p / 512; row 512, where that formula stops, is row 0 one tap later
void phase_taps(int p, float taps[kClkTaps])
{
    if (p < kClkPhases) {
        dabgpu_dpd_delay_taps((double)p / kClkPhases, taps);
        return;
    }
    for (int j = 0; j < kClkTaps; ++j) taps[j] = j == kClkCentre + 1 ? 1.f : 0.f;
}

int check_call(dabgpu_ctx *c, const void *in, int in_format, size_t n_in, const void *out, int out_format, size_t out_cap,
               size_t *n_out, unsigned long long *count)
{
    if (!c->clock.configured) return fail(c, DABGPU_E_INVALID, "clock: no setting (no dabgpu_set_clock call yet)");
    if ((in_format != 0 && in_format != DABGPU_FMT_S16) || (out_format != 0 && out_format != DABGPU_FMT_S16))
        return fail(c, DABGPU_E_INVALID, "clock: formats are complexf (0) or DABGPU_FMT_S16");
    // (unsigned arithmetic on any n_in: a count the checks below refuse is never used)
    *count = count_of(c->clock.step, c->clock.position + n_in) - count_of(c->clock.step, c->clock.position);
    return check_stream_call(c, c->clock, kRules, in, in_format, n_in, out, out_format, *count, out_cap, n_out);
}
const char *const kScoEarlyRange = "sco: early must lie inside the cyclic prefix (0 ... sym_size - spacing)";

int check_sco(dabgpu_ctx *c, const void *iq, int format, size_t n_frames, int early, bool device)
{
    if (int rc = check_capture_format(c, "sco", format)) return rc;
    if (early < 0 || early > c->g.sym_size - c->g.N) return fail(c, DABGPU_E_INVALID, kScoEarlyRange);
    if (n_frames == 0) return fail(c, DABGPU_E_INVALID, "sco: n_frames must not be 0");
    if (n_frames > (size_t)c->max_frames) return fail(c, DABGPU_E_CAPACITY, "n_frames exceeds max_frames of the context");
    if (!iq) return fail(c, DABGPU_E_INVALID, "null argument");
    if (device && !sample_aligned(iq, format)) return fail_misaligned(c, "sco");
    return DABGPU_OK;
}

// the derived figures of a set of sums (include/dabgpu.h: ppm, residual_cfo, quality, valid)
void sco_derive(const Geometry &g, const double *sum, dabgpu_sco_frame *out)
{
    std::memset(out, 0, sizeof *out);
    out->a_hi_re = sum[0];
    out->a_hi_im = sum[1];
    out->a_lo_re = sum[2];
    out->a_lo_im = sum[3];
    out->s = sum[4];
    if (!(sum[4] > 0.0)) return;
    const double turn = 2.0 * M_PI * (double)g.sym_size / (double)g.N;
    const double cr = sum[0] * sum[2] + sum[1] * sum[3], ci = sum[1] * sum[2] - sum[0] * sum[3];      // A_hi conj(A_lo)
    const double tr = sum[0] + sum[2], ti = sum[1] + sum[3];
    out->ppm = 1e6 * std::atan2(ci, cr) / (turn * (double)(g.K / 2 + 1));
    out->residual_cfo = std::atan2(ti, tr) / turn;
    out->quality = std::hypot(tr, ti) / sum[4];
    out->valid = 1;
}
}  // namespace

extern "C" {
int dabgpu_clock_check(double ppm)
{
    if (const char *why = ppm_refusal(ppm)) return fail(nullptr, DABGPU_E_INVALID, why);
    return DABGPU_OK;
}

int dabgpu_clock_step(double ppm, int64_t *step)
{
    if (!step) return fail(nullptr, DABGPU_E_INVALID, "null argument");
    if (const char *why = ppm_refusal(ppm)) return fail(nullptr, DABGPU_E_INVALID, why);
    *step = step_of(ppm);
    return DABGPU_OK;
}

int dabgpu_clock_count(double ppm, uint64_t T, uint64_t *M)
{
    if (!M) return fail(nullptr, DABGPU_E_INVALID, "null argument");
    if (const char *why = ppm_refusal(ppm)) return fail(nullptr, DABGPU_E_INVALID, why);
    if (T > kRules.max_position) return fail(nullptr, DABGPU_E_INVALID, kRules.bad_position);
    *M = count_of(step_of(ppm), T);
    return DABGPU_OK;
}

size_t dabgpu_clock_out_max(size_t n_in) { return n_in + n_in / 999 + 2; }

int dabgpu_clock_phase_taps(int p, float taps[32])
{
    if (!taps) return fail(nullptr, DABGPU_E_INVALID, "null argument");
    if (p < 0 || p > kClkPhases) return fail(nullptr, DABGPU_E_INVALID, "clock: the table's rows are 0 ... 512");
    phase_taps(p, taps);
    return DABGPU_OK;
}

double dabgpu_clock_inverse_ppm(double ppm) { return -ppm / (1.0 + ppm * 1e-6); }

int dabgpu_set_clock(dabgpu_ctx *c, double ppm)
{
    CTXCHK(c);
    if (const char *why = ppm_refusal(ppm)) return fail(c, DABGPU_E_INVALID, why);
    if (!c->clock.tab.p) {
        // (T[p][j], T[p + 1][j] - T[p][j]), the difference an fp32 subtraction: what the kernel blends from in one load
        std::vector<float> t((size_t)(kClkPhases + 1) * kClkTaps), pairs((size_t)kClkPhases * kClkTaps * 2);
        for (int p = 0; p <= kClkPhases; ++p) phase_taps(p, &t[(size_t)p * kClkTaps]);
        for (size_t i = 0; i < (size_t)kClkPhases * kClkTaps; ++i) {
            volatile float d = t[i + kClkTaps] - t[i];
            pairs[2 * i] = t[i];
            pairs[2 * i + 1] = d;
        }
        HIPCHK(c, upload(c->clock.tab, pairs, c->stream));
    }
    c->clock.step = step_of(ppm);
    c->clock.configured = true;
    c->clock.zero_pending = true;
    c->clock.position = 0;
    return DABGPU_OK;
}

int dabgpu_clock_reset(dabgpu_ctx *c, uint64_t position)
{
    CTXCHK(c);
    return stream_reset(c, c->clock, kRules, position);
}

int dabgpu_get_clock_position(dabgpu_ctx *c, uint64_t *position)
{
    CTXCHK(c);
    return stream_position(c, c->clock, position);
}

int dabgpu_debug_clock_run_samples(dabgpu_ctx *c, int samples)
{
    CTXCHK(c);
    return stream_run_samples(c, c->clock, kRules, samples);
}

int dabgpu_clock_dev(dabgpu_ctx *c, const void *d_in, int in_format, size_t n_in, void *d_out, int out_format, size_t out_cap,
                     size_t *n_out, void *stream)
{
    CTXCHK(c);
    unsigned long long count = 0;
    int rc = check_call(c, d_in, in_format, n_in, d_out, out_format, out_cap, n_out, &count);
    if (rc) return rc;
    DevCall call(c, stream);
    if (call.rc) return call.rc;
    StreamHistory h;
    if ((rc = h.begin(c, c->clock, kClkHist, call.s))) return rc;
    if (count) {
        ClockArgs a{};
        a.in = d_in;
        a.out = d_out;
        a.hist = h.cur;
        a.tab = (const float2 *)c->clock.tab.p;
        a.n = (long long)n_in;
        a.T = c->clock.position;
        a.m0 = count_of(c->clock.step, c->clock.position);
        a.count = (long long)count;
        a.step = c->clock.step;
        a.in_fmt = in_format ? 1 : 0;
        a.out_fmt = out_format ? 1 : 0;
        a.run = clock_run((size_t)count, c->clock.run_samples);
        HIPCHK(c, launch_clock(a, call.s));
    }
    if ((rc = h.end(c, c->clock, d_in, in_format, n_in, kClkHist, call.s))) return rc;
    *n_out = (size_t)count;
    return DABGPU_OK;
}

int dabgpu_clock(dabgpu_ctx *c, const void *in, int in_format, size_t n_in, void *out, int out_format, size_t out_cap, size_t *n_out)
{
    CTXCHK(c);
    unsigned long long count = 0;
    int rc = check_call(c, in, in_format, n_in, out, out_format, out_cap, n_out, &count);
    if (rc) return rc;
    return stream_from_host(c, c->clock, in, n_in * sample_bytes(in_format), out, (size_t)count * sample_bytes(out_format),
                            [&](const void *d_in, void *d_out) {
                                return dabgpu_clock_dev(c, d_in, in_format, n_in, d_out, out_format, (size_t)count, n_out, c->stream);
                            });
}

int dabgpu_sco_dev(dabgpu_ctx *c, const void *d_iq, int format, size_t n_frames, int early, void *stream)
{
    CTXCHK(c);
    int rc = apply_settings(c);
    if (rc) return rc;
    if ((rc = check_sco(c, d_iq, format, n_frames, early, true))) return rc;
    DevCall call(c, stream);
    if (call.rc) return call.rc;
    const size_t nblocks = (size_t)c->g.nb_symbols - 1;
    HIPCHK(c, c->sco.rows.reserve(n_frames * nblocks * kScoSums * sizeof(double)));
    HIPCHK(c, c->sco.sums.reserve((size_t)c->max_frames * kScoSums * sizeof(double)));
    ScoArgs a{};
    fill_rx_symbols(c, d_iq, format, n_frames, early, a);
    a.rows = (double *)c->sco.rows.p;
    a.frames = (double *)c->sco.sums.p;
    HIPCHK(c, launch_sco(a, call.s));
    c->sco.frames = n_frames;
    c->sco.stream = call.s;
    return DABGPU_OK;
}

int dabgpu_sco(dabgpu_ctx *c, const void *iq, int format, size_t n_frames, int early)
{
    CTXCHK(c);
    if (int rc = check_sco(c, iq, format, n_frames, early, false)) return rc;
    return capture_from_host(c, c->sco.in, iq, n_frames * tf_samples(c->g) * sample_bytes(format),
                             [&](const void *d) { return dabgpu_sco_dev(c, d, format, n_frames, early, c->stream); });
}

int dabgpu_get_sco(dabgpu_ctx *c, int frame, dabgpu_sco_frame *out)
{
    CTXCHK(c);
    if (!out) return fail(c, DABGPU_E_INVALID, "null argument");
    if (frame < -1 || (frame >= 0 && (size_t)frame >= c->sco.frames) || c->sco.frames == 0)
        return fail(c, DABGPU_E_INVALID, "no clock estimate for this frame (no call yet, or frame index out of range)");
    HIPCHK(c, wait_result(c, c->sco.stream));
    std::vector<double> sums(c->sco.frames * kScoSums);
    HIPCHK(c, hipMemcpy(sums.data(), c->sco.sums.p, sums.size() * sizeof(double), hipMemcpyDeviceToHost));
    if (frame >= 0) {
        sco_derive(c->g, &sums[(size_t)frame * kScoSums], out);
        return DABGPU_OK;
    }
    // every valid frame's sums, in frame order
    double total[kScoSums] = {0., 0., 0., 0., 0.};
    for (size_t f = 0; f < c->sco.frames; ++f) {
        if (!(sums[f * kScoSums + 4] > 0.0)) continue;
        for (int i = 0; i < kScoSums; ++i) total[i] += sums[f * kScoSums + i];
    }
    sco_derive(c->g, total, out);
    return DABGPU_OK;
}

}  // extern "C"
