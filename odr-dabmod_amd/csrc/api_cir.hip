// api_cir.hip -- the channel estimator of cir.hip behind the C-ABI: the impulse response the phase reference symbols of whole
// transmission frames went through, its echoes with level and delay, and the response on the carriers (dabgpu_cir / _dev,
// dabgpu_get_cir, dabgpu_get_cir_profile).  The reference has no receiver: nothing here replaces a plugin of its flowgraph,
// which is why no entry is named *_process.
#include "dabgpu_ctx.h"

using namespace dabgpu;
using namespace dabgpu_api;

static_assert(sizeof(dabgpu_cir_head) == sizeof(CirHead) && offsetof(dabgpu_cir_head, resp_max) == offsetof(CirHead, resp_max) &&
                  offsetof(dabgpu_cir_head, floor) == offsetof(CirHead, floor),
              "the device writes the public head");
static_assert(sizeof(dabgpu_cir_path) == sizeof(CirPath) && offsetof(dabgpu_cir_path, power) == offsetof(CirPath, power),
              "the device writes the public paths");
static_assert(DABGPU_CIR_MAX_PATHS == kCirMaxPaths, "path slots");

namespace {
constexpr size_t kHeadBytes = sizeof(CirHead);
constexpr size_t kResultBytes = kHeadBytes + kCirMaxPaths * sizeof(CirPath);        // head, then 16 path slots
static_assert(kHeadBytes == 128 && sizeof(CirPath) == 32 && kResultBytes == 640, "fixed layout of the result bytes");

// the refusals that need no context (dabgpu_cir_check); max_frames 0: not known; nullptr = fine
const char *settings_refusal(const Geometry &g, size_t n_frames, size_t max_frames, const dabgpu_cir_config *cfg)
{
    if (!cfg) return "null argument";
    if (n_frames < 1 || (max_frames && n_frames > max_frames)) return "cir: n_frames must lie in 1 ... max_frames";
    if (cfg->early < 0 || cfg->early > g.sym_size - g.N) return "cir: early must lie in 0 ... sym_size - spacing";
    if (cfg->window != 0 && cfg->window != 1) return "cir: window is 0 (rectangular) or 1 (Hann)";
    if (!std::isfinite(cfg->min_ratio) || cfg->min_ratio < 1.0f) return "cir: min_ratio must be finite and at least 1";
    if (!(cfg->min_rel >= 0.0f && cfg->min_rel < 1.0f)) return "cir: min_rel must lie in [0, 1)";
    return nullptr;
}

int check_cir(dabgpu_ctx *c, const void *frames, int format, size_t n_frames, const dabgpu_cir_config *cfg, bool device)
{
    if (const char *why = settings_refusal(c->g, n_frames, (size_t)c->max_frames, cfg)) return fail(c, DABGPU_E_INVALID, why);
    return check_capture(c, "cir", frames, format, device);
}

// S_w: the K weights in ascending carrier order, in float64
double weight_sum(int K, int window)
{
    double s = 0.0;
    for (int i = 0; i < K; ++i) s += window ? 0.5 - 0.5 * std::cos(2.0 * M_PI * ((double)i + 0.5) / (double)K) : 1.0;
    return s;
}
}  // namespace

extern "C" {
int dabgpu_cir_dev(dabgpu_ctx *c, const void *d_frames, int format, size_t n_frames, const dabgpu_cir_config *cfg, void *stream)
{
    CTXCHK(c);
    int rc = check_cir(c, d_frames, format, n_frames, cfg, true);
    if (rc) return rc;
    if ((rc = apply_settings(c))) return rc;
    DevCall call(c, stream);
    if (call.rc) return call.rc;
    const size_t N = (size_t)c->g.N;
    HIPCHK(c, c->cir.result.reserve(kResultBytes + 2 * N * sizeof(double)));
    HIPCHK(c, c->cir.rows.reserve((size_t)c->max_frames * 2 * N * sizeof(double)));
    c->cir.done = false;                                              // (a failed launch leaves no result behind)
    HIPCHK(c, hipMemsetAsync(c->cir.result.p, 0, kResultBytes, call.s));
    CirArgs a{};
    a.g = c->g;
    a.t = tables_of(c);
    a.iq = d_frames;
    a.fmt = format;
    a.n_frames = (int)n_frames;
    a.early = cfg->early;
    a.window = cfg->window;
    a.min_ratio = cfg->min_ratio;
    a.min_rel = cfg->min_rel;
    a.sum_w = weight_sum(c->g.K, cfg->window);
    a.rows = (double *)c->cir.rows.p;
    a.head = (CirHead *)c->cir.result.p;
    a.paths = (CirPath *)((char *)c->cir.result.p + kHeadBytes);
    a.pdp = (double *)((char *)c->cir.result.p + kResultBytes);
    a.resp = a.pdp + N;
    HIPCHK(c, launch_cir(a, call.s));
    c->cir.done = true;
    c->cir.stream = call.s;
    return DABGPU_OK;
}

int dabgpu_cir(dabgpu_ctx *c, const void *frames, int format, size_t n_frames, const dabgpu_cir_config *cfg)
{
    CTXCHK(c);
    if (int rc = check_cir(c, frames, format, n_frames, cfg, false)) return rc;
    return capture_from_host(c, c->cir.in, frames, n_frames * tf_samples(c->g) * sample_bytes(format),
                             [&](const void *d_frames) { return dabgpu_cir_dev(c, d_frames, format, n_frames, cfg, c->stream); });
}

int dabgpu_get_cir(dabgpu_ctx *c, dabgpu_cir_head *head, dabgpu_cir_path *out, size_t cap)
{
    CTXCHK(c);
    if (!head || (cap && !out)) return fail(c, DABGPU_E_INVALID, "null argument");
    if (!c->cir.done) return fail(c, DABGPU_E_INVALID, "no channel estimate (no dabgpu_cir* call yet)");
    HIPCHK(c, wait_result(c, c->cir.stream));
    HIPCHK(c, hipMemcpy(head, c->cir.result.p, kHeadBytes, hipMemcpyDeviceToHost));
    const size_t m = std::min<size_t>(cap, kCirMaxPaths);             // (whole slots: zeros behind n_paths)
    if (m) HIPCHK(c, hipMemcpy(out, (const char *)c->cir.result.p + kHeadBytes, m * sizeof(CirPath), hipMemcpyDeviceToHost));
    return DABGPU_OK;
}

int dabgpu_get_cir_profile(dabgpu_ctx *c, double *pdp, double *resp)
{
    CTXCHK(c);
    if (!c->cir.done) return fail(c, DABGPU_E_INVALID, "no channel estimate (no dabgpu_cir* call yet)");
    HIPCHK(c, wait_result(c, c->cir.stream));
    const size_t bytes = (size_t)c->g.N * sizeof(double);
    if (pdp) HIPCHK(c, hipMemcpy(pdp, (const char *)c->cir.result.p + kResultBytes, bytes, hipMemcpyDeviceToHost));
    if (resp) HIPCHK(c, hipMemcpy(resp, (const char *)c->cir.result.p + kResultBytes + bytes, bytes, hipMemcpyDeviceToHost));
    return DABGPU_OK;
}

int dabgpu_cir_check(int mode, size_t n_frames, const dabgpu_cir_config *cfg)
{
    Geometry g;
    if (!mode_geometry(mode, &g)) return fail(nullptr, DABGPU_E_INVALID, "cir: transmission mode not valid");
    if (const char *why = settings_refusal(g, n_frames, 0, cfg)) return fail(nullptr, DABGPU_E_INVALID, why);
    return DABGPU_OK;
}

}  // extern "C"
