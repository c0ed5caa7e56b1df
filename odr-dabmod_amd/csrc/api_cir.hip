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
    if (format != 0 && format != DABGPU_FMT_S16)
        return fail(c, DABGPU_E_INVALID, "cir: input format is complexf (0) or DABGPU_FMT_S16");
    if (!frames) return fail(c, DABGPU_E_INVALID, "null argument");
    if (device && ((uintptr_t)frames & (format ? 3u : 7u)))
        return fail(c, DABGPU_E_INVALID, "cir: buffers must be aligned to a sample (eight bytes complexf, four bytes s16)");
    return DABGPU_OK;
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
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    if (!stream && (rc = own_stream_joins_lanes(c))) return rc;       // (d_frames: a chain call's output on any lane)
    TraceScope trace(c->trace_enabled ? &c->last_variant : nullptr);
    const size_t N = (size_t)c->g.N;
    HIPCHK(c, c->d_cir.reserve(kResultBytes + 2 * N * sizeof(double)));
    HIPCHK(c, c->d_cir_rows.reserve((size_t)c->max_frames * 2 * N * sizeof(double)));
    c->cir_done = false;                                              // (a failed launch leaves no result behind)
    HIPCHK(c, hipMemsetAsync(c->d_cir.p, 0, kResultBytes, s));
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
    a.rows = (double *)c->d_cir_rows.p;
    a.head = (CirHead *)c->d_cir.p;
    a.paths = (CirPath *)((char *)c->d_cir.p + kHeadBytes);
    a.pdp = (double *)((char *)c->d_cir.p + kResultBytes);
    a.resp = a.pdp + N;
    HIPCHK(c, launch_cir(a, s));
    c->cir_done = true;
    c->cir_stream = s;
    return DABGPU_OK;
}

int dabgpu_cir(dabgpu_ctx *c, const void *frames, int format, size_t n_frames, const dabgpu_cir_config *cfg)
{
    CTXCHK(c);
    int rc = check_cir(c, frames, format, n_frames, cfg, false);
    if (rc) return rc;
    if ((rc = dabgpu_synchronize(c))) return rc;
    HostIO io(c);
    if ((rc = io.in(c->d_cir_in, frames, n_frames * tf_samples(c->g) * (format ? 4 : sizeof(float2))))) return rc;
    if ((rc = dabgpu_cir_dev(c, c->d_cir_in.p, format, n_frames, cfg, c->stream))) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return DABGPU_OK;
}

int dabgpu_get_cir(dabgpu_ctx *c, dabgpu_cir_head *head, dabgpu_cir_path *out, size_t cap)
{
    CTXCHK(c);
    if (!head || (cap && !out)) return fail(c, DABGPU_E_INVALID, "null argument");
    if (!c->cir_done) return fail(c, DABGPU_E_INVALID, "no channel estimate (no dabgpu_cir* call yet)");
    HIPCHK(c, hipStreamSynchronize(c->cir_stream ? c->cir_stream : c->stream));
    HIPCHK(c, hipMemcpy(head, c->d_cir.p, kHeadBytes, hipMemcpyDeviceToHost));
    const size_t m = std::min<size_t>(cap, kCirMaxPaths);             // (whole slots: zeros behind n_paths)
    if (m) HIPCHK(c, hipMemcpy(out, (const char *)c->d_cir.p + kHeadBytes, m * sizeof(CirPath), hipMemcpyDeviceToHost));
    return DABGPU_OK;
}

int dabgpu_get_cir_profile(dabgpu_ctx *c, double *pdp, double *resp)
{
    CTXCHK(c);
    if (!c->cir_done) return fail(c, DABGPU_E_INVALID, "no channel estimate (no dabgpu_cir* call yet)");
    HIPCHK(c, hipStreamSynchronize(c->cir_stream ? c->cir_stream : c->stream));
    const size_t bytes = (size_t)c->g.N * sizeof(double);
    if (pdp) HIPCHK(c, hipMemcpy(pdp, (const char *)c->d_cir.p + kResultBytes, bytes, hipMemcpyDeviceToHost));
    if (resp) HIPCHK(c, hipMemcpy(resp, (const char *)c->d_cir.p + kResultBytes + bytes, bytes, hipMemcpyDeviceToHost));
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
