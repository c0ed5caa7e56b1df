// api_tii_scan.hip -- the TII analyser of tii_scan.hip behind the C-ABI: which (comb, pattern) the null symbols of whole
// transmission frames carry, how strong each comb is and when it arrives (dabgpu_tii_scan / _dev, dabgpu_get_tii_scan).  The
// reference has no receiver: nothing here replaces a plugin of its flowgraph, which is why no entry is named *_process.
#include "dabgpu_ctx.h"

using namespace dabgpu;
using namespace dabgpu_api;

static_assert(sizeof(dabgpu_tii_scan_head) == sizeof(TiiScanHead) && offsetof(dabgpu_tii_scan_head, total) == offsetof(TiiScanHead, total),
              "the device writes the public head");
static_assert(sizeof(dabgpu_tii_entry) == sizeof(TiiEntry) && offsetof(dabgpu_tii_entry, runner_up) == offsetof(TiiEntry, runner_up),
              "the device writes the public entries");

namespace {
constexpr size_t kHeadBytes = sizeof(TiiScanHead);
constexpr size_t kResultBytes = kHeadBytes + kTiiCombs * sizeof(TiiEntry);          // head, then 24 entry slots
constexpr size_t kStateBytes = kResultBytes + kTiiCombs * sizeof(int);              // and the entries' grid centres
static_assert(kHeadBytes == 40 && kResultBytes == 1192, "fixed layout of the result bytes");

// the refusals that need no context (dabgpu_tii_scan_check); max_frames 0: not known; nullptr = fine
const char *settings_refusal(const Geometry &g, size_t n_frames, size_t max_frames, const dabgpu_tii_scan_config *cfg)
{
    if (g.mode != 1 && g.mode != 2) return "tii_scan: only transmission modes I and II carry TII";
    if (!cfg) return "null argument";
    if (n_frames < 2 || (max_frames && n_frames > max_frames)) return "tii_scan: n_frames must lie in 2 ... max_frames";
    if (cfg->early < 0 || cfg->early > g.null_size - g.N) return "tii_scan: early must lie in 0 ... null_size - spacing";
    if (!std::isfinite(cfg->min_ratio) || cfg->min_ratio < 1.0f) return "tii_scan: min_ratio must be finite and at least 1";
    if (!(cfg->min_rel >= 0.0f && cfg->min_rel < 1.0f)) return "tii_scan: min_rel must lie in [0, 1)";
    return nullptr;
}

int check_scan(dabgpu_ctx *c, const void *frames, int format, size_t n_frames, const dabgpu_tii_scan_config *cfg, bool device)
{
    if (const char *why = settings_refusal(c->g, n_frames, (size_t)c->max_frames, cfg)) return fail(c, DABGPU_E_INVALID, why);
    return check_capture(c, "tii_scan", frames, format, device);
}
}  // namespace

extern "C" {
int dabgpu_tii_scan_dev(dabgpu_ctx *c, const void *d_frames, int format, size_t n_frames, const dabgpu_tii_scan_config *cfg,
                        void *stream)
{
    CTXCHK(c);
    int rc = check_scan(c, d_frames, format, n_frames, cfg, true);
    if (rc) return rc;
    if ((rc = apply_settings(c))) return rc;
    DevCall call(c, stream);
    if (call.rc) return call.rc;
    HIPCHK(c, c->tii_scan.result.reserve(kStateBytes));
    HIPCHK(c, c->tii_scan.rows.reserve(n_frames * 3 * kTiiCells * sizeof(double)));
    HIPCHK(c, c->tii_scan.bins.reserve(n_frames * (size_t)c->g.K * sizeof(float2)));
    c->tii_scan.done = false;                                         // (a failed launch leaves no result behind)
    HIPCHK(c, hipMemsetAsync(c->tii_scan.result.p, 0, kStateBytes, call.s));
    TiiScanArgs a{};
    a.g = c->g;
    a.t = tables_of(c);
    a.iq = d_frames;
    a.fmt = format;
    a.n_frames = (int)n_frames;
    a.early = cfg->early;
    a.old_variant = cfg->old_variant ? 1 : 0;
    a.min_ratio = cfg->min_ratio;
    a.min_rel = cfg->min_rel;
    a.rows = (double *)c->tii_scan.rows.p;
    a.bins = (float2 *)c->tii_scan.bins.p;
    a.head = (TiiScanHead *)c->tii_scan.result.p;
    a.entries = (TiiEntry *)((char *)c->tii_scan.result.p + kHeadBytes);
    a.centre = (int *)((char *)c->tii_scan.result.p + kResultBytes);
    HIPCHK(c, launch_tii_scan(a, call.s));
    c->tii_scan.done = true;
    c->tii_scan.stream = call.s;
    return DABGPU_OK;
}

int dabgpu_tii_scan(dabgpu_ctx *c, const void *frames, int format, size_t n_frames, const dabgpu_tii_scan_config *cfg)
{
    CTXCHK(c);
    if (int rc = check_scan(c, frames, format, n_frames, cfg, false)) return rc;
    return capture_from_host(c, c->tii_scan.in, frames, n_frames * tf_samples(c->g) * sample_bytes(format),
                             [&](const void *d_frames) { return dabgpu_tii_scan_dev(c, d_frames, format, n_frames, cfg, c->stream); });
}

int dabgpu_get_tii_scan(dabgpu_ctx *c, dabgpu_tii_scan_head *head, dabgpu_tii_entry *out, size_t cap)
{
    CTXCHK(c);
    if (!head || (cap && !out)) return fail(c, DABGPU_E_INVALID, "null argument");
    if (!c->tii_scan.done) return fail(c, DABGPU_E_INVALID, "no TII scan result (no dabgpu_tii_scan* call yet)");
    HIPCHK(c, wait_result(c, c->tii_scan.stream));
    HIPCHK(c, hipMemcpy(head, c->tii_scan.result.p, kHeadBytes, hipMemcpyDeviceToHost));
    const size_t m = std::min<size_t>(cap, kTiiCombs);                // (whole slots: zeros behind n_entries)
    if (m) HIPCHK(c, hipMemcpy(out, (const char *)c->tii_scan.result.p + kHeadBytes, m * sizeof(TiiEntry), hipMemcpyDeviceToHost));
    return DABGPU_OK;
}

int dabgpu_tii_scan_check(int mode, size_t n_frames, const dabgpu_tii_scan_config *cfg)
{
    Geometry g;
    if (!mode_geometry(mode, &g)) return fail(nullptr, DABGPU_E_INVALID, "tii_scan: transmission mode not valid");
    if (const char *why = settings_refusal(g, n_frames, 0, cfg)) return fail(nullptr, DABGPU_E_INVALID, why);
    return DABGPU_OK;
}

}  // extern "C"
