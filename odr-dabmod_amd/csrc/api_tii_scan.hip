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
    if (format != 0 && format != DABGPU_FMT_S16)
        return fail(c, DABGPU_E_INVALID, "tii_scan: input format is complexf (0) or DABGPU_FMT_S16");
    if (!frames) return fail(c, DABGPU_E_INVALID, "null argument");
    if (device && ((uintptr_t)frames & (format ? 3u : 7u)))
        return fail(c, DABGPU_E_INVALID, "tii_scan: buffers must be aligned to a sample (eight bytes complexf, four bytes s16)");
    return DABGPU_OK;
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
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    if (!stream && (rc = own_stream_joins_lanes(c))) return rc;       // (d_frames: a chain call's output on any lane)
    TraceScope trace(c->trace_enabled ? &c->last_variant : nullptr);
    HIPCHK(c, c->d_tii_scan.reserve(kStateBytes));
    HIPCHK(c, c->d_tii_rows.reserve(n_frames * 3 * kTiiCells * sizeof(double)));
    HIPCHK(c, c->d_tii_bins.reserve(n_frames * (size_t)c->g.K * sizeof(float2)));
    c->tii_scan_done = false;                                         // (a failed launch leaves no result behind)
    HIPCHK(c, hipMemsetAsync(c->d_tii_scan.p, 0, kStateBytes, s));
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
    a.rows = (double *)c->d_tii_rows.p;
    a.bins = (float2 *)c->d_tii_bins.p;
    a.head = (TiiScanHead *)c->d_tii_scan.p;
    a.entries = (TiiEntry *)((char *)c->d_tii_scan.p + kHeadBytes);
    a.centre = (int *)((char *)c->d_tii_scan.p + kResultBytes);
    HIPCHK(c, launch_tii_scan(a, s));
    c->tii_scan_done = true;
    c->tii_scan_stream = s;
    return DABGPU_OK;
}

int dabgpu_tii_scan(dabgpu_ctx *c, const void *frames, int format, size_t n_frames, const dabgpu_tii_scan_config *cfg)
{
    CTXCHK(c);
    int rc = check_scan(c, frames, format, n_frames, cfg, false);
    if (rc) return rc;
    if ((rc = dabgpu_synchronize(c))) return rc;
    HostIO io(c);
    if ((rc = io.in(c->d_tii_in, frames, n_frames * tf_samples(c->g) * (format ? 4 : sizeof(float2))))) return rc;
    if ((rc = dabgpu_tii_scan_dev(c, c->d_tii_in.p, format, n_frames, cfg, c->stream))) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return DABGPU_OK;
}

int dabgpu_get_tii_scan(dabgpu_ctx *c, dabgpu_tii_scan_head *head, dabgpu_tii_entry *out, size_t cap)
{
    CTXCHK(c);
    if (!head || (cap && !out)) return fail(c, DABGPU_E_INVALID, "null argument");
    if (!c->tii_scan_done) return fail(c, DABGPU_E_INVALID, "no TII scan result (no dabgpu_tii_scan* call yet)");
    HIPCHK(c, hipStreamSynchronize(c->tii_scan_stream ? c->tii_scan_stream : c->stream));
    HIPCHK(c, hipMemcpy(head, c->d_tii_scan.p, kHeadBytes, hipMemcpyDeviceToHost));
    const size_t m = std::min<size_t>(cap, kTiiCombs);                // (whole slots: zeros behind n_entries)
    if (m) HIPCHK(c, hipMemcpy(out, (const char *)c->d_tii_scan.p + kHeadBytes, m * sizeof(TiiEntry), hipMemcpyDeviceToHost));
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
