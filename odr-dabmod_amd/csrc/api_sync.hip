// api_sync.hip -- the synchroniser of sync.hip behind the C-ABI: where the transmission frames of a native-rate capture start
// and how far off the carrier it sits (dabgpu_sync / _dev, dabgpu_get_sync_result), and the frames rotated back and cut out as
// dabgpu_demod* takes them (dabgpu_sync_extract / _dev).  The reference has no receiver: nothing here replaces a plugin of its
// flowgraph, which is why no entry is named *_process.
#include "dabgpu_ctx.h"

using namespace dabgpu;
using namespace dabgpu_api;

static_assert(sizeof(dabgpu_sync_frame) == sizeof(SyncFrame) && offsetof(dabgpu_sync_frame, null_depth) == offsetof(SyncFrame, null_depth),
              "the device writes the public record");

namespace {
constexpr size_t kHeadBytes = 32;
static_assert(sizeof(SyncHead) == kHeadBytes, "frame records follow the head");

// the refusals that depend on the shape alone (dabgpu_sync_check: no context, no device); nullptr = fine
const char *shape_refusal(const Geometry &g, size_t n_samples, int max_shift)
{
    if (max_shift < 0 || max_shift > kSyncMaxShift) return "sync: max_shift must lie in 0 ... 31";
    if (n_samples < 2 * tf_samples(g) + (size_t)g.null_size)
        return "sync: the capture is too short (n_samples >= 2 tf_samples + null_size: no whole frame is guaranteed in less)";
    return nullptr;
}

int check_sync(dabgpu_ctx *c, const void *iq, int format, size_t n_samples, int max_shift, bool device)
{
    if (int rc = check_capture(c, "sync", iq, format, device)) return rc;
    if (const char *why = shape_refusal(c->g, n_samples, max_shift)) return fail(c, DABGPU_E_INVALID, why);
    return DABGPU_OK;
}

size_t frame_slots(const dabgpu_ctx *c, size_t n_samples)
{
    return std::min<size_t>((size_t)c->max_frames, n_samples / tf_samples(c->g));
}

SyncArgs capture_args(dabgpu_ctx *c, const void *d_iq, int format, size_t n_samples, int max_shift)
{
    SyncArgs a{};
    a.g = c->g;
    a.t = tables_of(c);
    a.iq = d_iq;
    a.fmt = format;
    a.n = (long long)n_samples;
    a.max_shift = max_shift;
    a.slots = (int)frame_slots(c, n_samples);
    a.power = (float *)c->sync.power.p;
    a.nblk = (int)(std::min(n_samples, tf_samples(c->g) + (size_t)c->g.null_size) / (size_t)(c->g.N / 32));
    a.head = (SyncHead *)c->sync.result.p;
    a.frames = (SyncFrame *)((char *)c->sync.result.p + kHeadBytes);
    return a;
}
}  // namespace

extern "C" {
int dabgpu_sync_dev(dabgpu_ctx *c, const void *d_iq, int format, size_t n_samples, int max_shift, void *stream)
{
    CTXCHK(c);
    int rc = apply_settings(c);
    if (rc) return rc;
    if ((rc = check_sync(c, d_iq, format, n_samples, max_shift, true))) return rc;
    DevCall call(c, stream);
    if (call.rc) return call.rc;
    const size_t slots = frame_slots(c, n_samples);
    const size_t bytes = kHeadBytes + slots * sizeof(SyncFrame);
    HIPCHK(c, c->sync.result.reserve(bytes));
    HIPCHK(c, c->sync.power.reserve((tf_samples(c->g) + (size_t)c->g.null_size) / (size_t)(c->g.N / 32) * sizeof(float)));
    c->sync.n = 0;                                                    // (a failed launch leaves no result behind)
    HIPCHK(c, hipMemsetAsync(c->sync.result.p, 0, bytes, call.s));
    HIPCHK(c, launch_sync(capture_args(c, d_iq, format, n_samples, max_shift), call.s));
    c->sync.n = n_samples;
    c->sync.slots = slots;
    c->sync.stream = call.s;
    return DABGPU_OK;
}

int dabgpu_sync(dabgpu_ctx *c, const void *iq, int format, size_t n_samples, int max_shift)
{
    CTXCHK(c);
    if (int rc = check_sync(c, iq, format, n_samples, max_shift, false)) return rc;
    return capture_from_host(c, c->sync.in, iq, n_samples * sample_bytes(format),
                             [&](const void *d_iq) { return dabgpu_sync_dev(c, d_iq, format, n_samples, max_shift, c->stream); });
}

int dabgpu_get_sync_result(dabgpu_ctx *c, size_t *n_frames, dabgpu_sync_frame *out, size_t cap)
{
    CTXCHK(c);
    if (!n_frames || (cap && !out)) return fail(c, DABGPU_E_INVALID, "null argument");
    if (!c->sync.n) return fail(c, DABGPU_E_INVALID, "no synchroniser result (no dabgpu_sync* call yet)");
    HIPCHK(c, wait_result(c, c->sync.stream));
    SyncHead h;
    HIPCHK(c, hipMemcpy(&h, c->sync.result.p, sizeof h, hipMemcpyDeviceToHost));
    *n_frames = (size_t)h.count;
    const size_t m = std::min((size_t)h.count, cap);
    if (m) HIPCHK(c, hipMemcpy(out, (const char *)c->sync.result.p + kHeadBytes, m * sizeof(SyncFrame), hipMemcpyDeviceToHost));
    return DABGPU_OK;
}

int dabgpu_sync_extract_dev(dabgpu_ctx *c, const void *d_iq, int format, size_t n_samples, void *d_frames_out, void *stream)
{
    CTXCHK(c);
    int rc = check_sync(c, d_iq, format, n_samples, 0, true);
    if (rc) return rc;
    if (!d_frames_out) return fail(c, DABGPU_E_INVALID, "null argument");
    if (!sample_aligned(d_frames_out, 0)) return fail_misaligned(c, "sync");
    if (!c->sync.n || c->sync.n != n_samples)
        return fail(c, DABGPU_E_INVALID, "sync_extract: no dabgpu_sync* call on a capture of this many samples precedes it");
    DevCall call(c, stream);
    if (call.rc) return call.rc;
    HIPCHK(c, launch_sync_extract(capture_args(c, d_iq, format, n_samples, 0), (float2 *)d_frames_out, call.s));
    return DABGPU_OK;
}

int dabgpu_sync_extract(dabgpu_ctx *c, const void *iq, int format, size_t n_samples, void *frames_out)
{
    CTXCHK(c);
    int rc = check_sync(c, iq, format, n_samples, 0, false);
    if (rc) return rc;
    if (!frames_out) return fail(c, DABGPU_E_INVALID, "null argument");
    if (!c->sync.n || c->sync.n != n_samples)
        return fail(c, DABGPU_E_INVALID, "sync_extract: no dabgpu_sync* call on a capture of this many samples precedes it");
    if ((rc = dabgpu_synchronize(c))) return rc;
    const size_t out_bytes = c->sync.slots * tf_samples(c->g) * sizeof(float2);
    HostIO io(c);
    if ((rc = io.in(c->sync.in, iq, n_samples * sample_bytes(format)))) return rc;
    HIPCHK(c, c->sync.out.reserve(std::max<size_t>(out_bytes, 16)));
    if ((rc = dabgpu_sync_extract_dev(c, c->sync.in.p, format, n_samples, c->sync.out.p, c->stream))) return rc;
    return io.out(frames_out, c->sync.out.p, out_bytes);
}

int dabgpu_sync_check(int mode, size_t n_samples, int max_shift)
{
    Geometry g;
    if (!mode_geometry(mode, &g)) return fail(nullptr, DABGPU_E_INVALID, "sync: transmission mode not valid");
    if (const char *why = shape_refusal(g, n_samples, max_shift)) return fail(nullptr, DABGPU_E_INVALID, why);
    return DABGPU_OK;
}

}  // extern "C"
