// api_superframe.hip -- the DAB+ superframe reader of superframe.hip behind the C-ABI: Fire code, RS(120,110) and AU CRCs of one
// sub-channel of decoded images or raw ETI frames, every alignment of five images a candidate (dabgpu_superframe / _dev,
// dabgpu_get_superframe_records), the greedy walk over a call's records (dabgpu_get_superframe_result) and the shape check
// (dabgpu_superframe_check, host only).  The reference sends superframes, it reads none; nothing here replaces a plugin of
// its flowgraph, which is why no entry is named *_process.
#include "dabgpu_ctx.h"
#include "superframe.h"

using namespace dabgpu;
using namespace dabgpu_api;

static_assert(sizeof(dabgpu_sf_record) == sizeof(SfRecord) && offsetof(dabgpu_sf_record, au_start) == offsetof(SfRecord, au_start) &&
                  offsetof(dabgpu_sf_record, cw_errors) == offsetof(SfRecord, cw_errors) &&
                  offsetof(dabgpu_sf_record, au_ok) == offsetof(SfRecord, au_ok) &&
                  offsetof(dabgpu_sf_record, fire_crc) == offsetof(SfRecord, fire_crc) &&
                  offsetof(dabgpu_sf_record, rfa) == offsetof(SfRecord, rfa),
              "the device writes the public records");
static_assert(DABGPU_SF_FIRE_OK == SF_FIRE_OK && DABGPU_SF_ZERO == SF_ZERO && DABGPU_SF_HEADER_VALID == SF_HEADER_VALID &&
                  DABGPU_SF_RS_FAILED == SF_RS_FAILED && DABGPU_SF_WORD_FAILED == kSfFailed && DABGPU_SF_MAX_WORDS == kSfMaxS,
              "flags and slots");
static_assert(sizeof(dabgpu_sf_result) == 48, "fixed layout of the result");

namespace {

const char *const kNoCall = "no superframe call (no dabgpu_superframe* call yet)";

// why a call of this shape is refused; nullptr: it is not
const char *shape_refusal(size_t n_images, size_t offset, size_t framesize)
{
    if (n_images < (size_t)kSfFrames || n_images > ((size_t)1 << 22)) return "superframe: n_images must lie in 5 ... 2^22";
    if (framesize == 0 || framesize % 24 || framesize / 24 > (size_t)kSfMaxS)
        return "superframe: framesize must be 24 s with s in 1 ... 24 (8 ... 192 kbit/s)";
    if (offset % 4) return "superframe: offset must be a multiple of 4";
    if (offset > 6144 || offset + framesize > 6144) return "superframe: offset + framesize exceeds the 6144-byte image";
    return nullptr;
}

void walk(const std::vector<SfRecord> &rec, dabgpu_sf_result *out, std::vector<uint32_t> *accepted)
{
    std::memset(out, 0, sizeof *out);
    out->candidates = (uint32_t)rec.size();
    out->first = -1;
    size_t last = 0;
    for (size_t f = 0; f < rec.size();) {
        const SfRecord &r = rec[f];
        if (!sf_accepted(r.flags)) {
            f += 1;
            continue;
        }
        if (out->first < 0) out->first = (int32_t)f;
        else if (f % kSfFrames != last % kSfFrames) out->phase_changes++;
        last = f;
        const uint32_t ok = (uint32_t)__builtin_popcount(r.au_ok);
        out->superframes++;
        out->aus += r.num_aus;
        out->aus_ok += ok;
        out->aus_bad += r.num_aus - ok;
        out->rs_corrected += r.rs_corrected;
        out->rs_failed += r.rs_failed;
        out->rs_max = std::max<uint32_t>(out->rs_max, r.rs_max);
        accepted->push_back((uint32_t)f);
        f += kSfFrames;
    }
}

}  // namespace

extern "C" {
int dabgpu_superframe_check(size_t n_images, size_t offset, size_t framesize)
{
    if (const char *why = shape_refusal(n_images, offset, framesize)) return fail(nullptr, DABGPU_E_INVALID, why);
    return DABGPU_OK;
}

int dabgpu_superframe_dev(dabgpu_ctx *c, const void *d_images, size_t n_images, size_t offset, size_t framesize, void *d_out,
                          size_t out_cap, size_t *out_bytes, void *stream)
{
    CTXCHK(c);
    if (const char *why = shape_refusal(n_images, offset, framesize)) return fail(c, DABGPU_E_INVALID, why);
    if (!d_images || !d_out) return fail(c, DABGPU_E_INVALID, "null argument");
    if ((uintptr_t)d_images & 3u) return fail(c, DABGPU_E_INVALID, "superframe: images must be aligned to four bytes");
    const size_t s = framesize / 24, n = n_images - (kSfFrames - 1);
    if (int rc = check_out(c, n * kSfK * s, out_cap, out_bytes)) return rc;
    DevCall call(c, stream);
    if (call.rc) return call.rc;
    HIPCHK(c, c->superframe.rec.reserve(n * sizeof(SfRecord)));
    c->superframe.done = false;                                       // (a failed launch leaves no result behind)
    SfArgs a{};
    a.images = (const uint8_t *)d_images;
    a.n_images = (uint32_t)n_images;
    a.offset = (uint32_t)offset;
    a.s = (uint32_t)s;
    a.rec = (SfRecord *)c->superframe.rec.p;
    a.out = (uint8_t *)d_out;
    HIPCHK(c, launch_superframe(a, call.s));
    c->superframe.done = true;
    c->superframe.candidates = n;
    c->superframe.stream = call.s;
    return DABGPU_OK;
}

int dabgpu_superframe(dabgpu_ctx *c, const uint8_t *images, size_t n_images, size_t offset, size_t framesize, uint8_t *out,
                      size_t out_cap, size_t *out_bytes)
{
    CTXCHK(c);
    if (const char *why = shape_refusal(n_images, offset, framesize)) return fail(c, DABGPU_E_INVALID, why);
    if (!images || !out) return fail(c, DABGPU_E_INVALID, "null argument");
    const size_t need = (n_images - (kSfFrames - 1)) * kSfK * (framesize / 24);
    if (int rc = check_out(c, need, out_cap, out_bytes)) return rc;
    int rc = dabgpu_synchronize(c);
    if (rc) return rc;
    HostIO io(c);
    if ((rc = io.in(c->superframe.in, images, n_images * 6144))) return rc;
    HIPCHK(c, c->superframe.out.reserve(need));
    if ((rc = dabgpu_superframe_dev(c, c->superframe.in.p, n_images, offset, framesize, c->superframe.out.p, need, nullptr, c->stream)))
        return rc;
    return io.out(out, c->superframe.out.p, need);
}

int dabgpu_get_superframe_records(dabgpu_ctx *c, dabgpu_sf_record *out, size_t cap, size_t *n)
{
    CTXCHK(c);
    if (cap && !out) return fail(c, DABGPU_E_INVALID, "null argument");
    if (!c->superframe.done) return fail(c, DABGPU_E_INVALID, kNoCall);
    HIPCHK(c, wait_result(c, c->superframe.stream));
    if (n) *n = c->superframe.candidates;
    const size_t m = std::min(cap, c->superframe.candidates);
    if (m) HIPCHK(c, hipMemcpy(out, c->superframe.rec.p, m * sizeof(SfRecord), hipMemcpyDeviceToHost));
    return DABGPU_OK;
}

int dabgpu_get_superframe_result(dabgpu_ctx *c, dabgpu_sf_result *out, uint32_t *accepted, size_t cap)
{
    CTXCHK(c);
    if (!out || (cap && !accepted)) return fail(c, DABGPU_E_INVALID, "null argument");
    if (!c->superframe.done) return fail(c, DABGPU_E_INVALID, kNoCall);
    HIPCHK(c, wait_result(c, c->superframe.stream));
    std::vector<SfRecord> rec(c->superframe.candidates);
    HIPCHK(c, hipMemcpy(rec.data(), c->superframe.rec.p, rec.size() * sizeof(SfRecord), hipMemcpyDeviceToHost));
    std::vector<uint32_t> found;
    walk(rec, out, &found);
    for (size_t i = 0; i < std::min(cap, found.size()); ++i) accepted[i] = found[i];
    return DABGPU_OK;
}

}  // extern "C"
