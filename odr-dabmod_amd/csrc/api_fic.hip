// api_fic.hip -- the FIC reader of fic.hip behind the C-ABI: FIB CRCs and the FIGs that say how an ensemble is laid out, read
// from decoded images or raw ETI frames on the device (dabgpu_fic_scan / _dev, dabgpu_get_fic_result / _records / _services), and
// the host logic that turns a result into the ETI header dabgpu_frontend_configure wants (dabgpu_fic_make_header,
// dabgpu_fic_bootstrap_frame, dabgpu_decode_configure_from_fic).  The reference reads ensembles on the CPU (FICDecoder,
// src/FigParser.cpp); nothing here replaces a plugin of its flowgraph, which is why no entry is named *_process.
#include "dabgpu_ctx.h"
#include "fic.h"

#include <array>

using namespace dabgpu;
using namespace dabgpu_api;

static_assert(sizeof(dabgpu_fic_record) == sizeof(FicRecord) && offsetof(dabgpu_fic_record, sub) == offsetof(FicRecord, sub) &&
                  offsetof(dabgpu_fic_record, svc) == offsetof(FicRecord, svc) && offsetof(dabgpu_fic_record, comp) == offsetof(FicRecord, comp) &&
                  offsetof(dabgpu_fic_record, label) == offsetof(FicRecord, label) &&
                  offsetof(dabgpu_fic_record, fig0_ext) == offsetof(FicRecord, fig0_ext),
              "the device writes the public records");
static_assert(sizeof(dabgpu_fic_sub_entry) == sizeof(FicSubEntry) && sizeof(dabgpu_fic_component) == sizeof(FicComponent) &&
                  sizeof(dabgpu_fic_label) == sizeof(FicLabel) && sizeof(dabgpu_fic_service_entry) == sizeof(FicService),
              "the device writes the public records");
static_assert(DABGPU_FIC_REC_SUBCH == kFicRecSub && DABGPU_FIC_REC_SERVICES == kFicRecServices &&
                  DABGPU_FIC_REC_COMPONENTS == kFicRecComponents && DABGPU_FIC_CRC_OK == FIC_CRC_OK && DABGPU_FIC_ZERO == FIC_ZERO &&
                  DABGPU_FIC_TRUNCATED == FIC_TRUNCATED,
              "record slots and flags");
static_assert(sizeof(dabgpu_fic_result) == 4320 && sizeof(dabgpu_fic_subch) == 64 && sizeof(dabgpu_fic_service) == 136,
              "fixed layout of the result");

namespace {

#include "../host/protection_tables.inc"

const char *const kNoScan = "no FIC scan (no dabgpu_fic_scan* call yet)";

// EN 300 401 table 6 (the short form's table index): ascending bit rate, level 5 down to 1, the combinations that have a profile
struct ShortRow {
    uint16_t bitrate, cu;
    uint8_t level;
};
struct ShortTable {
    ShortRow row[64];
    int n = 0;
    ShortTable()
    {
        std::vector<const UepProfile *> all;
        for (const UepProfile &u : kUepProfiles) all.push_back(&u);
        std::stable_sort(all.begin(), all.end(), [](const UepProfile *a, const UepProfile *b) {
            return a->bitrate != b->bitrate ? a->bitrate < b->bitrate : a->level > b->level;
        });
        for (const UepProfile *u : all)
            if (n < 64) row[n++] = {u->bitrate, u->cu, u->level};
    }
};
const ShortTable &short_table()
{
    static const ShortTable t;
    return t;
}

const uint32_t kEepA[4] = {12, 8, 6, 4}, kEepB[4] = {27, 21, 18, 15};

// the fields that follow from a FIG 0/1 entry's raw word
void derive(uint32_t raw, dabgpu_fic_subch *s)
{
    const uint32_t b0 = raw >> 24, b1 = (raw >> 16) & 0xffu, b2 = (raw >> 8) & 0xffu, b3 = raw & 0xffu;
    s->subchid = b0 >> 2;
    s->sad = (b0 & 3u) << 8 | b1;
    s->form = b2 >> 7;
    s->raw = raw;
    if (!s->form) {
        s->table_switch = (b2 >> 6) & 1u;
        s->index_option = b2 & 63u;
        const ShortTable &t = short_table();
        if (!s->table_switch && (int)s->index_option < t.n) {
            const ShortRow &r = t.row[s->index_option];
            s->bitrate = r.bitrate;
            s->level = r.level;
            s->size_cu = r.cu;
            s->tpl = s->level - 1u;
            s->supported = 1;
        }
    } else {
        s->index_option = (b2 >> 4) & 7u;
        s->level = ((b2 >> 2) & 3u) + 1u;
        s->size_cu = (b2 & 3u) << 8 | b3;
        if (s->index_option <= 1) {
            const uint32_t f = (s->index_option ? kEepB : kEepA)[s->level - 1];
            if (s->size_cu && s->size_cu % f == 0) {
                s->bitrate = s->size_cu / f * (s->index_option ? 32u : 8u);
                s->tpl = 0x20u | s->index_option << 2 | (s->level - 1u);
                s->supported = 1;
            }
        }
    }
    s->stl = 3u * s->bitrate / 8u;
}

void build_result(const FicReduced &r, dabgpu_fic_result *out)
{
    std::memset(out, 0, sizeof *out);
    out->fibs = r.counter[FIC_C_FIBS];
    out->fibs_ok = r.counter[FIC_C_OK];
    out->fibs_bad = r.counter[FIC_C_BAD];
    out->fibs_zero = r.counter[FIC_C_ZERO];
    out->figs_truncated = r.counter[FIC_C_TRUNCATED];
    out->fig0_skipped = r.counter[FIC_C_FIG0_SKIPPED];
    out->services_dropped = r.counter[FIC_C_SERVICES_DROPPED];
    out->components_dropped = r.counter[FIC_C_COMPONENTS_DROPPED];
    out->labels_dropped = r.counter[FIC_C_LABELS_DROPPED];
    for (int t = 0; t < 8; ++t) out->figs_type[t] = r.counter[FIC_C_TYPE + t];
    for (int e = 0; e < 32; ++e) out->fig0_ext[e] = r.counter[FIC_C_EXT + e];
    if (r.eid.seen) {
        out->eid = r.eid.last_word;
        out->eid_seen = r.eid.seen;
        out->eid_changes = r.eid.changes;
        out->eid_first_fib = r.eid.first_fib;
        out->eid_last_fib = r.eid.last_fib;
    }
    for (int id = 0; id < 64; ++id) {
        const FicRun &run = r.sub[id];
        if (!run.seen) continue;
        dabgpu_fic_subch &s = out->sub[out->n_subch++];
        derive(run.last_word, &s);
        s.seen = run.seen;
        s.changes = run.changes;
        s.first_fib = run.first_fib;
        s.last_fib = run.last_fib;
    }
}

int mid_of_mode(int mode) { return mode >= 1 && mode <= 3 ? mode : mode == 4 ? 0 : -1; }

// SYNC, FC, the STC words, EOH, a zero payload, EOF, TIST; 0x55 behind them (tests/golden/synth.py writes the same)
void write_header(int mode, const std::vector<std::array<uint32_t, 4>> &stc, uint8_t *f)
{
    const size_t nst = stc.size(), fic = mode == 3 ? 128 : 96;
    size_t mst = 0;
    for (const auto &s : stc) mst += 8 * (size_t)s[3];
    const size_t fl = (4 * nst + 4 + fic + mst) / 4;
    std::memset(f, 0x55, 6144);
    f[0] = 0xff; f[1] = 0x07; f[2] = 0x3a; f[3] = 0xb6;
    f[4] = 0;
    f[5] = (uint8_t)(0x80u | nst);
    f[6] = (uint8_t)((mid_of_mode(mode) & 3) << 3 | ((fl >> 8) & 7u));
    f[7] = (uint8_t)(fl & 0xffu);
    size_t p = 8;
    for (const auto &s : stc) {                                         // (SCId, SAD, TPL, STL)
        f[p] = (uint8_t)((s[0] & 63u) << 2 | ((s[1] >> 8) & 3u));
        f[p + 1] = (uint8_t)(s[1] & 0xffu);
        f[p + 2] = (uint8_t)((s[2] & 63u) << 2 | ((s[3] >> 8) & 3u));
        f[p + 3] = (uint8_t)(s[3] & 0xffu);
        p += 4;
    }
    const size_t body = 4 + fic + mst;                                  // EOH, FIC, MST
    if (p + body + 8 > 6144) return;                                    // (dabgpu_frontend_describe refuses this frame)
    std::memset(f + p, 0, body);
    p += body;
    f[p] = 0; f[p + 1] = 0; f[p + 2] = 0xff; f[p + 3] = 0xff;
    std::memset(f + p + 4, 0xff, 4);
}

}  // namespace

extern "C" {
int dabgpu_fic_scan_dev(dabgpu_ctx *c, const void *d_images, size_t n_images, size_t fic_offset, void *stream)
{
    CTXCHK(c);
    const size_t fic_bytes = c->g.mode == 3 ? 128 : 96;
    if (fic_offset == DABGPU_FIC_OFFSET_CONFIGURED) {
        if (!c->fe_configured)
            return fail(c, DABGPU_E_INVALID, "fic_scan: the configured FIC offset needs a configured front-end (dabgpu_frontend_configure)");
        fic_offset = c->fe_layout.fic_offset;
    }
    if (n_images < 1 || n_images > ((size_t)1 << 22)) return fail(c, DABGPU_E_INVALID, "fic_scan: n_images must lie in 1 ... 2^22");
    if (fic_offset % 4) return fail(c, DABGPU_E_INVALID, "fic_scan: fic_offset must be a multiple of 4");
    if (fic_offset > 6144 || fic_offset + fic_bytes > 6144)
        return fail(c, DABGPU_E_INVALID, "fic_scan: fic_offset + fic_bytes exceeds the 6144-byte image");
    if (!d_images) return fail(c, DABGPU_E_INVALID, "null argument");
    if ((uintptr_t)d_images & 3u) return fail(c, DABGPU_E_INVALID, "fic_scan: images must be aligned to four bytes");
    DevCall call(c, stream);
    if (call.rc) return call.rc;
    const size_t fpi = fic_bytes / 32, n_fibs = n_images * fpi, n_blocks = (n_fibs + kFicBlock - 1) / kFicBlock;
    HIPCHK(c, c->fic.rec.reserve(n_fibs * sizeof(FicRecord)));
    HIPCHK(c, c->fic.partial.reserve(n_blocks * sizeof(FicReduced)));
    HIPCHK(c, c->fic.result.reserve(sizeof(FicReduced)));
    c->fic.done = false;                                              // (a failed launch leaves no result behind)
    FicArgs a{};
    a.images = (const uint8_t *)d_images;
    a.n_images = (uint32_t)n_images;
    a.fibs_per_image = (uint32_t)fpi;
    a.fic_offset = (uint32_t)fic_offset;
    a.rec = (FicRecord *)c->fic.rec.p;
    a.partial = (FicReduced *)c->fic.partial.p;
    a.result = (FicReduced *)c->fic.result.p;
    HIPCHK(c, launch_fic(a, call.s));
    c->fic.done = true;
    c->fic.fibs = n_fibs;
    c->fic.stream = call.s;
    return DABGPU_OK;
}

int dabgpu_fic_scan(dabgpu_ctx *c, const uint8_t *images, size_t n_images, size_t fic_offset)
{
    CTXCHK(c);
    if (n_images < 1 || n_images > ((size_t)1 << 22)) return fail(c, DABGPU_E_INVALID, "fic_scan: n_images must lie in 1 ... 2^22");
    if (!images) return fail(c, DABGPU_E_INVALID, "null argument");
    return capture_from_host(c, c->fic.in, images, n_images * 6144,
                             [&](const void *d_images) { return dabgpu_fic_scan_dev(c, d_images, n_images, fic_offset, c->stream); });
}

int dabgpu_get_fic_result(dabgpu_ctx *c, dabgpu_fic_result *out)
{
    CTXCHK(c);
    if (!out) return fail(c, DABGPU_E_INVALID, "null argument");
    if (!c->fic.done) return fail(c, DABGPU_E_INVALID, kNoScan);
    HIPCHK(c, wait_result(c, c->fic.stream));
    FicReduced r;
    HIPCHK(c, hipMemcpy(&r, c->fic.result.p, sizeof r, hipMemcpyDeviceToHost));
    build_result(r, out);
    return DABGPU_OK;
}

int dabgpu_get_fic_records(dabgpu_ctx *c, dabgpu_fic_record *out, size_t cap, size_t *n)
{
    CTXCHK(c);
    if (cap && !out) return fail(c, DABGPU_E_INVALID, "null argument");
    if (!c->fic.done) return fail(c, DABGPU_E_INVALID, kNoScan);
    HIPCHK(c, wait_result(c, c->fic.stream));
    if (n) *n = c->fic.fibs;
    const size_t m = std::min(cap, c->fic.fibs);
    if (m) HIPCHK(c, hipMemcpy(out, c->fic.rec.p, m * sizeof(FicRecord), hipMemcpyDeviceToHost));
    return DABGPU_OK;
}

int dabgpu_get_fic_services(dabgpu_ctx *c, dabgpu_fic_service *out, size_t cap, size_t *n, dabgpu_fic_label *ensemble)
{
    CTXCHK(c);
    if (cap && !out) return fail(c, DABGPU_E_INVALID, "null argument");
    if (!c->fic.done) return fail(c, DABGPU_E_INVALID, kNoScan);
    HIPCHK(c, wait_result(c, c->fic.stream));
    std::vector<FicRecord> rec(c->fic.fibs);
    HIPCHK(c, hipMemcpy(rec.data(), c->fic.rec.p, rec.size() * sizeof(FicRecord), hipMemcpyDeviceToHost));
    std::vector<dabgpu_fic_service> found;
    dabgpu_fic_label ens;
    std::memset(&ens, 0, sizeof ens);
    auto service = [&](uint32_t sid) -> dabgpu_fic_service & {
        for (auto &s : found)
            if (s.sid == sid) return s;
        dabgpu_fic_service s;
        std::memset(&s, 0, sizeof s);
        s.sid = sid;
        found.push_back(s);
        return found.back();
    };
    for (const FicRecord &r : rec) {
        if (!(r.flags & FIC_CRC_OK)) continue;
        for (unsigned i = 0; i < r.n_svc && i < (unsigned)kFicRecServices; ++i) {
            dabgpu_fic_service &s = service(r.svc[i].sid);
            s.sightings++;
            const unsigned nc = r.svc[i].info & 15u;
            for (unsigned k = 0; k < nc && r.svc[i].first_comp + k < (unsigned)kFicRecComponents; ++k) {
                const FicComponent &fc = r.comp[r.svc[i].first_comp + k];
                dabgpu_fic_component *at = nullptr;
                for (uint32_t j = 0; j < s.n_components; ++j)
                    if (s.comp[j].tmid == fc.tmid && s.comp[j].id == fc.id) at = &s.comp[j];
                if (!at) {
                    if (s.n_components >= DABGPU_FIC_MAX_COMPONENTS) {
                        s.components_dropped++;
                        continue;
                    }
                    at = &s.comp[s.n_components++];
                }
                at->id = fc.id; at->tmid = fc.tmid; at->type = fc.type; at->primary = fc.primary; at->ca = fc.ca;
            }
        }
        if (r.label.kind == 1) std::memcpy(&ens, &r.label, sizeof ens);
        if (r.label.kind == 2) std::memcpy(&service(r.label.id).label, &r.label, sizeof ens);
    }
    if (n) *n = found.size();
    for (size_t i = 0; i < std::min(cap, found.size()); ++i) out[i] = found[i];
    if (ensemble) *ensemble = ens;
    return DABGPU_OK;
}

int dabgpu_fic_bootstrap_frame(int mode, uint8_t *frame)
{
    if (!frame) return fail(nullptr, DABGPU_E_INVALID, "null argument");
    if (mid_of_mode(mode) < 0) return fail(nullptr, DABGPU_E_INVALID, "fic: transmission mode not valid");
    write_header(mode, {}, frame);
    return DABGPU_OK;
}

int dabgpu_fic_make_header(const dabgpu_fic_result *r, int mode, uint8_t *frame)
{
    if (!r || !frame) return fail(nullptr, DABGPU_E_INVALID, "null argument");
    if (mid_of_mode(mode) < 0) return fail(nullptr, DABGPU_E_INVALID, "fic: transmission mode not valid");
    if (r->n_subch == 0)
        return fail(nullptr, DABGPU_E_INVALID, "fic: no sub-channel organisation seen (no FIG 0/1 in a FIB whose CRC holds)");
    if (r->n_subch > 64) return fail(nullptr, DABGPU_E_INVALID, "fic: more than 64 sub-channels");
    std::vector<std::array<uint32_t, 4>> stc;
    for (uint32_t i = 0; i < r->n_subch; ++i) {
        const dabgpu_fic_subch &s = r->sub[i];
        const std::string who = "fic: sub-channel " + std::to_string(s.subchid);
        if (s.changes)
            return fail(nullptr, DABGPU_E_INVALID, who + " was redefined inside the capture (" + std::to_string(s.changes) + " changes)");
        if (!s.supported) {
            if (!s.form)
                return fail(nullptr, DABGPU_E_INVALID, who + " is not supported: short form with the table switch set");
            if (s.index_option > 1)
                return fail(nullptr, DABGPU_E_INVALID, who + " is not supported: long form with protection option " + std::to_string(s.index_option));
            return fail(nullptr, DABGPU_E_INVALID, who + " is not supported: EEP size " + std::to_string(s.size_cu) +
                                                       " is not a multiple of " +
                                                       std::to_string((s.index_option ? kEepB : kEepA)[(s.level - 1u) & 3u]));
        }
        stc.push_back({s.subchid, s.sad, s.tpl, s.stl});
    }
    write_header(mode, stc, frame);
    dabgpu_fe_layout *lay = new dabgpu_fe_layout;
    int rc = dabgpu_frontend_describe(frame, lay);
    if (!rc) rc = dabgpu_decode_check_layout(lay);
    delete lay;
    return rc;
}

int dabgpu_decode_configure_from_fic(dabgpu_ctx *c)
{
    CTXCHK(c);
    dabgpu_fic_result *r = new dabgpu_fic_result;
    std::vector<uint8_t> frame(6144);
    int rc = dabgpu_get_fic_result(c, r);
    if (!rc && (rc = dabgpu_fic_make_header(r, c->g.mode ? c->g.mode : 4, frame.data()))) rc = fail(c, rc, dabgpu_last_error(nullptr));
    delete r;
    if (rc) return rc;
    return dabgpu_frontend_configure(c, frame.data());
}

}  // extern "C"
