// fic.h -- the FIC reader (fic.hip, api_fic.hip): what one Fast Information Block says, as one fixed-size record, and the
// summary of a run of FIBs that the reduction combines.  The walk over a FIB (fic_read_fib) and the combination of two adjacent
// runs (fic_combine) are plain C++ for host and device: the kernel runs them per lane, a host compiler builds them alone.
// EN 300 401 5.2 (FIB, CRC, FIG header), 6.2.1 (FIG 0/0), 6.2.1 / 6.3.1 (FIG 0/1, 0/2), 8.1 (FIG 1/0, 1/1).
//
// The walk trusts no length: a FIG whose length runs past byte 29 ends the walk (figs_truncated), an entry that the end of its
// FIG cuts off is dropped, and no byte outside the FIB's 32 is read.  (The reference's FICDecoder, src/FigParser.cpp:105-321,
// trusts the lengths and reads on: the documented deviation, INTEGRATION.md F.)
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FIC_HD __host__ __device__ inline
#else
#define FIC_HD inline
#endif

namespace dabgpu {

constexpr int kFibBytes = 32, kFibData = 30;
constexpr int kFicRecSub = 9;             // FIG 0/1 entries one FIB can hold (28 field bytes / 3)
constexpr int kFicRecServices = 4;        // FIG 0/2 services kept per FIB
constexpr int kFicRecComponents = 8;      //   and their components, all services together
enum : uint32_t { FIC_CRC_OK = 1, FIC_ZERO = 2, FIC_TRUNCATED = 4 };

// the layouts of dabgpu_fic_sub_entry ... dabgpu_fic_record (include/dabgpu.h documents the fields)
struct FicSubEntry {
    uint32_t raw;
    uint16_t sad, size;
    uint8_t subchid, form, sw_option, index_level;
};
struct FicService {
    uint16_t sid;
    uint8_t info, first_comp;
};
struct FicComponent {
    uint16_t id;
    uint8_t tmid, type, primary, ca, service, reserved;
};
struct FicLabel {
    uint8_t kind, charset;
    uint16_t id, flag;
    uint8_t text[16];
    uint16_t reserved;
};
struct FicRecord {
    uint32_t flags;
    uint16_t eid_first, eid;
    uint8_t eid_seen, eid_changes, change, alarm;
    uint8_t cif_hi, cif_lo, n_sub, n_svc;
    uint8_t n_comp, services_dropped, components_dropped, labels_dropped;
    uint8_t figs_truncated, fig0_skipped, reserved[2];
    uint8_t figs_type[8];
    uint8_t fig0_ext[32];
    FicSubEntry sub[kFicRecSub];
    FicService svc[kFicRecServices];
    FicComponent comp[kFicRecComponents];
    FicLabel label;
    uint8_t pad[12];
};
static_assert(sizeof(FicSubEntry) == 12 && sizeof(FicService) == 4 && sizeof(FicComponent) == 8 && sizeof(FicLabel) == 24 &&
                  sizeof(FicRecord) == 288 && offsetof(FicRecord, sub) == 64 && offsetof(FicRecord, label) == 252,
              "fixed layout of a FIB's record");

// The summary of a run of FIBs for one key (a SubChId's FIG 0/1 entry, the EId): the first and the last word seen, how many,
// how often the word differed from the one before it, and the FIBs of the first and the last sighting.  seen = 0: nothing.
struct FicRun {
    uint32_t first_word, last_word, seen, changes, first_fib, last_fib;
};
// A then B, adjacent: associative, so any tree over adjacent runs gives what one pass over the FIBs gives.
FIC_HD FicRun fic_combine(const FicRun &a, const FicRun &b)
{
    if (!a.seen) return b;
    if (!b.seen) return a;
    FicRun r;
    r.first_word = a.first_word;
    r.last_word = b.last_word;
    r.seen = a.seen + b.seen;
    r.changes = a.changes + b.changes + (a.last_word != b.first_word ? 1u : 0u);
    r.first_fib = a.first_fib;
    r.last_fib = b.last_fib;
    return r;
}
FIC_HD FicRun fic_sighting(uint32_t word, uint32_t fib)
{
    FicRun r;
    r.first_word = r.last_word = word;
    r.seen = 1;
    r.changes = 0;
    r.first_fib = r.last_fib = fib;
    return r;
}

// what the reduction sums, per FIB: where each figure lies in FicReduced::counter
enum {
    FIC_C_FIBS = 0, FIC_C_OK, FIC_C_BAD, FIC_C_ZERO, FIC_C_TRUNCATED, FIC_C_FIG0_SKIPPED, FIC_C_SERVICES_DROPPED,
    FIC_C_COMPONENTS_DROPPED, FIC_C_LABELS_DROPPED, FIC_C_TYPE = 16, FIC_C_EXT = 24, FIC_COUNTERS = 56
};
FIC_HD uint32_t fic_counter_of(const FicRecord &r, int c)
{
    const bool ok = r.flags & FIC_CRC_OK, zero = r.flags & FIC_ZERO;
    switch (c) {
    case FIC_C_FIBS: return 1;
    case FIC_C_OK: return ok;
    case FIC_C_BAD: return !ok && !zero;
    case FIC_C_ZERO: return zero;
    case FIC_C_TRUNCATED: return r.figs_truncated;
    case FIC_C_FIG0_SKIPPED: return r.fig0_skipped;
    case FIC_C_SERVICES_DROPPED: return r.services_dropped;
    case FIC_C_COMPONENTS_DROPPED: return r.components_dropped;
    case FIC_C_LABELS_DROPPED: return r.labels_dropped;
    default: break;
    }
    if (c >= FIC_C_EXT && c < FIC_C_EXT + 32) return r.fig0_ext[c - FIC_C_EXT];
    if (c >= FIC_C_TYPE && c < FIC_C_TYPE + 8) return r.figs_type[c - FIC_C_TYPE];
    return 0;
}
struct FicReduced {
    uint32_t counter[64];
    FicRun eid;
    FicRun sub[64];
};

// CRC-16, x^16 + x^12 + x^5 + 1, register all ones at the start, result complemented (EN 300 401 5.2.1): one byte per step
FIC_HD uint32_t fic_crc_step(uint32_t crc, uint32_t byte)
{
    uint32_t x = ((crc >> 8) ^ byte) & 0xffu;
    x ^= x >> 4;
    return ((crc << 8) ^ (x << 12) ^ (x << 5) ^ x) & 0xffffu;
}

// One FIB, b[0 ... 31], into *r (every byte of it is written).
FIC_HD void fic_read_fib(const uint8_t *b, FicRecord *r)
{
    {
        uint32_t *w = reinterpret_cast<uint32_t *>(r);
        for (size_t i = 0; i < sizeof(FicRecord) / 4; ++i) w[i] = 0;
    }
    uint32_t crc = 0xffffu, any = 0;
    for (int i = 0; i < kFibData; ++i) {
        crc = fic_crc_step(crc, b[i]);
        any |= b[i];
    }
    crc ^= 0xffffu;
    any |= (uint32_t)b[30] | b[31];
    if (!any) r->flags = FIC_ZERO;
    if (crc != ((uint32_t)b[30] << 8 | b[31])) return;
    r->flags = FIC_CRC_OK;
    int p = 0;
    while (p < kFibData) {
        const uint32_t head = b[p];
        if (head == 0xffu) break;
        const int type = (int)(head >> 5), len = (int)(head & 31u), d = p + 1, end = d + len;
        if (end > kFibData) {
            r->figs_truncated = 1;
            r->flags |= FIC_TRUNCATED;
            break;
        }
        p = end;
        r->figs_type[type]++;
        if (len < 1) continue;
        const uint32_t h = b[d];
        if (type == 0) {
            const int ext = (int)(h & 31u);
            r->fig0_ext[ext]++;
            if (ext > 2) continue;
            if (h & 0xe0u) {                                           // C/N, OE or P/D: next configuration, other ensemble, data
                r->fig0_skipped++;
                continue;
            }
            int o = d + 1;
            if (ext == 0) {
                if (end - o < 4) continue;
                const uint16_t eid = (uint16_t)(b[o] << 8 | b[o + 1]);
                if (!r->eid_seen) r->eid_first = eid;
                else if (r->eid != eid) r->eid_changes++;
                r->eid = eid;
                r->eid_seen++;
                r->change = (uint8_t)(b[o + 2] >> 6);
                r->alarm = (b[o + 2] >> 5) & 1u;
                r->cif_hi = b[o + 2] & 31u;
                r->cif_lo = b[o + 3];
            } else if (ext == 1) {
                while (end - o >= 3) {
                    const uint32_t b0 = b[o], b1 = b[o + 1], b2 = b[o + 2];
                    const bool is_long = b2 & 0x80u;
                    if (is_long && end - o < 4) break;                 // cut off by the end of its FIG: dropped
                    const uint32_t b3 = is_long ? b[o + 3] : 0u;
                    o += is_long ? 4 : 3;
                    if (r->n_sub >= kFicRecSub) break;                 // (28 field bytes hold nine entries at the most)
                    FicSubEntry &e = r->sub[r->n_sub++];
                    e.raw = b0 << 24 | b1 << 16 | b2 << 8 | b3;
                    e.subchid = (uint8_t)(b0 >> 2);
                    e.sad = (uint16_t)((b0 & 3u) << 8 | b1);
                    e.form = is_long;
                    if (is_long) {
                        e.sw_option = (b2 >> 4) & 7u;
                        e.index_level = (b2 >> 2) & 3u;
                        e.size = (uint16_t)((b2 & 3u) << 8 | b3);
                    } else {
                        e.sw_option = (b2 >> 6) & 1u;
                        e.index_level = b2 & 63u;
                    }
                }
            } else {
                while (end - o >= 3) {
                    const uint32_t info = b[o + 2], nc = info & 15u;
                    if (end - o < 3 + 2 * (int)nc) break;              // cut off: dropped with its components
                    if (r->n_svc >= kFicRecServices || r->n_comp + nc > (uint32_t)kFicRecComponents) {
                        r->services_dropped++;
                        r->components_dropped += (uint8_t)nc;
                    } else {
                        FicService &s = r->svc[r->n_svc];
                        s.sid = (uint16_t)(b[o] << 8 | b[o + 1]);
                        s.info = (uint8_t)info;
                        s.first_comp = r->n_comp;
                        for (uint32_t k = 0; k < nc; ++k) {
                            const uint32_t c0 = b[o + 3 + 2 * k], c1 = b[o + 4 + 2 * k];
                            FicComponent &c = r->comp[r->n_comp++];
                            c.tmid = (uint8_t)(c0 >> 6);
                            c.type = c.tmid == 3 ? 0 : (uint8_t)(c0 & 63u);
                            c.id = c.tmid == 3 ? (uint16_t)((c0 & 63u) << 6 | c1 >> 2) : (uint16_t)(c1 >> 2);
                            c.primary = (c1 >> 1) & 1u;
                            c.ca = c1 & 1u;
                            c.service = r->n_svc;
                        }
                        r->n_svc++;
                    }
                    o += 3 + 2 * (int)nc;
                }
            }
        } else if (type == 1) {
            const int ext = (int)(h & 7u);
            if ((h & 8u) || ext > 1 || len != 1 + 2 + 16 + 2) continue;   // OE; not 1/0 or 1/1; not a whole label
            if (r->label.kind) {
                r->labels_dropped++;
                continue;
            }
            FicLabel &l = r->label;
            l.kind = (uint8_t)(1 + ext);
            l.charset = (uint8_t)(h >> 4);
            l.id = (uint16_t)(b[d + 1] << 8 | b[d + 2]);
            for (int k = 0; k < 16; ++k) l.text[k] = b[d + 3 + k];
            l.flag = (uint16_t)(b[d + 19] << 8 | b[d + 20]);
        }
    }
}

// fic.hip
struct FicArgs {
    const uint8_t *images;    // n_images x 6144 bytes, four-byte aligned
    uint32_t n_images, fibs_per_image, fic_offset;
    FicRecord *rec;           // n_images x fibs_per_image records, in stream order
    FicReduced *partial;      // scratch: one per 256 FIBs
    FicReduced *result;
};
constexpr int kFicBlock = 256;            // FIBs per workgroup, of both kernels
#if defined(__HIPCC__)
hipError_t launch_fic(const FicArgs &a, hipStream_t s);
#endif

}  // namespace dabgpu
