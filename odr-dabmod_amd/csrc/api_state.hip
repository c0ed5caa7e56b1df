// api_state.hip -- the stream state of a context (include/dabgpu.h, "stream state"): the Resampler's halo -- the last rs_nin
// native-rate input samples, src/Resampler.cpp:142-147,188-191 -- and the TII frame parity (TII::m_insert,
// src/TII.cpp:226-242).  Read into a host blob, installed from one, or computed from the coded bits of ONE lead-in frame
// (every transmission frame is at least 96 hops long: the state behind frame k - 1 depends on the settings, on k and on that
// frame alone), so that one stream can be checkpointed, moved, or split over several contexts.  With the front-end on the
// device the lead-in is ETI frames, and the seed sets the time interleaver's history as well (dabgpu_chain_seed_eti).
#include "dabgpu_ctx.h"

using namespace dabgpu;
using namespace dabgpu_api;

namespace {
// the blob's header (include/dabgpu.h documents the layout); the halo follows, oldest sample first
struct StateHeader {
    uint32_t magic, version, mode, tii_insert;
    uint64_t rs_in, rs_out;
    uint32_t rs_nin, reserved;
};
static_assert(sizeof(StateHeader) == DABGPU_STREAM_STATE_HEADER_BYTES, "the layout include/dabgpu.h documents");

// samples of halo in a blob taken under these settings: none while the Resampler is not in the chain (equal rates), else
// rs_nin = (2 N / M) M = 2 N for every ratio the library accepts (M a power of two up to N, src/Resampler.cpp:69-75).  For
// dabgpu_stream_state_bytes only, which answers for settings that are not applied yet; get and set copy c->rs_nin samples,
// what the kernels read (halo_samples(c)).
size_t halo_samples(const Settings &st, int N)
{
    if (st.rs_in == st.rs_out || resampler_ratio_error(N, st.rs_in, st.rs_out)) return 0;
    return 2 * (size_t)N;
}

// ... of the context as it stands, settings applied
size_t halo_samples(const dabgpu_ctx *c) { return c->cur.rs_in == c->cur.rs_out ? 0 : (size_t)c->rs_nin; }

// the halo buffer the next call reads (which of the two it is never leaves the library)
float2 *current_halo(dabgpu_ctx *c) { return (float2 *)c->d_rs_halo.p + (size_t)c->rs_halo_cur * (size_t)c->rs_nin; }

// settings applied, every stream of the context idle: what get / set work on
int settle(dabgpu_ctx *c)
{
    int rc = dabgpu_synchronize(c);
    if (rc) return rc;
    if ((rc = apply_settings(c))) return rc;
    if (halo_samples(c) && (rc = check_resampler(c))) return rc;
    if (halo_samples(c) != halo_samples(c->cur, c->g.N)) return fail(c, DABGPU_E_INVALID, "stream state: inconsistent halo length");
    return DABGPU_OK;
}

// What a seed refuses and what it runs, decided before anything is queued (dabgpu_chain_seed / _dev, dabgpu_chain_seed_eti /
// _dev): have_bits = the caller has a lead-in frame of coded bits for it
struct SeedPlan {
    bool resample = false;
    ChainPlan p;                          // the lead-in frame's run in front of the Resampler (resample && frame_index only)
};
int plan_seed(dabgpu_ctx *c, unsigned mask, uint64_t frame_index, bool have_bits, SeedPlan *sp)
{
    mask = normalised_mask(c->cur, mask);
    sp->resample = mask & DABGPU_STAGE_RESAMPLE;
    if (sp->resample) {
        const int rc = check_resampler(c);
        if (rc) return rc;
    }
    if (frame_index == 0 || !sp->resample) return DABGPU_OK;
    if (!have_bits) return fail(c, DABGPU_E_INVALID, "chain seed: no lead-in frame");
    // Frame frame_index - 1 through everything in front of the Resampler, as complexf whatever the output format, with
    // the TII parity it has in the stream; on the context's own scratch (lane 0), its CFR statistics in the scratch set
    // of the chain's internal runs, its launches outside the trace: the most recent chain call stays the one that
    // dabgpu_get_cfr_stats / dabgpu_get_num_clipped / dabgpu_debug_last_variant describe.
    c->call_lanes = 1;
    sp->p = plan_chain(c, true, 1, mask & ~(unsigned)(DABGPU_STAGE_RESAMPLE | DABGPU_STAGE_POLY), false, false, chain_cic(c));
    if (sp->p.error) return fail(c, DABGPU_E_INVALID, sp->p.error);
    if (sp->p.native < (size_t)c->rs_nin) return fail(c, DABGPU_E_INVALID, "chain seed: frame shorter than the halo");
    return DABGPU_OK;
}

// d_bits is the lead-in frame in device memory (not read when the call is host-only)
int run_seed(dabgpu_ctx *c, const SeedPlan &sp, const void *d_bits, uint64_t frame_index, hipStream_t s)
{
    if (frame_index == 0) {
        // stream start: what dabgpu_set_resampler leaves
        if (sp.resample) HIPCHK(c, hipMemsetAsync(current_halo(c), 0, (size_t)c->rs_nin * sizeof(float2), s));
        c->tii_insert = true;
        return DABGPU_OK;
    }
    if (sp.resample) {
        const ChainPlan &p = sp.p;
        HIPCHK(c, c->d_a.reserve(p.native * sizeof(float2)));
        // (a seed that fails from here on puts the parity back: never one that belongs to neither stream)
        const bool insert_before = c->tii_insert;
        c->tii_insert = ((frame_index - 1) & 1) == 0;
        // (CIC equaliser on: the carriers kernel first, with the parity just set -- TII is in the carriers)
        const void *d_in = d_bits;
        int rc = run_front(c, p, &d_in, s);
        if (!rc) rc = run_native_tii(c, p, d_in, (float2 *)c->d_a.p, s);
        // the halo = the last two hops of the input so far (src/Resampler.cpp:188-191)
        if (!rc) {
            const hipError_t e = hipMemcpyAsync(current_halo(c), (const float2 *)c->d_a.p + (p.native - (size_t)c->rs_nin),
                                                (size_t)c->rs_nin * sizeof(float2), hipMemcpyDeviceToDevice, s);
            if (e != hipSuccess) rc = hip_fail(c, e, "hipMemcpyAsync (halo)");
        }
        if (rc) {
            c->tii_insert = insert_before;
            return rc;
        }
    }
    c->tii_insert = (frame_index & 1) == 0;            // TII on frames 0, 2, 4 ... of the stream (src/TII.cpp:226-242)
    return DABGPU_OK;
}

int seed_dev(dabgpu_ctx *c, const void *d_bits, unsigned mask, uint64_t frame_index, hipStream_t s)
{
    SeedPlan sp;
    const int rc = plan_seed(c, mask, frame_index, d_bits != nullptr, &sp);
    return rc ? rc : run_seed(c, sp, d_bits, frame_index, s);
}

// dabgpu_chain_seed_eti / _dev behind their checks: d_eti holds the n_leadin = min(e, 15 + cifs) ETI frames in front of
// frame e.  All but the last cifs of them give the history in front of transmission frame e / cifs - 1; that frame then
// goes through the ordinary front-end -- which leaves the history in front of frame e -- into scratch, and its coded bits
// seed the chain.  In stream order on s: memset, seed encode, the front-end's encode / assemble / shift, the chain's seed.
int seed_eti_dev(dabgpu_ctx *c, const void *d_eti, size_t n_leadin, unsigned mask, uint64_t e, hipStream_t s)
{
    const size_t cifs = (size_t)c->fe_cifs;
    SeedPlan sp;
    int rc = plan_seed(c, mask, e / cifs, true, &sp);
    if (rc) return rc;
    if (n_leadin) HIPCHK(c, c->d_fe_seed.reserve(tf_in_bytes(c->g)));
    const size_t m = n_leadin ? n_leadin - cifs : 0;
    if ((rc = frontend_seed_rows(c, d_eti, m, s))) return rc;
    if (n_leadin && (rc = run_frontend(c, (const uint8_t *)d_eti + m * 6144, cifs, c->d_fe_seed.p, s))) return rc;
    return run_seed(c, sp, c->d_fe_seed.p, e / cifs, s);
}
// The time interleaver's history (api_frontend.hip) is stream state the blob does not carry and one transmission frame
// cannot reproduce (it spans fifteen ETI frames): a context with a configured front-end is not seeded.
const char *const kSeedWithFrontend =
    "chain seed: the context carries front-end state (dabgpu_frontend_configure) that a seed from one transmission frame cannot reproduce";
}  // namespace

extern "C" {

size_t dabgpu_stream_state_bytes(const dabgpu_ctx *c)
{
    if (!c) return 0;
    std::lock_guard<std::mutex> lk(const_cast<dabgpu_ctx *>(c)->mu);
    return sizeof(StateHeader) + halo_samples(c->set, c->g.N) * sizeof(float2);
}

int dabgpu_get_stream_state(dabgpu_ctx *c, void *buf, size_t cap, size_t *bytes)
{
    CTXCHK(c);
    if (!buf) return fail(c, DABGPU_E_INVALID, "null argument");
    int rc = settle(c);
    if (rc) return rc;
    const size_t n = halo_samples(c), need = sizeof(StateHeader) + n * sizeof(float2);
    if (bytes) *bytes = need;
    if (need > cap) return fail(c, DABGPU_E_CAPACITY, "stream state: buffer too small");
    StateHeader h{};
    h.magic = DABGPU_STREAM_STATE_MAGIC;
    h.version = DABGPU_STREAM_STATE_VERSION;
    h.mode = (uint32_t)c->g.mode;
    h.tii_insert = c->tii_insert ? 1u : 0u;
    h.rs_in = c->cur.rs_in;
    h.rs_out = c->cur.rs_out;
    h.rs_nin = (uint32_t)n;
    std::memcpy(buf, &h, sizeof h);
    if (n) HIPCHK(c, hipMemcpy((char *)buf + sizeof h, current_halo(c), n * sizeof(float2), hipMemcpyDeviceToHost));
    return DABGPU_OK;
}

int dabgpu_set_stream_state(dabgpu_ctx *c, const void *buf, size_t bytes)
{
    CTXCHK(c);
    if (!buf) return fail(c, DABGPU_E_INVALID, "null argument");
    int rc = settle(c);
    if (rc) return rc;
    StateHeader h;
    if (bytes < sizeof h) return fail(c, DABGPU_E_INVALID, "stream state: shorter than its header");
    std::memcpy(&h, buf, sizeof h);
    if (h.magic != DABGPU_STREAM_STATE_MAGIC) return fail(c, DABGPU_E_INVALID, "stream state: not a stream state (magic)");
    if (h.version != DABGPU_STREAM_STATE_VERSION) return fail(c, DABGPU_E_INVALID, "stream state: unknown version");
    if (h.mode != (uint32_t)c->g.mode) return fail(c, DABGPU_E_INVALID, "stream state: taken in another transmission mode");
    if (h.rs_in != c->cur.rs_in || h.rs_out != c->cur.rs_out)
        return fail(c, DABGPU_E_INVALID, "stream state: taken at another resampling ratio");
    const size_t n = halo_samples(c);
    if (h.rs_nin != n) return fail(c, DABGPU_E_INVALID, "stream state: another halo length");
    if (h.tii_insert > 1 || h.reserved) return fail(c, DABGPU_E_INVALID, "stream state: malformed header");
    if (bytes != sizeof h + n * sizeof(float2)) return fail(c, DABGPU_E_INVALID, "stream state: size does not match its header");
    if (n) HIPCHK(c, hipMemcpy(current_halo(c), (const char *)buf + sizeof h, n * sizeof(float2), hipMemcpyHostToDevice));
    c->tii_insert = h.tii_insert != 0;
    return DABGPU_OK;
}

int dabgpu_chain_seed_dev(dabgpu_ctx *c, const void *d_leadin_bits, unsigned mask, uint64_t frame_index, void *stream)
{
    CTXCHK(c);
    if (c->fe_configured) return fail(c, DABGPU_E_INVALID, kSeedWithFrontend);
    const int rc = apply_settings(c);
    if (rc) return rc;
    // (stream == NULL: lane 0, where the resampler chain calls that follow go -- api_lanes.hip, pick_lane)
    return seed_dev(c, d_leadin_bits, mask, frame_index, stream ? (hipStream_t)stream : c->stream);
}

int dabgpu_chain_seed(dabgpu_ctx *c, const uint8_t *leadin_bits, unsigned mask, uint64_t frame_index)
{
    CTXCHK(c);
    if (c->fe_configured) return fail(c, DABGPU_E_INVALID, kSeedWithFrontend);
    int rc = apply_settings(c);
    if (rc) return rc;
    const void *d_bits = nullptr;
    if (frame_index && (normalised_mask(c->cur, mask) & DABGPU_STAGE_RESAMPLE)) {
        if (!leadin_bits) return fail(c, DABGPU_E_INVALID, "chain seed: no lead-in frame");
        // staged in pinned memory, so that the call returns at once; the device copy is read in stream order, two frames of
        // it in turn (this seed's upload may pass the kernels of the seed before it)
        const size_t nb = tf_in_bytes(c->g);
        const int k = (int)(c->seed_seq++ & 1);
        if (!c->h_seed[k]) {
            HIPCHK(c, hipHostMalloc(&c->h_seed[k], nb, hipHostMallocDefault));
            HIPCHK(c, hipEventCreateWithFlags(&c->seed_ev[k], hipEventDisableTiming));
        } else
            HIPCHK(c, hipEventSynchronize(c->seed_ev[k]));     // (the seed before the last one has read its frame)
        HIPCHK(c, c->d_seed.reserve(2 * nb));
        std::memcpy(c->h_seed[k], leadin_bits, nb);
        void *d = (char *)c->d_seed.p + (size_t)k * nb;
        HIPCHK(c, hipMemcpyAsync(d, c->h_seed[k], nb, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipEventRecord(c->seed_ev[k], c->stream));
        d_bits = d;
    }
    return seed_dev(c, d_bits, mask, frame_index, c->stream);
}

int dabgpu_chain_seed_eti_dev(dabgpu_ctx *c, const void *d_eti_leadin, size_t n_leadin, unsigned mask, uint64_t e, void *stream)
{
    CTXCHK(c);
    int rc = frontend_seed_check(c, n_leadin, e, (size_t)kFeHistory + (size_t)(c->fe_configured ? c->fe_cifs : 0));
    if (rc) return rc;
    if (n_leadin && !d_eti_leadin) return fail(c, DABGPU_E_INVALID, "null argument");
    if ((rc = apply_settings(c))) return rc;
    if (!stream && (rc = own_stream_joins_lanes(c))) return rc;
    return seed_eti_dev(c, d_eti_leadin, n_leadin, mask, e, stream ? (hipStream_t)stream : c->stream);
}

int dabgpu_chain_seed_eti(dabgpu_ctx *c, const uint8_t *eti_leadin, size_t n_leadin, unsigned mask, uint64_t e)
{
    CTXCHK(c);
    int rc = frontend_seed_check(c, n_leadin, e, (size_t)kFeHistory + (size_t)(c->fe_configured ? c->fe_cifs : 0));
    if (rc) return rc;
    if ((rc = frontend_check_leadin_host(c, eti_leadin, n_leadin))) return rc;
    if ((rc = apply_settings(c))) return rc;
    if ((rc = own_stream_joins_lanes(c))) return rc;
    HostIO io(c);
    if ((rc = io.in(c->d_fe_eti, eti_leadin, n_leadin * 6144))) return rc;
    if ((rc = seed_eti_dev(c, c->d_fe_eti.p, n_leadin, mask, e, c->stream))) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));               // (the caller's frames have been read)
    return DABGPU_OK;
}

}  // extern "C"
