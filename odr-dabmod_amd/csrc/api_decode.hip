// api_decode.hip -- the channel decoder of decode.hip behind the C-ABI (include/dabgpu.h, "the channel decoder"): coded bits in
// the chain's input layout -> the ETI payload, per (frame, unit) figures.  The reference has no receiver: nothing here replaces
// a plugin of its flowgraph, which is why no entry is named *_process.  The layout is the front-end's (dabgpu_frontend_configure);
// the stream state is the last fifteen received rows, dabgpu_ctx::d_dec_rows.
#include "dabgpu_ctx.h"

using namespace dabgpu;
using namespace dabgpu_api;

namespace {

const char *const kDecNotConfigured = "decode: not configured (dabgpu_frontend_configure comes first)";

// the first capacity unit two sub-channels of the layout share, or -1
int shared_capacity_unit(const dabgpu_fe_layout &L, unsigned *first, unsigned *second)
{
    int owner[864];
    std::fill(owner, owner + 864, -1);
    for (unsigned i = 0; i < L.nst && i < DABGPU_FE_MAX_SUBCH; ++i)
        for (unsigned cu = L.sub[i].sad; cu < L.sub[i].sad + L.sub[i].cu && cu < 864; ++cu) {
            if (owner[cu] >= 0) {
                *first = (unsigned)owner[cu];
                *second = i;
                return (int)cu;
            }
            owner[cu] = (int)i;
        }
    return -1;
}

std::string overlap_message(const dabgpu_fe_layout &L)
{
    unsigned a = 0, b = 0;
    const int cu = shared_capacity_unit(L, &a, &b);
    if (cu < 0) return std::string();
    return "decode: sub-channels " + std::to_string(a) + " and " + std::to_string(b) + " of the STC list overlap at capacity unit " +
           std::to_string(cu) + " (the bits of the earlier one were never transmitted there)";
}

size_t dec_row_bytes(const dabgpu_ctx *c) { return (size_t)c->fe_fic_out + kFeCifBytes; }

// every refusal of a call, before anything is queued
int check_decode(dabgpu_ctx *c, size_t n_tf, size_t out_cap, size_t *out_bytes)
{
    if (!c->fe_configured) return fail(c, DABGPU_E_INVALID, kDecNotConfigured);
    if (!c->dec_refusal.empty()) return fail(c, DABGPU_E_INVALID, c->dec_refusal);
    if (!n_tf) return fail(c, DABGPU_E_INVALID, "decode: n_tf is at least one transmission frame");
    if (n_tf > (size_t)c->max_frames) return fail(c, DABGPU_E_CAPACITY, "n_frames exceeds max_frames of the context");
    return check_out(c, n_tf * (size_t)c->fe_cifs * 6144, out_cap, out_bytes);
}

// the buffers of the first use: rows, survivor scratch and records for max_frames transmission frames
int reserve_decode(dabgpu_ctx *c)
{
    const size_t max_out = (size_t)c->max_frames * (size_t)c->fe_cifs;
    HIPCHK(c, c->d_dec_rows.reserve(((size_t)kFeHistory + max_out) * dec_row_bytes(c)));
    HIPCHK(c, c->d_dec_tmp.reserve((size_t)kFeHistory * dec_row_bytes(c)));
    HIPCHK(c, c->d_dec_surv.reserve(std::max<size_t>(max_out * c->dec_slot.back() * sizeof(unsigned long long), 16)));
    HIPCHK(c, c->d_dec_stats.reserve(max_out * (size_t)c->fe_units * sizeof(DecUnitStats)));
    return DABGPU_OK;
}

int queue_decode(dabgpu_ctx *c, const void *d_bits, size_t n_tf, void *d_out, const void *d_ref, hipStream_t s)
{
    int rc = reserve_decode(c);
    if (rc) return rc;
    const size_t n = n_tf * (size_t)c->fe_cifs, row = dec_row_bytes(c), hist = (size_t)kFeHistory * row;
    if (c->dec_zero_pending) {
        // (the slot table travels with the zero history: both belong to the layout)
        HIPCHK(c, upload(c->d_dec_slot, c->dec_slot, s));
        HIPCHK(c, hipMemsetAsync(c->d_dec_rows.p, 0, hist, s));
        c->dec_zero_pending = false;
    }
    HIPCHK(c, hipMemsetAsync(d_out, 0, n * 6144, s));
    DecArgs a{};
    a.bits = (const uint8_t *)d_bits;
    a.rows = (uint8_t *)c->d_dec_rows.p;
    a.prbs = (const uint8_t *)c->d_fe_prbs.p;
    a.units = (const FeUnit *)c->d_fe_units.p;
    a.slot = (const uint32_t *)c->d_dec_slot.p;
    a.surv = (unsigned long long *)c->d_dec_surv.p;
    a.out = (uint8_t *)d_out;
    a.ref = (const uint8_t *)d_ref;
    a.stats = (DecUnitStats *)c->d_dec_stats.p;
    a.n_out = (int)n; a.n_units = c->fe_units; a.cifs = c->fe_cifs; a.fic_out = c->fe_fic_out;
    for (size_t u = 0; u + 1 < c->dec_slot.size(); ++u) a.sym_bytes = std::max(a.sym_bytes, (int)(c->dec_slot[u + 1] - c->dec_slot[u]));
    const unsigned long long lead = c->dec_pos < (unsigned long long)kFeHistory ? (unsigned long long)kFeHistory - c->dec_pos : 0;
    a.first_valid = (int)std::min<unsigned long long>(lead, n);
    HIPCHK(c, launch_dec_rows(a, s));
    HIPCHK(c, launch_dec_decode(a, s));
    // the last fifteen rows move to the front, in stream order (through a second buffer where they overlap)
    const uint8_t *last = a.rows + n * row;
    if (n >= (size_t)kFeHistory) {
        HIPCHK(c, hipMemcpyAsync(a.rows, last, hist, hipMemcpyDeviceToDevice, s));
    } else {
        HIPCHK(c, hipMemcpyAsync(c->d_dec_tmp.p, last, hist, hipMemcpyDeviceToDevice, s));
        HIPCHK(c, hipMemcpyAsync(a.rows, c->d_dec_tmp.p, hist, hipMemcpyDeviceToDevice, s));
    }
    c->dec_pos += n;
    c->dec_frames = n;
    c->dec_first_valid = (size_t)a.first_valid;
    c->dec_stream = s;
    return DABGPU_OK;
}

// ---- the soft decoder: the same call on int8 metrics and on a history of its own (eight bytes where the hard one has one)
int queue_decode_soft(dabgpu_ctx *c, const void *d_soft, size_t n_tf, void *d_out, const void *d_ref, hipStream_t s)
{
    const size_t max_out = (size_t)c->max_frames * (size_t)c->fe_cifs;
    const size_t n = n_tf * (size_t)c->fe_cifs, row = 8 * dec_row_bytes(c), hist = (size_t)kFeHistory * row;
    HIPCHK(c, c->d_decs_rows.reserve(((size_t)kFeHistory + max_out) * row));
    HIPCHK(c, c->d_decs_tmp.reserve(hist));
    HIPCHK(c, c->d_dec_surv.reserve(std::max<size_t>(max_out * c->dec_slot.back() * sizeof(unsigned long long), 16)));
    HIPCHK(c, c->d_decs_stats.reserve(max_out * (size_t)c->fe_units * sizeof(DecSoftUnitStats)));
    if (c->decs_zero_pending) {
        HIPCHK(c, upload(c->d_dec_slot, c->dec_slot, s));
        HIPCHK(c, hipMemsetAsync(c->d_decs_rows.p, 0, hist, s));
        c->decs_zero_pending = false;
    }
    HIPCHK(c, hipMemsetAsync(d_out, 0, n * 6144, s));
    DecSoftArgs a{};
    a.soft = (const int8_t *)d_soft;
    a.rows = (int8_t *)c->d_decs_rows.p;
    a.prbs = (const uint8_t *)c->d_fe_prbs.p;
    a.units = (const FeUnit *)c->d_fe_units.p;
    a.slot = (const uint32_t *)c->d_dec_slot.p;
    a.surv = (unsigned long long *)c->d_dec_surv.p;
    a.out = (uint8_t *)d_out;
    a.ref = (const uint8_t *)d_ref;
    a.stats = (DecSoftUnitStats *)c->d_decs_stats.p;
    a.n_out = (int)n; a.n_units = c->fe_units; a.cifs = c->fe_cifs; a.fic_out = c->fe_fic_out;
    unsigned out_bytes = (unsigned)c->fe_fic_out;
    for (uint32_t i = 0; i < c->fe_layout.nst; ++i) out_bytes = std::max(out_bytes, 8u * (unsigned)c->fe_layout.sub[i].cu);
    a.lds_bytes = (int)(8 * out_bytes);
    const unsigned long long lead = c->decs_pos < (unsigned long long)kFeHistory ? (unsigned long long)kFeHistory - c->decs_pos : 0;
    a.first_valid = (int)std::min<unsigned long long>(lead, n);
    HIPCHK(c, launch_dec_soft_rows(a, s));
    HIPCHK(c, launch_dec_soft_decode(a, s));
    const int8_t *last = a.rows + n * row;
    if (n >= (size_t)kFeHistory) {
        HIPCHK(c, hipMemcpyAsync(a.rows, last, hist, hipMemcpyDeviceToDevice, s));
    } else {
        HIPCHK(c, hipMemcpyAsync(c->d_decs_tmp.p, last, hist, hipMemcpyDeviceToDevice, s));
        HIPCHK(c, hipMemcpyAsync(a.rows, c->d_decs_tmp.p, hist, hipMemcpyDeviceToDevice, s));
    }
    c->decs_pos += n;
    c->decs_frames = n;
    c->decs_first_valid = (size_t)a.first_valid;
    c->decs_stream = s;
    return DABGPU_OK;
}

}  // namespace

namespace dabgpu_api {

int decode_configure(dabgpu_ctx *c)
{
    c->dec_refusal = overlap_message(c->fe_layout);
    // a unit's slot: its trellis steps rounded up to 64 survivor words (the kernel stores 64 at a time)
    std::vector<uint32_t> slot(1, 0u);
    auto add = [&](uint32_t in_bytes) { slot.push_back(slot.back() + (8 * in_bytes + 6 + 63) / 64 * 64); };
    add(c->fe_layout.fic_bytes);
    for (uint32_t i = 0; i < c->fe_layout.nst; ++i) add(c->fe_layout.sub[i].framesize);
    c->dec_slot = slot;
    c->dec_pos = 0;
    c->dec_zero_pending = true;
    c->dec_frames = 0;
    c->decs_pos = 0;
    c->decs_zero_pending = true;
    c->decs_frames = 0;
    return DABGPU_OK;
}

}  // namespace dabgpu_api

extern "C" {

int dabgpu_decode_check_layout(const dabgpu_fe_layout *layout)
{
    if (!layout) return fail(nullptr, DABGPU_E_INVALID, "null argument");
    if (layout->nst > DABGPU_FE_MAX_SUBCH) return fail(nullptr, DABGPU_E_INVALID, "decode: more sub-channels than the STC list holds");
    const std::string why = overlap_message(*layout);
    if (!why.empty()) return fail(nullptr, DABGPU_E_INVALID, why);
    // (one unit's trellis in the kernel's LDS: a frame's 6144 bytes cannot hold more, asked all the same)
    for (uint32_t i = 0; i < layout->nst; ++i)
        if (8 * (size_t)layout->sub[i].framesize + 6 + 64 > (size_t)kDecMaxSteps)
            return fail(nullptr, DABGPU_E_INVALID, "decode: a sub-channel of more payload than an ETI frame carries");
    return DABGPU_OK;
}

int dabgpu_decode_reset(dabgpu_ctx *c)
{
    CTXCHK(c);
    if (!c->fe_configured) return fail(c, DABGPU_E_INVALID, kDecNotConfigured);
    const int rc = dabgpu_synchronize(c);
    if (rc) return rc;
    c->dec_pos = 0;
    c->dec_zero_pending = true;
    c->decs_pos = 0;
    c->decs_zero_pending = true;
    return DABGPU_OK;
}

int dabgpu_decode_dev(dabgpu_ctx *c, const void *d_bits, size_t n_tf, void *d_eti_out, size_t out_cap, const void *d_ref_eti,
                      size_t *out_bytes, void *stream)
{
    CTXCHK(c);
    int rc = check_decode(c, n_tf, out_cap, out_bytes);
    if (rc) return rc;
    if (!d_bits || !d_eti_out) return fail(c, DABGPU_E_INVALID, "null argument");
    if ((uintptr_t)d_bits & 3) return fail(c, DABGPU_E_INVALID, "decode: the coded bits are read as 32-bit words (4-byte alignment)");
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    if (!stream && (rc = own_stream_joins_lanes(c))) return rc;
    TraceScope trace(c->trace_enabled ? &c->last_variant : nullptr);
    return queue_decode(c, d_bits, n_tf, d_eti_out, d_ref_eti, s);
}

int dabgpu_decode(dabgpu_ctx *c, const uint8_t *bits, size_t n_tf, uint8_t *eti_out, size_t out_cap, const uint8_t *ref_eti,
                  size_t *out_bytes)
{
    CTXCHK(c);
    int rc = check_decode(c, n_tf, out_cap, out_bytes);
    if (rc) return rc;
    if (!bits || !eti_out) return fail(c, DABGPU_E_INVALID, "null argument");
    if ((rc = own_stream_joins_lanes(c))) return rc;
    const size_t need = n_tf * (size_t)c->fe_cifs * 6144;
    HostIO io(c);
    if ((rc = io.in(c->d_dec_in, bits, n_tf * tf_in_bytes(c->g)))) return rc;
    if (ref_eti && (rc = io.in(c->d_dec_ref, ref_eti, need))) return rc;
    HIPCHK(c, c->d_dec_out.reserve(need));
    if ((rc = queue_decode(c, c->d_dec_in.p, n_tf, c->d_dec_out.p, ref_eti ? c->d_dec_ref.p : nullptr, c->stream))) return rc;
    return io.out(eti_out, c->d_dec_out.p, need);
}

int dabgpu_get_decode_stats(dabgpu_ctx *c, size_t frame, int unit, dabgpu_decode_stats *out)
{
    CTXCHK(c);
    if (!out) return fail(c, DABGPU_E_INVALID, "null argument");
    if (frame >= c->dec_frames)
        return fail(c, DABGPU_E_INVALID, "no decoder statistics for this frame (no call yet, or frame index out of range)");
    if (unit < -1 || unit >= c->fe_units) return fail(c, DABGPU_E_INVALID, "decode: unit is -1 (the frame), 0 (the FIC) or 1 + a sub-channel");
    HIPCHK(c, hipStreamSynchronize(c->dec_stream ? c->dec_stream : c->stream));
    std::vector<DecUnitStats> st((size_t)c->fe_units);
    HIPCHK(c, hipMemcpy(st.data(), (const DecUnitStats *)c->d_dec_stats.p + frame * (size_t)c->fe_units,
                        st.size() * sizeof(DecUnitStats), hipMemcpyDeviceToHost));
    std::memset(out, 0, sizeof *out);
    out->valid = frame >= c->dec_first_valid;
    for (int u = unit < 0 ? 0 : unit; u < (unit < 0 ? c->fe_units : unit + 1); ++u) {
        out->corrected += st[u].corrected;
        out->coded_bits += st[u].coded_bits;
        out->bit_errors += st[u].bit_errors;
        out->n_bits += st[u].n_bits;
    }
    return DABGPU_OK;
}

int dabgpu_decode_soft_dev(dabgpu_ctx *c, const void *d_soft, size_t n_tf, void *d_eti_out, size_t out_cap, const void *d_ref_eti,
                           size_t *out_bytes, void *stream)
{
    CTXCHK(c);
    int rc = check_decode(c, n_tf, out_cap, out_bytes);
    if (rc) return rc;
    if (!d_soft || !d_eti_out) return fail(c, DABGPU_E_INVALID, "null argument");
    if ((uintptr_t)d_soft & 3) return fail(c, DABGPU_E_INVALID, "decode: the soft metrics are read as 32-bit words (4-byte alignment)");
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    if (!stream && (rc = own_stream_joins_lanes(c))) return rc;
    TraceScope trace(c->trace_enabled ? &c->last_variant : nullptr);
    return queue_decode_soft(c, d_soft, n_tf, d_eti_out, d_ref_eti, s);
}

int dabgpu_decode_soft(dabgpu_ctx *c, const int8_t *soft, size_t n_tf, uint8_t *eti_out, size_t out_cap, const uint8_t *ref_eti,
                       size_t *out_bytes)
{
    CTXCHK(c);
    int rc = check_decode(c, n_tf, out_cap, out_bytes);
    if (rc) return rc;
    if (!soft || !eti_out) return fail(c, DABGPU_E_INVALID, "null argument");
    if ((rc = own_stream_joins_lanes(c))) return rc;
    const size_t need = n_tf * (size_t)c->fe_cifs * 6144;
    HostIO io(c);
    if ((rc = io.in(c->d_decs_in, soft, 8 * n_tf * tf_in_bytes(c->g)))) return rc;
    if (ref_eti && (rc = io.in(c->d_dec_ref, ref_eti, need))) return rc;
    HIPCHK(c, c->d_dec_out.reserve(need));
    if ((rc = queue_decode_soft(c, c->d_decs_in.p, n_tf, c->d_dec_out.p, ref_eti ? c->d_dec_ref.p : nullptr, c->stream))) return rc;
    return io.out(eti_out, c->d_dec_out.p, need);
}

int dabgpu_get_decode_soft_stats(dabgpu_ctx *c, size_t frame, int unit, dabgpu_decode_soft_stats *out)
{
    CTXCHK(c);
    if (!out) return fail(c, DABGPU_E_INVALID, "null argument");
    if (frame >= c->decs_frames)
        return fail(c, DABGPU_E_INVALID, "no soft decoder statistics for this frame (no call yet, or frame index out of range)");
    if (unit < -1 || unit >= c->fe_units) return fail(c, DABGPU_E_INVALID, "decode: unit is -1 (the frame), 0 (the FIC) or 1 + a sub-channel");
    HIPCHK(c, hipStreamSynchronize(c->decs_stream ? c->decs_stream : c->stream));
    std::vector<DecSoftUnitStats> st((size_t)c->fe_units);
    HIPCHK(c, hipMemcpy(st.data(), (const DecSoftUnitStats *)c->d_decs_stats.p + frame * (size_t)c->fe_units,
                        st.size() * sizeof(DecSoftUnitStats), hipMemcpyDeviceToHost));
    std::memset(out, 0, sizeof *out);
    out->valid = frame >= c->decs_first_valid;
    for (int u = unit < 0 ? 0 : unit; u < (unit < 0 ? c->fe_units : unit + 1); ++u) {
        out->metric += st[u].metric;
        out->contra_sum += st[u].contra_sum;
        out->soft_sum += st[u].soft_sum;
        out->corrected += st[u].corrected;
        out->erasures += st[u].erasures;
        out->coded_bits += st[u].coded_bits;
        out->bit_errors += st[u].bit_errors;
        out->n_bits += st[u].n_bits;
    }
    return DABGPU_OK;
}

}  // extern "C"
