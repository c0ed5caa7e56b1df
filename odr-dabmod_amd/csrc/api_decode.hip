// api_decode.hip -- the channel decoder of decode.hip behind the C-ABI (include/dabgpu.h, "the channel decoder"): coded bits in
// the chain's input layout -> the ETI payload, per (frame, unit) figures.  The reference has no receiver: nothing here replaces
// a plugin of its flowgraph, which is why no entry is named *_process.  The layout is the front-end's (dabgpu_frontend_configure);
// the stream state is the last fifteen received rows of either metric width, DecodeStream::rows.
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

// every refusal of a call, before anything is queued
int check_decode(dabgpu_ctx *c, size_t n_tf, size_t out_cap, size_t *out_bytes)
{
    if (!c->fe_configured) return fail(c, DABGPU_E_INVALID, kDecNotConfigured);
    if (!c->decode.refusal.empty()) return fail(c, DABGPU_E_INVALID, c->decode.refusal);
    if (!n_tf) return fail(c, DABGPU_E_INVALID, "decode: n_tf is at least one transmission frame");
    if (n_tf > (size_t)c->max_frames) return fail(c, DABGPU_E_CAPACITY, "n_frames exceeds max_frames of the context");
    return check_out(c, n_tf * (size_t)c->fe_cifs * 6144, out_cap, out_bytes);
}

// What differs between the two metric widths beside DecodeStream::width and the args struct: the LDS figure (hard: the steps
// of the layout's longest unit; soft: 8 x the punctured bytes of its largest).
int lds_bytes(const DecArgs &, const dabgpu_ctx *c)
{
    int steps = 0;
    const std::vector<uint32_t> &slot = c->decode.slot;
    for (size_t u = 0; u + 1 < slot.size(); ++u) steps = std::max(steps, (int)(slot[u + 1] - slot[u]));
    return steps;
}
int lds_bytes(const DecSoftArgs &, const dabgpu_ctx *c)
{
    unsigned out_bytes = (unsigned)c->fe_fic_out;
    for (uint32_t i = 0; i < c->fe_layout.nst; ++i) out_bytes = std::max(out_bytes, 8u * (unsigned)c->fe_layout.sub[i].cu);
    return (int)(8 * out_bytes);
}

// one call on `s`, for either width (Args: DecArgs on st = decode.hard, DecSoftArgs on decode.soft).  The buffers of the
// first use: rows, survivor scratch and records for max_frames transmission frames.
template <typename Args>
int queue_decode(dabgpu_ctx *c, DecodeStream &st, const void *d_in, size_t n_tf, void *d_out, const void *d_ref, hipStream_t s)
{
    DecodeState &d = c->decode;
    Args a{};
    const size_t max_out = (size_t)c->max_frames * (size_t)c->fe_cifs;
    const size_t n = n_tf * (size_t)c->fe_cifs, row = st.width * ((size_t)c->fe_fic_out + kFeCifBytes), hist = (size_t)kFeHistory * row;
    HIPCHK(c, st.rows.reserve(((size_t)kFeHistory + max_out) * row));
    HIPCHK(c, st.tmp.reserve(hist));
    HIPCHK(c, d.surv.reserve(std::max<size_t>(max_out * d.slot.back() * sizeof(unsigned long long), 16)));
    HIPCHK(c, st.stats.reserve(max_out * (size_t)c->fe_units * sizeof(*a.stats)));
    if (st.zero_pending) {
        // (the slot table travels with the zero history: both belong to the layout)
        HIPCHK(c, upload(d.slot_dev, d.slot, s));
        HIPCHK(c, hipMemsetAsync(st.rows.p, 0, hist, s));
        st.zero_pending = false;
    }
    HIPCHK(c, hipMemsetAsync(d_out, 0, n * 6144, s));
    a.in = (decltype(a.in))d_in;
    a.lds_bytes = lds_bytes(a, c);
    a.rows = (decltype(a.rows))st.rows.p;
    a.prbs = (const uint8_t *)c->d_fe_prbs.p;
    a.units = (const FeUnit *)c->d_fe_units.p;
    a.slot = (const uint32_t *)d.slot_dev.p;
    a.surv = (unsigned long long *)d.surv.p;
    a.out = (uint8_t *)d_out;
    a.ref = (const uint8_t *)d_ref;
    a.stats = (decltype(a.stats))st.stats.p;
    a.n_out = (int)n; a.n_units = c->fe_units; a.cifs = c->fe_cifs; a.fic_out = c->fe_fic_out;
    const unsigned long long lead = st.pos < (unsigned long long)kFeHistory ? (unsigned long long)kFeHistory - st.pos : 0;
    a.first_valid = (int)std::min<unsigned long long>(lead, n);
    HIPCHK(c, launch_dec_rows(a, s));
    HIPCHK(c, launch_dec_decode(a, s));
    // the last fifteen rows move to the front, in stream order (through a second buffer where they overlap)
    const char *last = (const char *)st.rows.p + n * row;
    if (n >= (size_t)kFeHistory) {
        HIPCHK(c, hipMemcpyAsync(st.rows.p, last, hist, hipMemcpyDeviceToDevice, s));
    } else {
        HIPCHK(c, hipMemcpyAsync(st.tmp.p, last, hist, hipMemcpyDeviceToDevice, s));
        HIPCHK(c, hipMemcpyAsync(st.rows.p, st.tmp.p, hist, hipMemcpyDeviceToDevice, s));
    }
    st.pos += n;
    st.frames = n;
    st.first_valid = (size_t)a.first_valid;
    st.stream = s;
    return DABGPU_OK;
}

// the device-pointer entry of either width; `misaligned`: its refusal of an input that is not dword aligned
template <typename Args>
int decode_dev(dabgpu_ctx *c, DecodeStream &st, const char *misaligned, const void *d_in, size_t n_tf, void *d_eti_out, size_t out_cap,
               const void *d_ref_eti, size_t *out_bytes, void *stream)
{
    CTXCHK(c);
    if (int rc = check_decode(c, n_tf, out_cap, out_bytes)) return rc;
    if (!d_in || !d_eti_out) return fail(c, DABGPU_E_INVALID, "null argument");
    if ((uintptr_t)d_in & 3) return fail(c, DABGPU_E_INVALID, misaligned);
    DevCall call(c, stream);
    if (call.rc) return call.rc;
    return queue_decode<Args>(c, st, d_in, n_tf, d_eti_out, d_ref_eti, call.s);
}

// the host-pointer entry of either width
template <typename Args>
int decode_host(dabgpu_ctx *c, DecodeStream &st, const void *in, size_t n_tf, uint8_t *eti_out, size_t out_cap, const uint8_t *ref_eti,
                size_t *out_bytes)
{
    CTXCHK(c);
    int rc = check_decode(c, n_tf, out_cap, out_bytes);
    if (rc) return rc;
    if (!in || !eti_out) return fail(c, DABGPU_E_INVALID, "null argument");
    if ((rc = own_stream_joins_lanes(c))) return rc;
    const size_t need = n_tf * (size_t)c->fe_cifs * 6144;
    HostIO io(c);
    if ((rc = io.in(st.in, in, st.width * n_tf * tf_in_bytes(c->g)))) return rc;
    if (ref_eti && (rc = io.in(c->decode.ref, ref_eti, need))) return rc;
    HIPCHK(c, c->decode.out.reserve(need));
    if ((rc = queue_decode<Args>(c, st, st.in.p, n_tf, c->decode.out.p, ref_eti ? c->decode.ref.p : nullptr, c->stream))) return rc;
    return io.out(eti_out, c->decode.out.p, need);
}

// The statistics getter of either width: the checks, the wait for the call, the frame's records (Unit each) from the device,
// *out zeroed but for `valid`; add(record) sums one unit's record into *out.  `none`: the refusal of a frame without figures
template <typename Unit, typename Out, typename Add>
int get_stats(dabgpu_ctx *c, DecodeStream DecodeState::*which, const char *none, size_t frame, int unit, Out *out, Add add)
{
    CTXCHK(c);
    if (!out) return fail(c, DABGPU_E_INVALID, "null argument");
    const DecodeStream &st = c->decode.*which;
    if (frame >= st.frames) return fail(c, DABGPU_E_INVALID, none);
    if (unit < -1 || unit >= c->fe_units) return fail(c, DABGPU_E_INVALID, "decode: unit is -1 (the frame), 0 (the FIC) or 1 + a sub-channel");
    HIPCHK(c, wait_result(c, st.stream));
    std::vector<Unit> rec((size_t)c->fe_units);
    HIPCHK(c, hipMemcpy(rec.data(), (const Unit *)st.stats.p + frame * (size_t)c->fe_units, rec.size() * sizeof(Unit), hipMemcpyDeviceToHost));
    std::memset(out, 0, sizeof *out);
    out->valid = frame >= st.first_valid;
    for (int u = unit < 0 ? 0 : unit; u < (unit < 0 ? c->fe_units : unit + 1); ++u) add(rec[u]);
    return DABGPU_OK;
}

// both streams back at their start: the next call of each zeroes its history
void reset_streams(dabgpu_ctx *c)
{
    for (DecodeStream *st : {&c->decode.hard, &c->decode.soft}) {
        st->pos = 0;
        st->zero_pending = true;
    }
}

}  // namespace

namespace dabgpu_api {

int decode_configure(dabgpu_ctx *c)
{
    c->decode.refusal = overlap_message(c->fe_layout);
    // a unit's slot: its trellis steps rounded up to 64 survivor words (the kernel stores 64 at a time)
    std::vector<uint32_t> slot(1, 0u);
    auto add = [&](uint32_t in_bytes) { slot.push_back(slot.back() + (8 * in_bytes + 6 + 63) / 64 * 64); };
    add(c->fe_layout.fic_bytes);
    for (uint32_t i = 0; i < c->fe_layout.nst; ++i) add(c->fe_layout.sub[i].framesize);
    c->decode.slot = slot;
    reset_streams(c);
    c->decode.hard.frames = c->decode.soft.frames = 0;
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
    reset_streams(c);
    return DABGPU_OK;
}

int dabgpu_decode_dev(dabgpu_ctx *c, const void *d_bits, size_t n_tf, void *d_eti_out, size_t out_cap, const void *d_ref_eti,
                      size_t *out_bytes, void *stream)
{
    return decode_dev<DecArgs>(c, c->decode.hard, "decode: the coded bits are read as 32-bit words (4-byte alignment)", d_bits, n_tf,
                               d_eti_out, out_cap, d_ref_eti, out_bytes, stream);
}

int dabgpu_decode(dabgpu_ctx *c, const uint8_t *bits, size_t n_tf, uint8_t *eti_out, size_t out_cap, const uint8_t *ref_eti,
                  size_t *out_bytes)
{
    return decode_host<DecArgs>(c, c->decode.hard, bits, n_tf, eti_out, out_cap, ref_eti, out_bytes);
}

int dabgpu_get_decode_stats(dabgpu_ctx *c, size_t frame, int unit, dabgpu_decode_stats *out)
{
    return get_stats<DecUnitStats>(c, &DecodeState::hard, "no decoder statistics for this frame (no call yet, or frame index out of range)",
                                   frame, unit, out, [&](const DecUnitStats &u) {
                                       out->corrected += u.corrected;
                                       out->coded_bits += u.coded_bits;
                                       out->bit_errors += u.bit_errors;
                                       out->n_bits += u.n_bits;
                                   });
}

int dabgpu_decode_soft_dev(dabgpu_ctx *c, const void *d_soft, size_t n_tf, void *d_eti_out, size_t out_cap, const void *d_ref_eti,
                           size_t *out_bytes, void *stream)
{
    return decode_dev<DecSoftArgs>(c, c->decode.soft, "decode: the soft metrics are read as 32-bit words (4-byte alignment)", d_soft, n_tf,
                                   d_eti_out, out_cap, d_ref_eti, out_bytes, stream);
}

int dabgpu_decode_soft(dabgpu_ctx *c, const int8_t *soft, size_t n_tf, uint8_t *eti_out, size_t out_cap, const uint8_t *ref_eti,
                       size_t *out_bytes)
{
    return decode_host<DecSoftArgs>(c, c->decode.soft, soft, n_tf, eti_out, out_cap, ref_eti, out_bytes);
}

int dabgpu_get_decode_soft_stats(dabgpu_ctx *c, size_t frame, int unit, dabgpu_decode_soft_stats *out)
{
    return get_stats<DecSoftUnitStats>(c, &DecodeState::soft,
                                       "no soft decoder statistics for this frame (no call yet, or frame index out of range)", frame, unit, out,
                                       [&](const DecSoftUnitStats &u) {
                                           out->metric += u.metric;
                                           out->contra_sum += u.contra_sum;
                                           out->soft_sum += u.soft_sum;
                                           out->corrected += u.corrected;
                                           out->erasures += u.erasures;
                                           out->coded_bits += u.coded_bits;
                                           out->bit_errors += u.bit_errors;
                                           out->n_bits += u.n_bits;
                                       });
}

}  // extern "C"
