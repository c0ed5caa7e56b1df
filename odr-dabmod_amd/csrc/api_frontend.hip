// api_frontend.hip -- the front-end on the device (include/dabgpu.h, "the front-end on the device"): the layout of an ETI(NI)
// frame (host only), configure / reset, ETI -> coded bits, ETI -> IQ.  The kernels are in frontend.hip; the stream state (the
// time interleaver's fifteen frames of history) lives in dabgpu_ctx::d_fe_hist: read into a host blob, installed from one,
// or computed from the ETI frames in front of a position of the stream (dabgpu_frontend_seed).
#include "dabgpu_ctx.h"

using namespace dabgpu;
using namespace dabgpu_api;

namespace {

#include "../host/protection_tables.inc"

struct Refused {
    std::string what;
};

// SubchannelSource::SubchannelSource (src/SubchannelSource.cpp:84-163,657-688; host/Frontend.cpp): protection profile -> rules
// and size.  size_t arithmetic in the reference's order, wrap-around included: a profile whose block count goes "negative"
// is refused by the size checks below exactly where the CPU puncturer refuses it.
struct Profile {
    std::vector<std::pair<size_t, uint32_t>> rules;     // (length in bytes of mother-code output, pattern)
    size_t cu = 0xffff;
};

Profile subchannel_profile(size_t stl, size_t tpl)
{
    Profile p;
    const size_t framesize = stl * 8, br = framesize / 3;
    auto rule = [&](size_t blocks, int pi) { p.rules.emplace_back(blocks * 16, kPuncturingVector[pi]); };
    const bool eep = (tpl >> 5) & 1;
    const size_t level = eep ? (tpl & 3) + 1 : (tpl & 7) + 1, option = eep ? (tpl >> 2) & 7 : 0;
    if (eep) {
        if (option == 0) {
            switch (level) {
                case 1: rule(6 * br / 8 - 3, 24); rule(3, 23); p.cu = (br / 8) * 12; break;
                case 2:
                    if (br == 8) { rule(5, 13); rule(1, 12); } else { rule(2 * br / 8 - 3, 14); rule(4 * br / 8 + 3, 13); }
                    p.cu = (br / 8) * 8;
                    break;
                case 3: rule(6 * br / 8 - 3, 8); rule(3, 7); p.cu = (br / 8) * 6; break;
                case 4: rule(4 * br / 8 - 3, 3); rule(2 * br / 8 + 3, 2); p.cu = (br / 8) * 4; break;
                default: throw Refused{"SubchannelSource::SubchannelSource unknown protection level!"};
            }
        } else if (option == 1) {
            static const int pi_body[4] = {10, 6, 4, 2}, pi_end[4] = {9, 5, 3, 1};
            static const size_t cu[4] = {27, 21, 18, 15};
            rule(24 * br / 32 - 3, pi_body[level - 1]);
            rule(3, pi_end[level - 1]);
            p.cu = (br / 32) * cu[level - 1];
        } else {
            throw Refused{"SubchannelSource::SubchannelSource unknown protection option!"};
        }
    } else {
        const UepProfile *q = nullptr;
        for (const UepProfile &u : kUepProfiles)
            if (u.bitrate == br && u.level == level) q = &u;
        if (!q) throw Refused{"SubchannelSource UEP puncturing rules do not exist!"};
        for (int i = 0; i < q->nrules; ++i) rule(q->l[i], q->pi[i]);
        p.cu = q->cu;
    }
    return p;
}

// PuncturingEncoder::adjust_item_size and the checks at the top of ::process (src/PuncturingEncoder.cpp:60-65,125-139):
// fills rule[] / n_rules, returns whether the padding byte of EN 300 401 table 31 follows
bool punctured_size(const std::vector<std::pair<size_t, uint32_t>> &rules, size_t in_len, size_t num_cu, dabgpu_fe_rule *out,
                    uint32_t *n_out, size_t *out_bytes)
{
    size_t in_size = 3, out_bits = (size_t)__builtin_popcount(0xcccccc);
    for (const auto &r : rules) {
        const size_t groups = (r.first + 3) / 4;
        in_size += 4 * groups;
        out_bits += groups * (size_t)__builtin_popcount(r.second);
    }
    size_t block = (out_bits + 7) / 8;
    bool padding = false;
    if (num_cu > 0) {
        if (num_cu * 8 == block + 1) padding = true;
        else if (num_cu * 8 != block)
            throw Refused{"PuncturingEncoder encoder initialisation failed.  CU: " + std::to_string(num_cu) +
                          " block_size: " + std::to_string(block)};
        block = num_cu * 8;
    }
    if (in_size != in_len || rules.empty() || rules.size() > DABGPU_FE_MAX_RULES)
        throw Refused{"PuncturingEncoder::process wrong input size"};
    *n_out = (uint32_t)rules.size();
    for (size_t i = 0; i < rules.size(); ++i) out[i] = {(uint32_t)((rules[i].first + 3) / 4), rules[i].second};
    *out_bytes = block;
    return padding;
}

void describe(const uint8_t *f, dabgpu_fe_layout *L)
{
    std::memset(L, 0, sizeof *L);
    const unsigned ficf = f[5] >> 7, nst = f[5] & 0x7f, mid = (f[6] >> 3) & 3;
    if (!ficf) throw Refused{"FIC must be present to modulate!"};                 // EtiReader::loadEtiData
    L->mode = mid ? mid : 4;
    L->nst = nst;
    // FicSource (src/FicSource.cpp:51-59): 3 or 4 FIBs per 24 ms at code rate 1/3
    const size_t fibs = mid == 3 ? 4 : 3;
    L->fic_bytes = (uint32_t)(32 * fibs);
    L->fic_offset = 12 + 4 * nst;
    L->tail_bytes = 3;
    L->tail_pattern = 0xcccccc;
    size_t fic_out = 0;
    punctured_size({{(8 * fibs - 3) * 16, kPuncturingVector[16]}, {3 * 16, kPuncturingVector[15]}}, 4 * L->fic_bytes + 3, 0,
                   L->fic_rule, &L->fic_n_rules, &fic_out);
    std::vector<Profile> prof;
    size_t offset = L->fic_offset + L->fic_bytes, payload = 0;
    for (unsigned i = 0; i < nst; ++i) {                                             // SubchannelSource, in STC order
        const uint8_t *s = f + 8 + 4 * i;
        dabgpu_fe_subch &sc = L->sub[i];
        sc.sad = ((s[0] & 3u) << 8) | s[1];
        sc.stl = ((s[2] & 3u) << 8) | s[3];
        sc.tpl = s[2] >> 2;
        sc.framesize = 8 * sc.stl;
        sc.offset = (uint32_t)offset;
        offset += sc.framesize;
        payload += sc.framesize;
        prof.push_back(subchannel_profile(sc.stl, sc.tpl));
    }
    // the header against the frame (host/Frontend.cpp, EtiReader::loadEtiData): EOH, FIC, MST, EOF, TIST
    if (4 + L->fic_bytes + payload + 8 > 6144 - 8 - 4 * (size_t)nst)
        throw Refused{"EtiReader: stream characterisation exceeds the 6144-byte ETI frame"};
    for (unsigned i = 0; i < nst; ++i) {                                             // SubchannelSource::framesizeCu
        if (prof[i].cu == 0) throw Refused{"SubchannelSource::framesizeCu protection not yet coded!"};
        if (prof[i].cu == 0xffff) throw Refused{"SubchannelSource::framesizeCu invalid protection!"};
    }
    for (unsigned i = 0; i < nst; ++i) {                                             // PuncturingEncoder::process
        dabgpu_fe_subch &sc = L->sub[i];
        size_t out_bytes = 0;
        sc.padding_byte = punctured_size(prof[i].rules, 4 * (size_t)sc.framesize + 3, prof[i].cu, sc.rule, &sc.n_rules, &out_bytes);
        sc.cu = (uint32_t)prof[i].cu;
    }
    for (unsigned i = 0; i < nst; ++i)                                               // FrameMultiplexer::process
        if ((size_t)L->sub[i].sad * 8 + (size_t)L->sub[i].cu * 8 > 864 * 8)
            throw Refused{"FrameMultiplexer: sub-channel beyond the end of the CIF"};
}

int cifs_of_mode(int mode) { return mode == 1 ? 4 : mode == 4 ? 2 : 1; }

// one unit's segment table: where each run of groups under one pattern starts in the output, the tail behind them
FeUnit make_unit(const dabgpu_fe_rule *rule, uint32_t n_rules, uint32_t in_off, uint32_t in_bytes, uint32_t out_bytes,
                 uint32_t dst_off, int owner)
{
    FeUnit u{};
    u.in_off = in_off; u.in_bytes = in_bytes; u.out_bytes = out_bytes; u.dst_off = dst_off; u.owner = owner;
    u.nseg = n_rules;
    uint32_t g = 0, bit = 0;
    for (uint32_t r = 0; r < n_rules; ++r) {
        u.g0[r] = g; u.base[r] = bit; u.pat[r] = rule[r].pattern;
        g += rule[r].groups;
        bit += rule[r].groups * (uint32_t)__builtin_popcount(rule[r].pattern);
    }
    u.g0[n_rules] = g; u.base[n_rules] = bit; u.pat[n_rules] = 0xcccccc00u;         // the 24-bit tail rule, left-aligned
    u.g0[n_rules + 1] = g + 1;
    return u;
}

// the start of a stream: rows 0 ... 14 of the history are zero (TimeInterleaver's ring at construction).  configure zeroes
// the rows behind them too (`rows` in all): a call writes only the capacity units a sub-channel owns, so every other byte
// of every row is zero from then on, whichever way the rows were filled -- what makes two front-end state blobs taken at
// the same position of a stream equal byte for byte.
hipError_t zero_history(dabgpu_ctx *c, size_t rows = kFeHistory)
{
    const hipError_t e = hipMemsetAsync(c->d_fe_hist.p, 0, rows * kFeCifBytes, c->stream);
    return e != hipSuccess ? e : hipStreamSynchronize(c->stream);
}

const char *const kNotConfigured = "frontend: not configured (dabgpu_frontend_configure comes first)";

// the front-end state blob's header (include/dabgpu.h documents the layout); the fifteen history rows follow, oldest first
struct FeStateHeader {
    uint32_t magic, version, mode, fc, rows, row_bytes, nst, reserved;
    uint8_t stc[4 * DABGPU_FE_MAX_SUBCH];
};
static_assert(sizeof(FeStateHeader) == DABGPU_FE_STATE_HEADER_BYTES && kFeHistory == DABGPU_FE_HISTORY_FRAMES,
              "the layout include/dabgpu.h documents");
constexpr size_t kFeStateBytes = sizeof(FeStateHeader) + (size_t)kFeHistory * kFeCifBytes;

// what frontend_check_host compares, as the blob carries it: FICF / NST, the MID bits, the NST STC words
FeStateHeader state_header(const dabgpu_ctx *c)
{
    FeStateHeader h{};
    h.magic = DABGPU_FE_STATE_MAGIC;
    h.version = DABGPU_FE_STATE_VERSION;
    h.mode = (uint32_t)(c->g.mode ? c->g.mode : 4);
    h.fc = (uint32_t)c->fe_header[0] | (uint32_t)c->fe_header[1] << 8;
    h.rows = kFeHistory;
    h.row_bytes = kFeCifBytes;
    h.nst = c->fe_layout.nst;
    std::memcpy(h.stc, c->fe_header.data() + 3, 4 * (size_t)h.nst);
    return h;
}

}  // namespace

namespace dabgpu_api {

int frontend_check_shape(dabgpu_ctx *c, size_t n_eti, size_t *n_tf)
{
    if (!c->fe_configured) return fail(c, DABGPU_E_INVALID, kNotConfigured);
    if (n_eti % (size_t)c->fe_cifs)
        return fail(c, DABGPU_E_INVALID, "frontend: ETI frames come as whole transmission frames (a multiple of " +
                                             std::to_string(c->fe_cifs) + " in this mode)");
    *n_tf = n_eti / (size_t)c->fe_cifs;
    if (*n_tf > (size_t)c->max_frames) return fail(c, DABGPU_E_CAPACITY, "n_frames exceeds max_frames of the context");
    return DABGPU_OK;
}

int frontend_check_host(dabgpu_ctx *c, const uint8_t *eti, size_t n_eti)
{
    if (!eti && n_eti) return fail(c, DABGPU_E_INVALID, "null argument");
    if (n_eti && (eti[6] >> 5) % (unsigned)c->fe_cifs)
        return fail(c, DABGPU_E_INVALID, "frontend: the frame phase of a call's first frame must be a multiple of " +
                                             std::to_string(c->fe_cifs) + " (FP = " + std::to_string(eti[6] >> 5) + ")");
    return frontend_check_layout(c, eti, n_eti);
}

int frontend_check_layout(dabgpu_ctx *c, const uint8_t *eti, size_t n_eti)
{
    const std::vector<uint8_t> &h = c->fe_header;
    const size_t nst = c->fe_layout.nst;
    for (size_t k = 0; k < n_eti; ++k) {
        const uint8_t *f = eti + k * 6144;
        if (!(f[5] >> 7)) return fail(c, DABGPU_E_INVALID, "FIC must be present to modulate!");
        if ((f[5] & 0x7fu) != nst)
            return fail(c, DABGPU_E_INVALID, "FrameMultiplexer detected subchannel size change from " + std::to_string(nst) +
                                                 " to " + std::to_string(f[5] & 0x7fu));
        if ((f[6] & 0x18) != h[1] || std::memcmp(f + 8, h.data() + 3, 4 * nst) != 0)
            return fail(c, DABGPU_E_INVALID, "FrameMultiplexer detected a multiplex reconfiguration");
    }
    return DABGPU_OK;
}

int run_frontend(dabgpu_ctx *c, const void *d_eti, size_t n_eti, void *d_bits, hipStream_t s)
{
    if (!n_eti) return DABGPU_OK;
    HIPCHK(c, c->d_fe_fic.reserve(n_eti * (size_t)c->fe_fic_out));
    FeArgs a{};
    a.eti = (const uint8_t *)d_eti;
    a.prbs = (const uint8_t *)c->d_fe_prbs.p;
    a.units = (const FeUnit *)c->d_fe_units.p;
    a.owner = (const int16_t *)c->d_fe_owner.p;
    a.hist = (uint8_t *)c->d_fe_hist.p;
    a.fic = (uint8_t *)c->d_fe_fic.p;
    a.out = (uint8_t *)d_bits;
    a.n_eti = (int)n_eti; a.n_units = c->fe_units; a.cifs = c->fe_cifs; a.fic_out = c->fe_fic_out;
    a.unit0 = 0; a.row0 = kFeHistory;
    HIPCHK(c, launch_fe_encode(a, s));
    HIPCHK(c, launch_fe_assemble(a, s));
    // the last fifteen rows of the call move to the front, in stream order (through a second buffer where they overlap)
    const size_t hist = (size_t)kFeHistory * kFeCifBytes;
    const uint8_t *last = a.hist + n_eti * kFeCifBytes;
    if (n_eti >= (size_t)kFeHistory) {
        HIPCHK(c, hipMemcpyAsync(a.hist, last, hist, hipMemcpyDeviceToDevice, s));
    } else {
        HIPCHK(c, hipMemcpyAsync(c->d_fe_tmp.p, last, hist, hipMemcpyDeviceToDevice, s));
        HIPCHK(c, hipMemcpyAsync(a.hist, c->d_fe_tmp.p, hist, hipMemcpyDeviceToDevice, s));
    }
    return DABGPU_OK;
}

int frontend_seed_check(dabgpu_ctx *c, size_t n_leadin, uint64_t e, size_t reach)
{
    if (!c->fe_configured) return fail(c, DABGPU_E_INVALID, kNotConfigured);
    if (e % (uint64_t)c->fe_cifs)
        return fail(c, DABGPU_E_INVALID, "frontend seed: a stream is taken up at a whole transmission frame (e a multiple of " +
                                             std::to_string(c->fe_cifs) + " in this mode)");
    const size_t want = (size_t)std::min<uint64_t>(e, reach);
    if (n_leadin != want)
        return fail(c, DABGPU_E_INVALID, "frontend seed: the lead-in in front of ETI frame " + std::to_string(e) + " is " +
                                             std::to_string(want) + " frames (given: " + std::to_string(n_leadin) + ")");
    return DABGPU_OK;
}

int frontend_check_leadin_host(dabgpu_ctx *c, const uint8_t *eti, size_t n_leadin)
{
    if (!n_leadin) return DABGPU_OK;
    if (!eti) return fail(c, DABGPU_E_INVALID, "null argument");
    const int rc = frontend_check_layout(c, eti, n_leadin);
    if (rc) return rc;
    const unsigned fp = eti[(n_leadin - 1) * 6144 + 6] >> 5, cifs = (unsigned)c->fe_cifs;
    if (fp % cifs != cifs - 1)
        return fail(c, DABGPU_E_INVALID, "frontend seed: the last lead-in frame closes a transmission frame (FP = " +
                                             std::to_string(fp) + ", not " + std::to_string(cifs - 1) + " modulo " +
                                             std::to_string(cifs) + ")");
    return DABGPU_OK;
}

int frontend_seed_rows(dabgpu_ctx *c, const void *d_eti, size_t m, hipStream_t s)
{
    if (m > (size_t)kFeHistory) return fail(c, DABGPU_E_INVALID, "frontend seed: more lead-in frames than the history holds");
    // rows that lie before the start of the stream are zero, as after configure; the others keep the bytes no sub-channel
    // owns, which are zero since configure and which no launch writes
    if (m < (size_t)kFeHistory) HIPCHK(c, hipMemsetAsync(c->d_fe_hist.p, 0, ((size_t)kFeHistory - m) * kFeCifBytes, s));
    if (!m) return DABGPU_OK;
    FeArgs a{};
    a.eti = (const uint8_t *)d_eti;
    a.prbs = (const uint8_t *)c->d_fe_prbs.p;
    a.units = (const FeUnit *)c->d_fe_units.p;
    a.owner = (const int16_t *)c->d_fe_owner.p;
    a.hist = (uint8_t *)c->d_fe_hist.p;
    a.n_eti = (int)m; a.n_units = c->fe_units; a.cifs = c->fe_cifs; a.fic_out = c->fe_fic_out;
    a.unit0 = 1; a.row0 = kFeHistory - (int)m;
    HIPCHK(c, launch_fe_encode(a, s));
    return DABGPU_OK;
}

}  // namespace dabgpu_api

extern "C" {

int dabgpu_frontend_describe(const uint8_t *frame, dabgpu_fe_layout *out)
{
    if (!frame || !out) return fail(nullptr, DABGPU_E_INVALID, "null argument");
    try {
        describe(frame, out);
    } catch (const Refused &r) {
        return fail(nullptr, DABGPU_E_INVALID, r.what);
    }
    return DABGPU_OK;
}

int dabgpu_frontend_configure(dabgpu_ctx *c, const uint8_t *frame)
{
    CTXCHK(c);
    if (!frame) return fail(c, DABGPU_E_INVALID, "null argument");
    dabgpu_fe_layout L;
    try {
        describe(frame, &L);
    } catch (const Refused &r) {
        return fail(c, DABGPU_E_INVALID, r.what);
    }
    const int ctx_mode = c->g.mode ? c->g.mode : 4;
    if ((int)L.mode != ctx_mode)
        return fail(c, DABGPU_E_INVALID, "frontend: the ETI frame is of transmission mode " + std::to_string(L.mode) +
                                             ", the context of mode " + std::to_string(ctx_mode));
    int rc = dabgpu_synchronize(c);
    if (rc) return rc;
    c->fe_configured = false;
    const int cifs = cifs_of_mode(ctx_mode);
    // units: the FIC, then the sub-channels in STC order; which capacity units each one owns (the last one wins)
    std::vector<FeUnit> units;
    size_t fic_bits = 12;
    for (uint32_t r = 0; r < L.fic_n_rules; ++r) fic_bits += (size_t)L.fic_rule[r].groups * __builtin_popcount(L.fic_rule[r].pattern);
    const uint32_t fic_out = (uint32_t)((fic_bits + 7) / 8);
    if ((size_t)cifs * (fic_out + kFeCifBytes) != tf_in_bytes(c->g) || fic_out % 4)
        return fail(c, DABGPU_E_INVALID, "frontend: the punctured FIC does not fit the mode's transmission frame");
    units.push_back(make_unit(L.fic_rule, L.fic_n_rules, L.fic_offset, L.fic_bytes, fic_out, 0, -1));
    std::vector<int16_t> owner(864, (int16_t)-1);
    for (uint32_t i = 0; i < L.nst; ++i) {
        const dabgpu_fe_subch &sc = L.sub[i];
        units.push_back(make_unit(sc.rule, sc.n_rules, sc.offset, sc.framesize, 8 * sc.cu, 8 * sc.sad, (int)i));
        for (uint32_t cu = sc.sad; cu < sc.sad + sc.cu; ++cu) owner[cu] = (int16_t)i;
    }
    // the dispersal sequence x^9 + x^5 + 1, all ones at the start (PrbsGenerator, src/PrbsGenerator.cpp:58-73,144-153): the
    // register restarts with every frame and unit, so one table serves them all, and the CIF's padding
    std::vector<uint8_t> prbs(kFeCifBytes);
    uint32_t acc = 0x1ff;
    for (auto &b : prbs) {
        for (int k = 0; k < 8; ++k) acc = (acc << 1) ^ (uint32_t)__builtin_parity(acc & 0x110u);
        b = (uint8_t)acc;
    }
    HIPCHK(c, upload(c->d_fe_prbs, prbs, c->stream));
    HIPCHK(c, upload(c->d_fe_units, units, c->stream));
    HIPCHK(c, upload(c->d_fe_owner, owner, c->stream));
    const size_t rows = (size_t)kFeHistory + (size_t)c->max_frames * cifs;
    HIPCHK(c, c->d_fe_hist.reserve(rows * kFeCifBytes));
    HIPCHK(c, c->d_fe_tmp.reserve((size_t)kFeHistory * kFeCifBytes));
    HIPCHK(c, zero_history(c, rows));
    c->fe_layout = L;
    c->fe_units = (int)units.size();
    c->fe_cifs = cifs;
    c->fe_fic_out = (int)fic_out;
    c->fe_header.assign(frame + 5, frame + 8 + 4 * L.nst);
    c->fe_header[1] &= 0x18;
    c->fe_configured = true;
    return decode_configure(c);                                      // (the channel decoder's history belongs to the layout too)
}

int dabgpu_frontend_reset(dabgpu_ctx *c)
{
    CTXCHK(c);
    if (!c->fe_configured) return fail(c, DABGPU_E_INVALID, kNotConfigured);
    int rc = dabgpu_synchronize(c);
    if (rc) return rc;
    HIPCHK(c, zero_history(c));
    return DABGPU_OK;
}

size_t dabgpu_frontend_state_bytes(const dabgpu_ctx *c) { return c ? kFeStateBytes : 0; }

int dabgpu_frontend_get_state(dabgpu_ctx *c, void *buf, size_t cap, size_t *bytes)
{
    CTXCHK(c);
    if (!buf) return fail(c, DABGPU_E_INVALID, "null argument");
    if (!c->fe_configured) return fail(c, DABGPU_E_INVALID, kNotConfigured);
    const int rc = dabgpu_synchronize(c);
    if (rc) return rc;
    if (bytes) *bytes = kFeStateBytes;
    if (kFeStateBytes > cap) return fail(c, DABGPU_E_CAPACITY, "frontend state: buffer too small");
    const FeStateHeader h = state_header(c);
    std::memcpy(buf, &h, sizeof h);
    HIPCHK(c, hipMemcpy((char *)buf + sizeof h, c->d_fe_hist.p, (size_t)kFeHistory * kFeCifBytes, hipMemcpyDeviceToHost));
    return DABGPU_OK;
}

int dabgpu_frontend_set_state(dabgpu_ctx *c, const void *buf, size_t bytes)
{
    CTXCHK(c);
    if (!buf) return fail(c, DABGPU_E_INVALID, "null argument");
    if (!c->fe_configured) return fail(c, DABGPU_E_INVALID, kNotConfigured);
    const int rc = dabgpu_synchronize(c);
    if (rc) return rc;
    FeStateHeader h;
    if (bytes < sizeof h) return fail(c, DABGPU_E_INVALID, "frontend state: shorter than its header");
    std::memcpy(&h, buf, sizeof h);
    if (h.magic != DABGPU_FE_STATE_MAGIC) return fail(c, DABGPU_E_INVALID, "frontend state: not a front-end state (magic)");
    if (h.version != DABGPU_FE_STATE_VERSION) return fail(c, DABGPU_E_INVALID, "frontend state: unknown version");
    if (bytes != kFeStateBytes || h.rows != (uint32_t)kFeHistory || h.row_bytes != (uint32_t)kFeCifBytes || h.reserved)
        return fail(c, DABGPU_E_INVALID, "frontend state: size does not match its header");
    const FeStateHeader mine = state_header(c);
    if (h.mode != mine.mode) return fail(c, DABGPU_E_INVALID, "frontend state: taken in another transmission mode");
    if (h.fc != mine.fc || h.nst != mine.nst || std::memcmp(h.stc, mine.stc, sizeof h.stc) != 0)
        return fail(c, DABGPU_E_INVALID, "frontend state: taken on another multiplex layout");
    HIPCHK(c, hipMemcpy(c->d_fe_hist.p, (const char *)buf + sizeof h, (size_t)kFeHistory * kFeCifBytes, hipMemcpyHostToDevice));
    return DABGPU_OK;
}

int dabgpu_frontend_seed_dev(dabgpu_ctx *c, const void *d_eti_leadin, size_t n_leadin, uint64_t e, void *stream)
{
    CTXCHK(c);
    int rc = frontend_seed_check(c, n_leadin, e, kFeHistory);
    if (rc) return rc;
    if (n_leadin && !d_eti_leadin) return fail(c, DABGPU_E_INVALID, "null argument");
    if (!stream && (rc = own_stream_joins_lanes(c))) return rc;
    return frontend_seed_rows(c, d_eti_leadin, n_leadin, stream ? (hipStream_t)stream : c->stream);
}

int dabgpu_frontend_seed(dabgpu_ctx *c, const uint8_t *eti_leadin, size_t n_leadin, uint64_t e)
{
    CTXCHK(c);
    int rc = frontend_seed_check(c, n_leadin, e, kFeHistory);
    if (rc) return rc;
    if ((rc = frontend_check_leadin_host(c, eti_leadin, n_leadin))) return rc;
    if ((rc = own_stream_joins_lanes(c))) return rc;
    HostIO io(c);
    if ((rc = io.in(c->d_fe_eti, eti_leadin, n_leadin * 6144))) return rc;
    if ((rc = frontend_seed_rows(c, c->d_fe_eti.p, n_leadin, c->stream))) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));               // (the caller's frames have been read)
    return DABGPU_OK;
}

int dabgpu_frontend_process_dev(dabgpu_ctx *c, const void *d_eti, size_t n_eti, void *d_bits, size_t out_cap, size_t *out_bytes,
                                void *stream)
{
    CTXCHK(c);
    size_t n_tf = 0;
    int rc = frontend_check_shape(c, n_eti, &n_tf);
    if (rc) return rc;
    if ((rc = check_out(c, n_tf * tf_in_bytes(c->g), out_cap, out_bytes))) return rc;
    if (!n_eti) return DABGPU_OK;
    if (!d_eti || !d_bits) return fail(c, DABGPU_E_INVALID, "null argument");
    if ((uintptr_t)d_bits & 3) return fail(c, DABGPU_E_INVALID, "frontend: the output is written as 32-bit words (4-byte alignment)");
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    if (!stream && (rc = own_stream_joins_lanes(c))) return rc;
    return run_frontend(c, d_eti, n_eti, d_bits, s);
}

int dabgpu_frontend_process(dabgpu_ctx *c, const uint8_t *eti, size_t n_eti, void *bits, size_t out_cap, size_t *out_bytes)
{
    CTXCHK(c);
    size_t n_tf = 0;
    int rc = frontend_check_shape(c, n_eti, &n_tf);
    if (rc) return rc;
    if ((rc = frontend_check_host(c, eti, n_eti))) return rc;
    const size_t need = n_tf * tf_in_bytes(c->g);
    if ((rc = check_out(c, need, out_cap, out_bytes))) return rc;
    if (!n_eti) return DABGPU_OK;
    HIPCHK(c, c->d_in.reserve(std::max<size_t>(need, 16)));
    HostIO io(c);
    if ((rc = io.in(c->d_fe_eti, eti, n_eti * 6144))) return rc;
    if ((rc = run_frontend(c, c->d_fe_eti.p, n_eti, c->d_in.p, c->stream))) return rc;
    return io.out(bits, c->d_in.p, need);
}

int dabgpu_chain_process_eti(dabgpu_ctx *c, const uint8_t *eti, size_t n_eti, unsigned mask, void *iq_out, size_t out_cap,
                             size_t *out_bytes)
{
    CTXCHK(c);
    size_t n_tf = 0;
    int rc = frontend_check_shape(c, n_eti, &n_tf);
    if (rc) return rc;
    if ((rc = frontend_check_host(c, eti, n_eti))) return rc;
    c->clip_from_collect = false;
    if ((rc = apply_settings(c))) return rc;
    const ChainPlan p = plan_chain(c, true, n_tf, mask, true, true, chain_cic(c));
    if (p.error) return fail(c, DABGPU_E_INVALID, p.error);          // (before the front-end advances its history)
    if (const char *why = monitor_refusal(c, p)) return fail(c, DABGPU_E_INVALID, why);
    const size_t need = p.out_bytes;
    if ((rc = check_out(c, need, out_cap, out_bytes))) return rc;
    HIPCHK(c, c->d_in.reserve(std::max<size_t>(n_tf * tf_in_bytes(c->g), 16)));
    HIPCHK(c, c->d_out.reserve(std::max<size_t>(need, 16)));
    HostIO io(c);
    if ((rc = io.in(c->d_fe_eti, eti, n_eti * 6144))) return rc;
    if ((rc = run_frontend(c, c->d_fe_eti.p, n_eti, c->d_in.p, c->stream))) return rc;
    size_t ob = 0;
    {
        TraceScope trace(c->trace_enabled ? &c->last_variant : nullptr);
        rc = run_chain(c, p, c->d_in.p, c->d_out.p, need, &ob, c->stream);
        if (!rc) rc = run_monitor(c, p, c->d_in.p, c->d_out.p, c->stream);
        if (!rc) rc = run_spectrum_monitor(c, p, c->d_out.p, c->stream);
    }
    if (rc) return rc;
    return io.out(iq_out, c->d_out.p, need);
}

int dabgpu_chain_submit_eti(dabgpu_ctx *c, const uint8_t *eti, size_t n_eti, unsigned mask)
{
    CTXCHK(c);
    size_t n_tf = 0;
    int rc = frontend_check_shape(c, n_eti, &n_tf);
    if (rc) return rc;
    if ((rc = frontend_check_host(c, eti, n_eti))) return rc;
    return chain_submit(c, eti, n_tf, mask, true);
}

}  // extern "C"
