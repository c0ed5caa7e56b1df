// conv_code_check.cpp -- the channel coding the device kernels share (odr-dabmod_amd/csrc/conv_code.h) on the host alone, held
// to the CPU classes of odr-dabmod_amd/host/Frontend.cpp: the mother code against ConvEncoder, keep_bits / spread_bits on every
// puncturing vector, the segment lookup against a linear walk and against PuncturingEncoder, delay_mask against
// TimeInterleaver, and the transmission-frame word to row rule against the layout written out.  No HIP library is linked.
//   c++ -std=c++17 -Iodr-dabmod_amd/csrc -Iodr-dabmod_amd/host -Iinclude tools/conv_code_check.cpp odr-dabmod_amd/host/Frontend.cpp
//       odr-dabmod_amd/host/Buffer.cpp odr-dabmod_amd/host/ModPlugin.cpp                          (tests/test_conv_code_host.py)
#include "conv_code.h"

#include <cstdio>
#include <cstring>
#include <vector>

#include "Frontend.h"

namespace {
#include "protection_tables.inc"

int g_failed = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            if (++g_failed <= 20) std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
        }                                                                  \
    } while (0)

using namespace dabgpu;
constexpr uint32_t kTail = 0xcccccc00u;       // the 24-bit tail rule, left-aligned in 32 bits

uint32_t be32(const uint8_t *p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3]; }

// a unit's segment table from the CPU classes' rules: derived here again, by the arithmetic of api_frontend.hip's make_unit but
// not by its code (that file needs HIP); the tables the library uploads are held by the GPU tests
FeUnit unit_of(const std::vector<PuncturingRule> &rules, uint32_t in_bytes)
{
    FeUnit u{};
    u.in_bytes = in_bytes;
    u.nseg = (uint32_t)rules.size();
    uint32_t g = 0, bit = 0;
    for (uint32_t r = 0; r < u.nseg; ++r) {
        u.g0[r] = g; u.base[r] = bit; u.pat[r] = rules[r].pattern();
        g += (uint32_t)((rules[r].length() + 3) / 4);
        bit += (uint32_t)((rules[r].length() + 3) / 4 * rules[r].bit_size());
    }
    u.g0[u.nseg] = g; u.base[u.nseg] = bit; u.pat[u.nseg] = kTail;
    u.g0[u.nseg + 1] = g + 1;
    u.out_bytes = (bit + 12 + 7) / 8;
    return u;
}

// mother_code over all (previous six bits, byte) pairs, and the tail word, against ConvEncoder on two-byte frames
int check_mother_code()
{
    ConvEncoder enc(2);
    Buffer in(2), out;
    int n = 0;
    for (uint32_t prev = 0; prev < 64; ++prev)
        for (uint32_t byte = 0; byte < 256; ++byte, ++n) {
            uint8_t *p = static_cast<uint8_t *>(in.getData());
            p[0] = (uint8_t)(0x80u | prev);             // (bits older than six steps do not count)
            p[1] = (uint8_t)byte;
            enc.process(&in, &out);
            const uint8_t *o = static_cast<const uint8_t *>(out.getData());
            CHECK(out.getLength() == 11);
            CHECK(be32(o) == mother_code(0, p[0]));
            CHECK(be32(o + 4) == mother_code(prev, byte));
            CHECK(be32(o + 4) == mother_code(p[0], byte));
            CHECK((((uint32_t)o[8] << 24) | ((uint32_t)o[9] << 16) | ((uint32_t)o[10] << 8)) == (mother_code(byte, 0) & 0xffffff00u));
        }
    // the decoder's expected nibble is the code of the window with the oldest bit 0; the other branch's is its complement
    for (uint32_t s = 0; s < 64; ++s) {
        CHECK(branch_nibble(s) == code_nibble(s));
        CHECK(code_nibble(0x40u | s) == (branch_nibble(s) ^ 0xfu));
        CHECK(branch_nibble(s) == (mother_code(s >> 1, (s & 1u) << 7) >> 28));
    }
    return n;
}

// spread_bits(keep_bits(w, p), p, popc p) == w & p for every puncturing vector and the tail pattern
int check_keep_spread()
{
    std::vector<uint32_t> patterns(kPuncturingVector, kPuncturingVector + 25);
    patterns.push_back(kTail);
    uint32_t w = 0x12345678u;
    int n = 0;
    for (uint32_t p : patterns)
        for (int k = 0; k < 1000; ++k, ++n) {
            w = w * 1664525u + 1013904223u;
            const uint32_t kept = (uint32_t)__builtin_popcount(p), acc = keep_bits(w, p);
            CHECK(kept == 32 || (acc >> kept) == 0);
            CHECK(spread_bits(acc, p, kept) == (w & p));
        }
    CHECK(keep_bits(0xffffffffu, kTail) == 0xfffu && spread_bits(0xfffu, kTail, 12) == kTail);
    return n;
}

// the sixteen delay masks against TimeInterleaver: one frame of ones, then zeros -- call d gives back the bits delayed by d
void check_delay_mask()
{
    TimeInterleaver ti(4);
    Buffer in(4), out;
    uint32_t all = 0;
    int bits = 0;
    for (int d = 0; d < 16; ++d) {
        std::memset(in.getData(), d == 0 ? 0xff : 0, 4);
        ti.process(&in, &out);
        uint32_t v;
        std::memcpy(&v, out.getData(), 4);              // (a little-endian dword, as the kernels read it)
        CHECK(v == delay_mask(d));
        all |= delay_mask(d);
        bits += __builtin_popcount(delay_mask(d));
    }
    CHECK(all == 0xffffffffu && bits == 32);
}

// fe_segment against a linear walk over the groups, and the unit punctured through it against PuncturingEncoder
int check_segments(const std::vector<PuncturingRule> &rules, uint32_t in_bytes, uint32_t want_rules)
{
    CHECK(rules.size() == want_rules);
    const FeUnit u = unit_of(rules, in_bytes);
    CHECK(u.g0[u.nseg] == in_bytes);
    uint32_t r = 0, left = (uint32_t)((rules[0].length() + 3) / 4), bit = 0;
    for (uint32_t i = 0; i <= in_bytes; ++i) {
        const uint32_t pattern = i < in_bytes ? rules[r].pattern() : kTail;
        const FeSegment g = fe_segment(u, i);
        CHECK(g.pattern == pattern && g.kept == (uint32_t)__builtin_popcount(pattern) && g.at == bit);
        bit += g.kept;
        if (i < in_bytes && --left == 0 && ++r < rules.size()) left = (uint32_t)((rules[r].length() + 3) / 4);
    }
    CHECK(bit == u.base[u.nseg] + 12);

    // a payload through ConvEncoder and PuncturingEncoder, and through mother_code, fe_segment and keep_bits as fe_encode_kernel does
    std::vector<uint8_t> payload(in_bytes);
    uint32_t w = 0x9e3779b9u;
    for (uint8_t &b : payload) b = (uint8_t)((w = w * 1664525u + 1013904223u) >> 24);
    Buffer in(payload), coded, punctured;
    ConvEncoder enc(in_bytes);
    PuncturingEncoder pun;
    for (const PuncturingRule &rule : rules) pun.append_rule(rule);
    pun.append_tail_rule(PuncturingRule(3, 0xcccccc));
    enc.process(&in, &coded);
    pun.process(&coded, &punctured);
    CHECK(punctured.getLength() == u.out_bytes);
    std::vector<uint8_t> mine(u.out_bytes + 8, 0);
    for (uint32_t i = 0; i <= in_bytes; ++i) {
        const uint32_t code = mother_code(i ? payload[i - 1] : 0u, i < in_bytes ? payload[i] : 0u);
        const FeSegment g = fe_segment(u, i);
        const uint32_t acc = keep_bits(code, g.pattern);
        for (uint32_t k = 0; k < g.kept; ++k)
            if ((acc >> (g.kept - 1 - k)) & 1u) mine[(g.at + k) >> 3] |= (uint8_t)(0x80u >> ((g.at + k) & 7u));
    }
    CHECK(std::memcmp(mine.data(), punctured.getData(), std::min<size_t>(u.out_bytes, punctured.getLength())) == 0);
    return (int)in_bytes + 1;
}

// tf_row_word forwards (every word of a transmission frame against the layout written out: the FICs of its ETI frames, then
// their CIFs) and backwards (every word of every row is reached, once)
int check_rows(uint32_t cifs, uint32_t fic_row, uint32_t cif_row)
{
    const uint32_t row_words = fic_row + cif_row;
    std::vector<int> hits(cifs * row_words, 0);
    uint32_t w = 0;
    for (uint32_t k = 0; k < cifs; ++k)
        for (uint32_t at = 0; at < fic_row; ++at, ++w) {
            const RowWord r = tf_row_word(w, cifs, fic_row, cif_row);
            CHECK(r.k == k && r.at == at);
            ++hits[r.k * row_words + r.at];
        }
    for (uint32_t k = 0; k < cifs; ++k)
        for (uint32_t at = 0; at < cif_row; ++at, ++w) {
            const RowWord r = tf_row_word(w, cifs, fic_row, cif_row);
            CHECK(r.k == k && r.at == fic_row + at);
            ++hits[r.k * row_words + r.at];
        }
    CHECK(w == cifs * row_words);
    for (int h : hits) CHECK(h == 1);
    return (int)w;
}

}  // namespace

int main()
{
    const int codes = check_mother_code();
    const int words = check_keep_spread();
    check_delay_mask();
    // EEP 3-A at 64 kbit/s (two rules) and UEP level 3 at 32 kbit/s (four rules)
    const SubchannelSource eep(0, 24, 0x22), uep(0, 12, 2);
    int groups = check_segments(eep.get_rules(), (uint32_t)eep.framesize(), 2);
    groups += check_segments(uep.get_rules(), (uint32_t)uep.framesize(), 4);
    // modes I - IV: (CIFs per transmission frame, punctured FIC bytes per ETI frame); hard rows and soft rows
    const uint32_t modes[4][2] = {{4, 288}, {1, 288}, {1, 384}, {2, 288}};
    int row_words = 0;
    for (const auto &m : modes) {
        row_words += check_rows(m[0], m[1] / 4, kFeCifBytes / 4);
        row_words += check_rows(m[0], 2 * m[1], 2 * kFeCifBytes);
    }
    if (g_failed) {
        std::fprintf(stderr, "conv_code: %d checks failed\n", g_failed);
        return 1;
    }
    std::printf("conv_code ok: %d code words, %d punctured words, 16 delays, %d groups, %d row words\n", codes, words, groups, row_words);
    return 0;
}
