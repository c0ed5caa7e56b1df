// superframe.h -- the DAB+ superframe reader (superframe.hip, api_superframe.hip): what one candidate -- five consecutive
// sub-channel frames -- says, as one fixed-size record; GF(2^8) of the outer code as compile-time tables; Fire code, header and
// AU CRC (sf_read_header, sf_au_ok) in plain C++ for host and device.
// ETSI TS 102 563 5.2 (superframe, header), 5.3 (Fire code), 5.4 (AU CRC), 6 (RS(120,110), interleaving over the five frames).
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SF_HD __host__ __device__ inline
#else
#define SF_HD inline
#endif

namespace dabgpu {

constexpr int kSfFrames = 5;               // sub-channel frames per superframe
constexpr int kSfN = 120, kSfK = 110;      // bytes per codeword, data bytes of them
constexpr int kSfParity = 10;
constexpr int kSfMaxS = 24;                // codewords per superframe at most (192 kbit/s)
constexpr uint32_t kSfFailed = 0xffu;      // cw_errors of an uncorrectable word
enum : uint32_t { SF_FIRE_OK = 1, SF_ZERO = 2, SF_HEADER_VALID = 4, SF_RS_FAILED = 8 };

// the layout of dabgpu_sf_record (include/dabgpu.h documents the fields)
struct SfRecord {
    uint32_t flags;
    uint16_t rs_corrected, rs_failed;
    uint8_t rs_max, num_aus, au_ok, header;
    uint8_t rfa, dac_rate, sbr_flag, aac_channel_mode, ps_flag, mpeg_surround_config, reserved0[2];
    uint16_t au_start[7];
    uint16_t fire_crc;
    uint8_t cw_errors[kSfMaxS];
    uint32_t reserved1;
};
static_assert(sizeof(SfRecord) == 64 && offsetof(SfRecord, au_start) == 20 && offsetof(SfRecord, cw_errors) == 36,
              "fixed layout of a candidate's record");

SF_HD bool sf_accepted(uint32_t flags) { return (flags & (SF_FIRE_OK | SF_ZERO | SF_HEADER_VALID)) == (SF_FIRE_OK | SF_HEADER_VALID); }

// GF(2^8), x^8 + x^4 + x^3 + x^2 + 1: exp[i] = alpha^i for i < 510 (twice over, so a sum of two logarithms needs no reduction)
struct SfField {
    uint8_t exp[512], log[256];
    constexpr SfField() : exp{}, log{}
    {
        uint32_t x = 1;
        for (int i = 0; i < 255; ++i) {
            exp[i] = (uint8_t)x;
            log[x] = (uint8_t)i;
            x <<= 1;
            if (x & 0x100u) x ^= 0x11du;
        }
        for (int i = 255; i < 512; ++i) exp[i] = exp[i - 255];
    }
};

// CRC-16, one byte per step, most significant bit first
SF_HD uint32_t sf_crc_step(uint32_t crc, uint32_t byte, uint32_t poly)
{
    crc ^= byte << 8;
    for (int k = 0; k < 8; ++k) crc = (crc & 0x8000u) ? ((crc << 1) ^ poly) & 0xffffu : (crc << 1) & 0xffffu;
    return crc;
}

// Fire code, header and validity of a superframe's corrected bytes b[0 ... 110 s - 1] into the record (flags: FIRE_OK, ZERO,
// HEADER_VALID or-ed in; header fields, num_aus, au_start, fire_crc written).  Reads bytes 0 ... 11 only.
SF_HD void sf_read_header(const uint8_t *b, uint32_t s, SfRecord *r)
{
    uint32_t crc = 0, any = (uint32_t)b[0] | b[1];
    for (int i = 2; i < 11; ++i) {
        crc = sf_crc_step(crc, b[i], 0x782fu);
        any |= b[i];
    }
    r->fire_crc = (uint16_t)crc;
    if (crc == ((uint32_t)b[0] << 8 | b[1])) r->flags |= SF_FIRE_OK;
    if (!any) r->flags |= SF_ZERO;
    const uint32_t h = b[2];
    r->header = (uint8_t)h;
    r->rfa = (uint8_t)(h >> 7);
    r->dac_rate = (h >> 6) & 1u;
    r->sbr_flag = (h >> 5) & 1u;
    r->aac_channel_mode = (h >> 4) & 1u;
    r->ps_flag = (h >> 3) & 1u;
    r->mpeg_surround_config = h & 7u;
    const uint32_t num = r->sbr_flag ? (r->dac_rate ? 3u : 2u) : (r->dac_rate ? 6u : 4u);
    const uint32_t first = r->sbr_flag ? (r->dac_rate ? 6u : 5u) : (r->dac_rate ? 11u : 8u);
    r->num_aus = (uint8_t)num;
    uint32_t prev = first;
    bool valid = true;
    r->au_start[0] = (uint16_t)first;
    for (uint32_t k = 1; k <= 6; ++k) {
        uint32_t v = 0;
        if (k < num) {
            const uint32_t bit = 24 + 12 * (k - 1), at = bit >> 3, w = (uint32_t)b[at] << 8 | b[at + 1];
            v = (bit & 7u) ? (w & 0xfffu) : (w >> 4);
        } else if (k == num) {
            v = (uint32_t)kSfK * s;
        }
        r->au_start[k] = (uint16_t)v;
        if (k <= num) {
            if (v < prev + 3) valid = false;
            prev = v;
        }
    }
    if (valid) r->flags |= SF_HEADER_VALID;
}

// the AU b[from ... to - 1]: the FIB's CRC (0x1021, register all ones, complemented) over all but its last two bytes against them
SF_HD bool sf_au_ok(const uint8_t *b, uint32_t from, uint32_t to)
{
    uint32_t crc = 0xffffu;
    for (uint32_t i = from; i + 2 < to; ++i) {
        uint32_t x = ((crc >> 8) ^ b[i]) & 0xffu;
        x ^= x >> 4;
        crc = ((crc << 8) ^ (x << 12) ^ (x << 5) ^ x) & 0xffffu;
    }
    return (crc ^ 0xffffu) == ((uint32_t)b[to - 2] << 8 | b[to - 1]);
}

// superframe.hip
struct SfArgs {
    const uint8_t *images;    // n_images x 6144 bytes, four-byte aligned
    uint32_t n_images, offset, s;   // the sub-channel: byte offset in an image (a multiple of 4), framesize = 24 s
    SfRecord *rec;            // n_images - 4 records
    uint8_t *out;             // (n_images - 4) x 110 s bytes
};
constexpr int kSfBlock = 256;              // one workgroup per candidate: four waves, one codeword per wave at a time
#if defined(__HIPCC__)
hipError_t launch_superframe(const SfArgs &a, hipStream_t s);
#endif

}  // namespace dabgpu
