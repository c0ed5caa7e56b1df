// fft_planes_check.cpp -- proves the index maps of the split-plane FFT exchanges (odr-dabmod_amd/csrc/fft_planes.h) on the host.
//
//   c++ -std=c++17 -O1 -I odr-dabmod_amd/csrc tools/fft_planes_check.cpp -o fft_planes_check && ./fft_planes_check
//   (add -fsanitize=address,undefined for the checked build; tests/test_fft_planes_maps.py builds and runs both)
//
// For N = 2048 it asserts that
//   1. every map is a bijection and its inverse functions invert it;
//   2. every exchange write is lane-contiguous inside a wave (what ds_write_addtid_b32 needs), inside its row, inside the plane;
//   3. every gather is 16-byte aligned, inside its row, and bank-conflict-free under the lane groups and the bank rule of
//      ds_read_b128 (four groups of sixteen lanes, bank = dword address mod 64); the partner read of the gain statistic
//      likewise under the rule of ds_read_b32 (two groups of 32 lanes, bank = dword address mod 32);
//   4. a float64 transform that moves its data ONLY through those maps equals a direct DFT, its outputs placed where the last
//      stage's lanes leave them: x[2 t + b + 512 k3] in register b + 2 k3 of lane t;
//   5. the 16-byte output stores of the frame kernel (body, cyclic prefix) and the 44 boundary outputs together write every one of
//      a symbol segment's 2552 positions exactly once, every 16-byte store at an even sample offset from the frame's base, and the
//      16-byte accesses to the equalised boundary's parked windows are aligned pairs; with the difference window, which is kept one
//      entry lower, they cover exactly the samples the boundary reads.
// Exit status 0 and one summary line when all of it holds; the first failure is reported and ends the run with status 1.
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <vector>

#include "fft_planes.h"

using namespace dabgpu::fftp;
typedef std::complex<double> cd;

static int failures = 0;
#define CHECK(cond, ...)                                                  \
    do {                                                                  \
        if (!(cond)) {                                                    \
            std::fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__);     \
            std::fprintf(stderr, __VA_ARGS__);                            \
            std::fprintf(stderr, "\n");                                   \
            if (++failures > 20) std::exit(1);                            \
        }                                                                 \
    } while (0)

// the lane groups one LDS cycle serves of a wave's ds_read_b128
static const int kGroups128[4][16] = {
    {0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27},
    {4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31},
    {32, 33, 34, 35, 44, 45, 46, 47, 52, 53, 54, 55, 56, 57, 58, 59},
    {36, 37, 38, 39, 40, 41, 42, 43, 48, 49, 50, 51, 60, 61, 62, 63},
};

// extra LDS cycles of one 16-byte read per lane at dword address addr[lane] (256 lanes, four waves)
static int conflicts128(const std::vector<int> &addr)
{
    int extra = 0;
    for (int w = 0; w < kT / 64; ++w)
        for (int g = 0; g < 4; ++g) {
            std::set<int> seen[64];
            for (int i = 0; i < 16; ++i) {
                const int a = addr[64 * w + kGroups128[g][i]];
                for (int d = 0; d < 4; ++d) seen[(a + d) % 64].insert(a + d);
            }
            int worst = 1;
            for (int b = 0; b < 64; ++b) worst = std::max(worst, (int)seen[b].size());
            extra += worst - 1;
        }
    return extra;
}
static int conflicts32(const std::vector<int> &addr)
{
    int extra = 0;
    for (int g = 0; g < kT / 32; ++g) {
        std::set<int> seen[32];
        for (int i = 0; i < 32; ++i) seen[addr[32 * g + i] % 32].insert(addr[32 * g + i]);
        int worst = 1;
        for (int b = 0; b < 32; ++b) worst = std::max(worst, (int)seen[b].size());
        extra += worst - 1;
    }
    return extra;
}

static void check_gather(const char *name, const std::vector<int> &addr, int width)
{
    for (int l = 0; l < kT; ++l) {
        CHECK(addr[l] % 4 == 0, "%s: lane %d reads at dword %d, not 16-byte aligned", name, l, addr[l]);
        CHECK(addr[l] >= 0 && addr[l] % kPitch + width <= kT && addr[l] + width <= kPlane, "%s: lane %d leaves its row", name, l);
    }
    for (int h = 0; h < width; h += 4) {
        std::vector<int> a(addr);
        for (int &x : a) x += h;
        const int extra = conflicts128(a);
        CHECK(extra == 0, "%s + %d: %d extra LDS cycles from bank conflicts", name, h, extra);
    }
}

static void dft(const cd *in, cd *out, int n)          // backward: exp(+2 pi i jk/n)
{
    for (int k = 0; k < n; ++k) {
        cd s = 0;
        for (int j = 0; j < n; ++j) s += in[j] * std::polar(1.0, 2.0 * M_PI * (double)((j * k) % n) / n);
        out[k] = s;
    }
}

int main()
{
    double rel_out = 0.;
    static_assert(kN == 8 * kT && kPitch >= kT && kPitch % 4 == 0 && kBytes == 2 * 8 * kPitch * 4 && kElems * 8 == kBytes, "geometry");

    // ---- 1. bijections ----------------------------------------------------------------------------------------------------
    {
        std::set<int> s;
        for (int l = 0; l < kT; ++l) {
            const int t = in_index(l);
            CHECK(t >= 0 && t < kT && in_lane(t) == l, "in_index / in_lane at lane %d", l);
            s.insert(t);
            const int p = in_partner(l);
            CHECK(p >= 0 && p < kT && ((in_index(p) + t) & (kT - 1)) == 0, "in_partner at lane %d", l);
        }
        CHECK((int)s.size() == kT, "in_index is no bijection");
    }
    {
        std::set<int> s;
        for (int k0 = 0; k0 < 8; ++k0)
            for (int c = 0; c < 4; ++c) {
                const int u = u1(k0, c);
                CHECK(u >= 0 && u < 32 && u1_k0(u) == k0 && u1_c(u) == c, "u1 at (%d, %d)", k0, c);
                s.insert(u);
            }
        CHECK(s.size() == 32, "u1 is no bijection");
    }
    {
        std::set<int> s;
        for (int k0 = 0; k0 < 8; ++k0)
            for (int k1 = 0; k1 < 8; ++k1) {
                const int v = q(k0, k1);
                CHECK(v >= 0 && v < 64 && q_k0(v) == k0 && q_k1(v) == k1, "q at (%d, %d)", k0, k1);
                s.insert(v);
            }
        CHECK(s.size() == 64, "q is no bijection");
    }
    {
        std::set<int> s1, s2;
        for (int l = 0; l < kT; ++l) {
            CHECK(lane1(lane1_k0(l), lane1_b(l), lane1_c(l)) == l, "lane1 at %d", l);
            CHECK(lane2(lane2_k0(l), lane2_k1(l), lane2_c(l)) == l, "lane2 at %d", l);
            s1.insert(64 * lane1_k0(l) + 8 * lane1_b(l) + lane1_c(l));
            s2.insert(64 * lane2_k0(l) + 8 * lane2_k1(l) + lane2_c(l));
        }
        CHECK(s1.size() == (size_t)kT && s2.size() == (size_t)kT, "lane1 / lane2 are no bijections");
    }
    {
        // last stage: butterfly b of lane t is the butterfly (k0, k1, k2) of outputs k0 + 8 k1 + 64 k2 + 512 k3 = 2 t + b + 512 k3
        std::set<int> s, o;
        for (int t = 0; t < kT; ++t)
            for (int b = 0; b < 2; ++b) {
                const int k0 = last_k0(t, b), k1 = last_k1(t), k2 = last_k2(t);
                CHECK(k0 >= 0 && k0 < 8 && k1 >= 0 && k1 < 8 && k2 >= 0 && k2 < 8, "last stage: indices of lane %d", t);
                CHECK(k0 + 8 * k1 + 64 * k2 == 2 * t + b && tw4_index(t, b) == 2 * t + b, "last stage: lane %d, butterfly %d", t, b);
                s.insert(k0 + 8 * k1 + 64 * k2);
                for (int k3 = 0; k3 < 4; ++k3) {
                    CHECK(out_sample(t, b, k3) == k0 + 8 * k1 + 64 * k2 + 512 * k3, "out_sample at lane %d", t);
                    o.insert(out_sample(t, b, k3));
                }
            }
        CHECK(s.size() == 512 && o.size() == (size_t)kN && *o.begin() == 0 && *o.rbegin() == kN - 1, "the last stage's lanes are no bijection");
    }

    // ---- 2. writes: 64 consecutive dwords per wave and slot, rows apart, inside the plane ----------------------------------
    for (int slot = 0; slot < 8; ++slot)
        for (int w = 0; w < kT / 64; ++w)
            for (int i = 0; i < 64; ++i) {
                const int at = write_at(slot, 64 * w + i);
                CHECK(at == write_at(slot, 64 * w) + i, "write of slot %d, wave %d is not lane-contiguous", slot, w);
                CHECK(at >= slot * kPitch && at < slot * kPitch + kT && at < kPlane, "write of slot %d leaves its row", slot);
            }

    // ---- 3. gathers ---------------------------------------------------------------------------------------------------------
    {
        std::vector<int> a1(kT), a2(kT), a3(kT), a3b(kT), ap(kT);
        for (int l = 0; l < kT; ++l) {
            a1[l] = read1(l);
            a2[l] = read2(l);
            a3[l] = read3(l, 0);
            a3b[l] = read3(l, 1);
            const int row = write_at(last_k2(l), 0);
            CHECK(a3b[l] == row + ((a3[l] - row) ^ kRead3Flip), "gather 3: butterfly 1 of lane %d is not butterfly 0's column ^ %d", l, kRead3Flip);
            ap[l] = in_partner(l);
        }
        check_gather("gather 1", a1, 8);
        check_gather("gather 2", a2, 8);
        check_gather("gather 3, butterfly 0", a3, 4);
        check_gather("gather 3, butterfly 1", a3b, 4);
        const int extra = conflicts32(ap);
        CHECK(extra == 0, "partner read of the gain statistic: %d extra LDS cycles", extra);
    }

    // ---- 4. the transform, data moved through the maps alone ------------------------------------------------------------------
    {
        std::vector<cd> x(kN), want(kN), got(kN, cd(1e300, 1e300));
        unsigned long long st = 0x9E3779B97F4A7C15ull;
        auto rnd = [&]() {
            st = st * 6364136223846793005ull + 1442695040888963407ull;
            return (double)(st >> 11) / (double)(1ull << 53) - 0.5;
        };
        for (cd &v : x) v = cd(rnd(), rnd());
        dft(x.data(), want.data(), kN);

        const cd nan(std::nan(""), std::nan(""));
        std::vector<cd> plane(kPlane, nan), next(kPlane, nan);
        cd v[8], y[8];
        for (int l = 0; l < kT; ++l) {                         // stage 1
            for (int r = 0; r < 8; ++r) v[r] = x[in_index(l) + kT * r];
            dft(v, y, 8);
            for (int k0 = 0; k0 < 8; ++k0) plane[write_at(k0, l)] = y[k0];
        }
        for (int l1 = 0; l1 < kT; ++l1) {                      // stage 2
            for (int a = 0; a < 8; ++a) v[a] = plane[read1(l1) + a] * std::polar(1.0, 2.0 * M_PI * (a * tw2_index(l1)) / 64.0);
            dft(v, y, 8);
            for (int k1 = 0; k1 < 8; ++k1) next[write_at(k1, l1)] = y[k1];
        }
        plane.assign(kPlane, nan);
        for (int l2 = 0; l2 < kT; ++l2) {                      // stage 3
            for (int b = 0; b < 8; ++b) v[b] = next[read2(l2) + b] * std::polar(1.0, 2.0 * M_PI * (b * tw3_index(l2)) / 512.0);
            dft(v, y, 8);
            for (int k2 = 0; k2 < 8; ++k2) plane[write_at(k2, l2)] = y[k2];
        }
        for (int t = 0; t < kT; ++t)                           // last stage: two radix-4 butterflies
            for (int beta = 0; beta < 2; ++beta) {
                for (int c = 0; c < 4; ++c)
                    v[c] = plane[read3(t, beta) + c] * std::polar(1.0, 2.0 * M_PI * ((c * tw4_index(t, beta)) % kN) / (double)kN);
                dft(v, y, 4);
                for (int k3 = 0; k3 < 4; ++k3) got[out_sample(t, beta, k3)] = y[k3];
            }
        double err = 0., ref = 0.;
        for (int k = 0; k < kN; ++k) {
            err += std::norm(got[k] - want[k]);
            ref += std::norm(want[k]);
        }
        const double rel = std::sqrt(err / ref);
        // (float64: the four stages and the direct sum both round at a few 1e-16 per operation)
        CHECK(rel < 1e-13, "transform through the maps differs from the DFT: rel. error %.3g", rel);
        rel_out = rel;
    }

    // ---- 5. the output stores of a symbol and the windows of the equalised boundary ----------------------------------------------
    {
        // Mode I frame: a null segment of 2656 samples, then segments of kSeg = 2552; every length that enters a store offset is even
        static_assert(kSeg == 2552 && 2656 % 2 == 0 && kSeg % 2 == 0 && kCp % 2 == 0 && (kN - kC) % 2 == 0, "even lengths");
        std::vector<int> written(kSeg, 0);
        int stores16 = 0;
        for (int k3 = 0; k3 < kPairSlots; ++k3)
            for (int t = 0; t < kT; ++t) {
                CHECK(out_sample(t, 1, k3) == out_sample(t, 0, k3) + 1 && out_sample(t, 0, k3) % 2 == 0, "pair slot %d, lane %d holds no pair", k3, t);
                if (body_lane(k3, t)) {
                    const int at = body_at(k3, t);
                    CHECK(at % 2 == 0 && at >= kCp && at + 1 < kSeg - kC, "body store of slot %d, lane %d at %d", k3, t, at);
                    CHECK(at == kCp + out_sample(t, 0, k3), "body store of slot %d, lane %d holds other samples", k3, t);
                    if (at >= 0 && at + 1 < kSeg) { ++written[at]; ++written[at + 1]; }
                    ++stores16;
                }
                if (prefix_lane(k3, t)) {
                    const int at = prefix_at(k3, t);
                    CHECK(k3 == 3 && t >= 4 && at == 2 * (t - 4), "prefix store of slot %d, lane %d", k3, t);
                    CHECK(at % 2 == 0 && at >= 0 && at + 1 < kCp, "prefix store of slot %d, lane %d at %d", k3, t, at);
                    if (at >= 0 && at + 1 < kSeg) { ++written[at]; ++written[at + 1]; }
                    ++stores16;
                }
                // (a lane's four 16-byte body stores lie 1 KB apart per wave: lane t at byte 16 t of its pair slot)
                CHECK(body_at(k3, t) - body_at(k3, 0) == 2 * t, "body stores of slot %d are not lane-contiguous", k3);
            }
        for (int i = 0; i < kC; ++i) ++written[kSeg - kC + i];                 // the boundary outputs (8-byte stores)
        for (int n = 0; n < kSeg; ++n) CHECK(written[n] == 1, "segment position %d is written %d times", n, written[n]);
        CHECK(stores16 * 2 + kC == kSeg, "%d 16-byte stores", stores16);
        // every segment starts at an even sample of the frame, so an even offset inside it is a 16-byte multiple from the frame's base
        for (int s = 1; s <= 76; ++s) CHECK((2656 + (s - 1) * kSeg) % 2 == 0, "segment %d starts at an odd sample", s);

        // windows: w and the two parked ones, each entry written exactly once, by aligned pairs
        std::vector<int> w(kWinLen, 0), parked(kWinLen, 0), zread(kWinLen, 0);
        for (int k3 = 0; k3 < kPairSlots; ++k3)
            for (int t = 0; t < kT; ++t) {
                const int n = out_sample(t, 0, k3);
                if (win_w_lane(k3, t)) {
                    const int i = win_index_w(n);
                    CHECK(i % 2 == 0 && i >= 0 && i + 1 < kWinLen, "w pair of slot %d, lane %d at %d", k3, t, i);
                    CHECK(n == kN - kCp + (i - kWinQ0), "w index %d is sample %d", i, n);
                    // (the z_prev pair is read at i, aligned; w is kept kWinWShift lower, as two halves, the one for q = -104 dropped)
                    if (i >= 0 && i + 1 < kWinLen) { ++zread[i]; ++zread[i + 1]; }
                    for (int h = 0; h < 2; ++h)
                        if (i + h - kWinWShift >= 0 && i + h - kWinWShift < kWinLen) ++w[i + h - kWinWShift];
                    CHECK((k3 == 2 && t >= 208) || (k3 == 3 && t < 54), "w written by slot %d, lane %d", k3, t);
                }
                if (win_tail_lane(k3, t)) {
                    const int i = win_index_tail(n);
                    CHECK(i % 2 == 0 && i >= 0 && i + 1 < kWinQ0 && n == kN + (i - kWinQ0), "tail window pair of slot %d, lane %d at %d", k3, t, i);
                    if (i >= 0 && i + 1 < kWinLen) { ++parked[i]; ++parked[i + 1]; }
                    CHECK(k3 == 3 && t >= 204, "tail window written by slot %d, lane %d", k3, t);
                }
                if (win_head_lane(k3, t)) {
                    const int i = win_index_head(n);
                    CHECK(i % 2 == 0 && i >= kWinQ0 && i + 1 < kWinLen && n == i - kWinQ0, "head window pair of slot %d, lane %d at %d", k3, t, i);
                    if (i >= 0 && i + 1 < kWinLen) { ++parked[i]; ++parked[i + 1]; }
                    CHECK(k3 == 0 && t < 50, "head window written by slot %d, lane %d", k3, t);
                }
            }
        for (int i = 0; i < kWinLen; ++i) {
            CHECK(parked[i] == 1 && zread[i] == 1, "parked window entry %d: written %d times, read %d times", i, parked[i], zread[i]);
            // w: entries 0 .. kWinLen - 2 = q in [-kWinQL, kWinQH], what the inverse filter reads (index q + kWinQL)
            CHECK(w[i] == (i < kWinLen - kWinWShift ? 1 : 0), "w entry %d is written %d times", i, w[i]);
        }
        // parked: q in [-kWinQL, kWinQH] = indices 1 .. kWinLen - 1: entry 0 (q = -kWinQL - 1) is there for the alignment alone
        CHECK(kWinQ0 - kWinQL == 1 && kWinQ0 + kWinQH == kWinLen - 1 && kWinWShift == kWinQ0 - kWinQL, "window range");
    }
    if (!failures) std::printf("fft_planes_check: maps, writes, gathers ok; transform rel. error %.3g\n", rel_out);
    return failures ? 1 : 0;
}
