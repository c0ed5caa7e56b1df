// fft_planes.h -- index maps of the split-plane exchanges of the 2048-point transform (device_common.h: Fft::run_planes).
// Nothing but constexpr integer functions: the frame kernel includes it, and so does the host program that proves the maps
// (tools/fft_planes_check.cpp: bijections, lane-contiguous writes, conflict-free gathers, a float64 transform against a DFT).
//
// The transform is the 8 . 8 . 8 . 4 decimation of device_common.h (input index n = c + 4 b + 32 a + 256 r, outputs k0, k1, k2,
// k3 of the four stages), the same butterflies and twiddles in the same order.  What differs is WHICH LANE holds which element
// between the stages.  Every exchange writes one dword per lane and slot into a real and an imaginary plane of eight rows,
//     plane[slot][lane]        (row pitch kPitch dwords),
// which is what ds_write_addtid_b32 can do -- a wave writes 64 consecutive dwords, no address register --, and the lane that
// works on the next stage finds its eight inputs as eight ADJACENT source lanes of one row: two 16-byte reads per plane.
//
//   stage 1   lane l  = a + 8 b + 64 c          inputs r = 0 .. 7 of t = 32 a + 4 b + c       writes row k0, column l
//   stage 2   lane l1 = b + 8 u1(k0, c)         reads row k0, columns 8 b + 64 c + (a = 0 .. 7)  writes row k1, column l1
//   stage 3   lane l2 = c + 4 q(k0, k1)         reads row k1, columns 8 u1(k0, c) + (b = 0 .. 7) writes row k2, column l2
//   stage 4   lane t  = (k0 >> 1) + 4 k1 + 32 k2  butterfly b = k0 & 1 reads row k2, columns 4 q(k0, k1) + (c = 0 .. 3)
// and lane t leaves the last stage with x[2 t + b + 512 k3] in register b + 2 k3: PAIRS of consecutive samples, so that a symbol
// goes out in 16-byte stores, 1 KB contiguous per wave (the store arithmetic at the end of this file).  Which lane runs which
// final butterfly is nothing but a read address and a twiddle index: the butterflies and the table values are those of the
// natural-order form (lane k0 + 8 k1 + 64 j, rows j and j + 4), output for output.
// u1 and q are bit permutations (q with one exclusive-or), chosen by enumeration so that with kPitch = 260 every 16-byte read
// is bank-conflict-free under the lane groups ds_read_b128 is served in ({0-3, 12-15, 20-27}, {4-11, 16-19, 28-31}, + 32).
#pragma once

namespace dabgpu {
namespace fftp {

constexpr int kN = 2048, kT = 256;
constexpr int kPitch = 260;                 // dwords per row: 65 sixteen-byte slots, odd
constexpr int kPlane = 8 * kPitch;          // dwords per plane (re, then im)
constexpr int kBytes = 2 * kPlane * 4;      // 16640: both planes
constexpr int kElems = kBytes / 8;          // the same in complex slots

// ---- stage 1: which first-stage index the lane works on -------------------------------------------------------------------
constexpr int in_index(int l) { return 32 * (l & 7) + 4 * ((l >> 3) & 7) + (l >> 6); }
constexpr int in_lane(int t) { return (t >> 5) + 8 * ((t >> 2) & 7) + 64 * (t & 3); }
// the lane that holds carrier -k for this lane's carrier k (gain statistic of the frame kernel)
constexpr int in_partner(int l) { return in_lane((kT - in_index(l)) & (kT - 1)); }

// ---- u1: (k0, c) -> 0 .. 31 ------------------------------------------------------------------------------------------------
constexpr int u1(int k0, int c) { return (k0 & 1) | ((c >> 1) << 1) | ((c & 1) << 2) | ((k0 >> 1) << 3); }
constexpr int u1_k0(int u) { return (u & 1) | ((u >> 3) << 1); }
constexpr int u1_c(int u) { return ((u >> 2) & 1) | (((u >> 1) & 1) << 1); }

// ---- q: (k0, k1) -> 0 .. 63 ------------------------------------------------------------------------------------------------
// bits 0 .. 5: k0_1, k1_0, k1_1 ^ k0_0, k0_2, k1_1, k1_2 -- the low bit of k0 (the last stage's butterfly index) moves bit 2 alone
constexpr int q(int k0, int k1)
{
    return ((k0 >> 1) & 1) | ((k1 & 1) << 1) | ((((k1 >> 1) ^ k0) & 1) << 2) | (((k0 >> 2) & 1) << 3) | (((k1 >> 1) & 1) << 4) |
           (((k1 >> 2) & 1) << 5);
}
constexpr int q_k0(int v) { return (((v >> 2) ^ (v >> 4)) & 1) | ((v & 1) << 1) | (((v >> 3) & 1) << 2); }
constexpr int q_k1(int v) { return ((v >> 1) & 1) | (((v >> 4) & 1) << 1) | (((v >> 5) & 1) << 2); }

// ---- the lanes of stages 2 and 3 ---------------------------------------------------------------------------------------------
constexpr int lane1(int k0, int b, int c) { return b + 8 * u1(k0, c); }
constexpr int lane1_k0(int l1) { return u1_k0(l1 >> 3); }
constexpr int lane1_b(int l1) { return l1 & 7; }
constexpr int lane1_c(int l1) { return u1_c(l1 >> 3); }
constexpr int lane2(int k0, int k1, int c) { return c + 4 * q(k0, k1); }
constexpr int lane2_k0(int l2) { return q_k0(l2 >> 2); }
constexpr int lane2_k1(int l2) { return q_k1(l2 >> 2); }
constexpr int lane2_c(int l2) { return l2 & 3; }

// ---- where a lane writes and reads (dword index inside a plane) ---------------------------------------------------------------
constexpr int write_at(int slot, int lane) { return slot * kPitch + lane; }
// gather 1: eight dwords from here = inputs a = 0 .. 7 of stage 2
constexpr int read1(int l1) { return write_at(lane1_k0(l1), in_lane(4 * lane1_b(l1) + lane1_c(l1))); }
// gather 2: eight dwords from here = inputs b = 0 .. 7 of stage 3
constexpr int read2(int l2) { return write_at(lane2_k1(l2), lane1(lane2_k0(l2), 0, lane2_c(l2))); }
// gather 3: four dwords from here = inputs c = 0 .. 3 of butterfly b of lane t, i.e. of outputs 2 t + b + 512 k3.  Butterfly 1
// reads in the same row at butterfly 0's COLUMN with bit 4 flipped (k0's low bit moves bit 2 of q alone, and the column is 4 q)
constexpr int last_k0(int t, int b) { return 2 * (t & 3) + b; }
constexpr int last_k1(int t) { return (t >> 2) & 7; }
constexpr int last_k2(int t) { return t >> 5; }
constexpr int read3(int t, int b = 0) { return write_at(last_k2(t), lane2(last_k0(t, b), last_k1(t), 0)); }
constexpr int kRead3Flip = 16;

// ---- twiddle indices ------------------------------------------------------------------------------------------------------------
// stage 2 multiplies input a by W_64^(a k0), stage 3 input b by W_512^(b (k0 + 8 k1)), the last stage input c of butterfly
// b of lane t by W_2048^(c (2 t + b))
constexpr int tw2_index(int l1) { return lane1_k0(l1); }
constexpr int tw3_index(int l2) { return lane2_k0(l2) + 8 * lane2_k1(l2); }
constexpr int tw4_index(int t, int b) { return 2 * t + b; }

// ---- what leaves the last stage, and where it goes (frame kernel, Mode I: cyclic prefix kCp, the last kC outputs of a symbol --
// ---- the boundary outputs -- are not the transform's) ----------------------------------------------------------------------
// register b + 2 k3 of lane t holds sample out_sample(t, b, k3); "pair slot" k3 = registers 2 k3, 2 k3 + 1 = one 16-byte store
constexpr int kCp = 504, kC = 44, kSeg = kN + kCp, kPairSlots = 4;
constexpr int out_sample(int t, int b, int k3) { return 2 * t + b + 2 * kT * k3; }
// body: samples n < kN - kC go to segment position kCp + n (pair slot 3: lanes < 234)
constexpr bool body_lane(int k3, int t) { return out_sample(t, 1, k3) < kN - kC; }
constexpr int body_at(int k3, int t) { return kCp + out_sample(t, 0, k3); }
// cyclic prefix: samples n >= kN - kCp go to segment position n - (kN - kCp) (pair slot 3 alone: lanes >= 4, pair offset t - 4)
constexpr bool prefix_lane(int k3, int t) { return out_sample(t, 0, k3) >= kN - kCp; }
constexpr int prefix_at(int k3, int t) { return out_sample(t, 0, k3) - (kN - kCp); }
static_assert((kN - kCp) % 2 == 0 && (kN - kC) % 2 == 0 && kCp % 2 == 0 && !prefix_lane(2, kT - 1),
              "a pair never straddles the body's end or the prefix' start; the prefix lies in pair slot 3");
// The equalised boundary's windows (tf_kernel.h): index i of a window stands for q = i - kWinQ0 -- sample kN - kCp + q of the
// current symbol (the difference w is formed there against the previous symbol's parked window), sample q mod kN of the symbol
// that parks its tail and head for the next one.  Index 0 stands for an EVEN sample -- one entry in front of q = -103, where the
// 8-byte forms start --, so that every pair is one aligned 16-byte LDS access.  The difference w itself is kept kWinWShift = 1
// lower (entry 0 = q = -103, what the inverse filter's aligned reads expect), written as the two 8-byte halves of the pair.
constexpr int kWinQL = 103, kWinQH = 99;                        // q in [-kWinQL, kWinQH] is what the boundary reads
constexpr int kWinQ0 = kWinQL + 1;                              // index of q = 0: 104
constexpr int kWinLen = kWinQ0 + kWinQH + 1;                    // 204 entries, the first never read under a non-zero tap
constexpr int kWinWShift = 1;
constexpr int win_index_w(int n) { return n - (kN - kCp - kWinQ0); }          // sample n of the current symbol -> parked index; w: - kWinWShift
constexpr bool win_w_lane(int k3, int t) { return win_index_w(out_sample(t, 0, k3)) >= 0 && win_index_w(out_sample(t, 1, k3)) < kWinLen; }
constexpr bool win_tail_lane(int k3, int t) { return out_sample(t, 0, k3) >= kN - kWinQ0; }     // parked: q < 0, index n - (kN - kWinQ0)
constexpr int win_index_tail(int n) { return n - (kN - kWinQ0); }
constexpr bool win_head_lane(int k3, int t) { return out_sample(t, 1, k3) <= kWinQH; }           // parked: q >= 0, index kWinQ0 + n
constexpr int win_index_head(int n) { return kWinQ0 + n; }
static_assert((kN - kCp - kWinQ0) % 2 == 0 && (kN - kWinQ0) % 2 == 0 && kWinQ0 % 2 == 0 && kWinLen % 2 == 0, "windows start and end on pairs");

}  // namespace fftp
}  // namespace dabgpu
