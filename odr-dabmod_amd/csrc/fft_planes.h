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
//   stage 4   lane t  = k0 + 8 k1 + 64 j        reads rows j and j + 4, columns 4 q(k0, k1) + (c = 0 .. 3)
// and lane t leaves the last stage with x[t + 256 m], m = 0 .. 7, in natural order -- as the padded 8-byte exchanges do.
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
constexpr int q(int k0, int k1)
{
    return ((k0 >> 1) & 1) | ((k1 & 1) << 1) | ((k0 & 1) << 2) | (((k1 ^ (k1 >> 1)) & 1) << 3) | (((k0 >> 2) & 1) << 4) |
           (((k1 >> 2) & 1) << 5);
}
constexpr int q_k0(int v) { return ((v >> 2) & 1) | ((v & 1) << 1) | (((v >> 4) & 1) << 2); }
constexpr int q_k1(int v) { return ((v >> 1) & 1) | ((((v >> 3) ^ (v >> 1)) & 1) << 1) | (((v >> 5) & 1) << 2); }

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
// gather 3: four dwords from here = inputs c = 0 .. 3 of butterfly 0 (row j); butterfly 1 reads four rows further down
constexpr int read3(int t) { return write_at(t >> 6, lane2(t & 7, (t >> 3) & 7, 0)); }
constexpr int kRead3Second = 4 * kPitch;

// ---- twiddle indices ------------------------------------------------------------------------------------------------------------
// stage 2 multiplies input a by W_64^(a k0), stage 3 input b by W_512^(b (k0 + 8 k1)), the last stage input c of butterfly
// beta by W_2048^(c (t + 256 beta))
constexpr int tw2_index(int l1) { return lane1_k0(l1); }
constexpr int tw3_index(int l2) { return lane2_k0(l2) + 8 * lane2_k1(l2); }

}  // namespace fftp
}  // namespace dabgpu
