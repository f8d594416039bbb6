// Quarter-sample luma fetch from a reference picture and its frame-level half-sample planes
// (me.hip me_halfpel_planes), and the vector bit cost the motion search prices with: shared by
// the search (me.hip) and the decision passes after it (h264_b.hip, h264_p_refine.hip,
// hevc_merge.hip).
#pragma once
#include "kcommon.h"

namespace mivc {
namespace gpu {

constexpr int kHpMargin = 4;  // half-sample plane margin (samples); coordinates clamp into it exactly

constexpr int kNoCost = 0x3FFFFFFF;  // the search's cost of an MB it did not search

// Exp-Golomb length of se(v) with a count-leading-zeros instead of a loop
__device__ __forceinline__ int mvbits_se(int v) {
  const uint32_t x = (v <= 0 ? static_cast<uint32_t>(-2 * v) : static_cast<uint32_t>(2 * v - 1)) + 1u;
  return 2 * (31 - __clz(x)) + 1;
}

// per-byte rounding average (a + b + 1) >> 1 of two packed words: v_lerp_u8, whose third operand
// supplies each byte's rounding bit
__device__ __forceinline__ uint32_t avg4b(uint32_t a, uint32_t b) { return __builtin_amdgcn_lerp(a, b, 0x01010101u); }

// implicit weighted bi-prediction of 4 packed samples (8.4.2.3.2 with logWD 5, offsets 0):
// (a * (64 - w1) + b * w1 + 32) >> 6; w1 = 32 is the plain rounded average
__device__ __forceinline__ uint32_t wavg4b(uint32_t a, uint32_t b, int w1) {
  if (w1 == 32) return avg4b(a, b);
  const int w0 = 64 - w1;
  uint32_t o = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int v = (static_cast<int>((a >> (8 * k)) & 255u) * w0 + static_cast<int>((b >> (8 * k)) & 255u) * w1 + 32) >> 6;
    o |= static_cast<uint32_t>(clampi(v, 0, 255)) << (8 * k);
  }
  return o;
}

// Quarter-sample luma position (xf, yf) = two (plane, du, dv) taps averaged (the G/b/h/j
// form of clause 8.4.2.2.1 used by me.hip): plane 0 = integer samples, 1 = b (half x),
// 2 = h (half y), 3 = j (centre).  `inline`: one definition for every unit that includes this,
// and every code object still keeps its own copy (no relocatable device code).  Not `static`:
// with internal linkage the optimiser folds the table's contents into plane4's control flow,
// which costs instructions and time (p_part8x8 +10 %, profiles/bframe_split.md).
inline __constant__ int8_t kQTap[16][2][3] = {
    {{0, 0, 0}, {0, 0, 0}}, {{0, 0, 0}, {1, 0, 0}}, {{1, 0, 0}, {1, 0, 0}}, {{0, 1, 0}, {1, 0, 0}},
    {{0, 0, 0}, {2, 0, 0}}, {{1, 0, 0}, {2, 0, 0}}, {{3, 0, 0}, {1, 0, 0}}, {{1, 0, 0}, {2, 1, 0}},
    {{2, 0, 0}, {2, 0, 0}}, {{3, 0, 0}, {2, 0, 0}}, {{3, 0, 0}, {3, 0, 0}}, {{3, 0, 0}, {2, 1, 0}},
    {{0, 0, 1}, {2, 0, 0}}, {{1, 0, 1}, {2, 0, 0}}, {{3, 0, 0}, {1, 0, 1}}, {{1, 0, 1}, {2, 1, 0}},
};

// 4 consecutive samples (u .. u+3, v) of one plane; coordinates clamp to the plane's
// extension (integer plane: the picture; half-sample planes: their 4-sample margin)
__device__ __forceinline__ uint32_t plane4(const uint8_t* G, const uint8_t* hp, int W, int H, int pl, int u, int v) {
  const uint8_t* row;
  int lo, hi, base;
  if (pl == 0) {
    row = G + static_cast<size_t>(clampi(v, 0, H - 1)) * W;
    lo = 0;
    hi = W - 1;
    base = 0;
  } else {
    const int PW = W + 2 * kHpMargin, PH = H + 2 * kHpMargin;
    row = hp + static_cast<size_t>(pl - 1) * PW * PH +
          static_cast<size_t>(clampi(v, -kHpMargin, H + kHpMargin - 1) + kHpMargin) * PW;
    lo = -kHpMargin;
    hi = W + kHpMargin - 1;
    base = kHpMargin;
  }
  const int x = u + base, a = x & ~3;
  if (u >= lo && u + 3 <= hi && a + 8 <= hi + base + 1) {
    const uint32_t w0 = *reinterpret_cast<const uint32_t*>(row + a);
    const uint32_t w1 = *reinterpret_cast<const uint32_t*>(row + a + 4);
    return __builtin_amdgcn_alignbyte(w1, w0, x & 3);
  }
  uint32_t w = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) w |= static_cast<uint32_t>(row[clampi(u + k, lo, hi) + base]) << (8 * k);
  return w;
}

// predicted samples (x .. x+3, y) of a 16x16 block displaced by the quarter-sample vector
__device__ __forceinline__ uint32_t mc4(const uint8_t* G, const uint8_t* hp, int W, int H, int x, int y, int mvx,
                                        int mvy) {
  const int q = (mvy & 3) * 4 + (mvx & 3);
  const int xi = x + (mvx >> 2), yi = y + (mvy >> 2);
  const uint32_t A = plane4(G, hp, W, H, kQTap[q][0][0], xi + kQTap[q][0][1], yi + kQTap[q][0][2]);
  const uint32_t Bv = plane4(G, hp, W, H, kQTap[q][1][0], xi + kQTap[q][1][1], yi + kQTap[q][1][2]);
  return avg4b(A, Bv);
}

// 8 bytes at a 4-byte aligned address as one access (global_load_dwordx2)
struct __attribute__((packed, aligned(4))) QpelPair {
  uint32_t lo, hi;
};

// plane4 of the four rows v .. v+3, the work that does not depend on the row done once: one
// inside test for the block (the rows need no clamp, and the aligned 8 bytes lie in the plane:
// plane4's condition for every row -- its u + 3 <= hi follows from the 8 bytes fitting), then
// four 8-byte loads a pitch apart.  Any other block goes through plane4 row by row.
__device__ __forceinline__ void plane4x4(const uint8_t* G, const uint8_t* hp, int W, int H, int pl, int u, int v,
                                         uint32_t (&out)[4]) {
  const int PW = W + 2 * kHpMargin, PH = H + 2 * kHpMargin;
  const int m = pl == 0 ? 0 : kHpMargin, pitch = pl == 0 ? W : PW;
  const int x = u + m, a = x & ~3;
  if (u >= -m && a + 8 <= pitch && v >= -m && v + 3 <= H + m - 1) {
    const uint8_t* p = (pl == 0 ? G : hp + static_cast<size_t>(pl - 1) * PW * PH) +
                       static_cast<size_t>(v + m) * pitch + a;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const QpelPair w = *reinterpret_cast<const QpelPair*>(p + static_cast<size_t>(k) * pitch);
      out[k] = __builtin_amdgcn_alignbyte(w.hi, w.lo, x & 3);
    }
    return;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) out[k] = plane4(G, hp, W, H, pl, u, v + k);
}

// the 4x4 block at (x, y) displaced by the quarter-sample vector, as four packed rows: equal
// to mc4 of rows y .. y+3 bit for bit.  The phase, the taps and the addresses are worked out
// once for the block; a phase whose two taps are the same sample (integer and pure half
// positions) fetches it once, avg4b(A, A) being A.
__device__ __forceinline__ void mc4x4(const uint8_t* G, const uint8_t* hp, int W, int H, int x, int y, int mvx,
                                      int mvy, uint32_t (&out)[4]) {
  const int q = (mvy & 3) * 4 + (mvx & 3);
  const int xi = x + (mvx >> 2), yi = y + (mvy >> 2);
  const int p0 = kQTap[q][0][0], u0 = kQTap[q][0][1], v0 = kQTap[q][0][2];
  const int p1 = kQTap[q][1][0], u1 = kQTap[q][1][1], v1 = kQTap[q][1][2];
  plane4x4(G, hp, W, H, p0, xi + u0, yi + v0, out);
  if (p0 == p1 && u0 == u1 && v0 == v1) return;
  uint32_t b[4];
  plane4x4(G, hp, W, H, p1, xi + u1, yi + v1, b);
#pragma unroll
  for (int k = 0; k < 4; ++k) out[k] = avg4b(out[k], b[k]);
}

}  // namespace gpu
}  // namespace mivc
