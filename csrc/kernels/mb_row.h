// Four macroblocks (16x16 blocks) per wave, one 16-lane row each: a lane owns one 4x4 block
// (raster order) of its MB, prices it from registers, and the row sums with DPP.  The passes
// laid out this way (p_mv_refine, b_decide, hevc_merge_refine, hevc_b_choose, hevc_b_merge,
// encode_inter_mb) are chains of dependent loads per MB (vectors -> prediction -> cost), so
// MBs in flight set their speed: one MB per wave was about half as fast.
#pragma once
#include "kcommon.h"

namespace mivc {
namespace gpu {

constexpr int kMbsPerWave = 4;

// grid.x of a (units, slots) launch with 64 threads per workgroup
inline int mb_row_grid(int nmb) { return (nmb + kMbsPerWave - 1) / kMbsPerWave; }

// 4:2:0 chroma of an MB is eight 4x4 blocks, a lane each: eight MBs per wave (encode_inter_chroma)
constexpr int kMbsPerChromaWave = 8;
inline int chroma_wave_grid(int nmb) { return (nmb + kMbsPerChromaWave - 1) / kMbsPerChromaWave; }

struct MbRow {
  int slot, mb;  // mb: raster index in the slot's picture
  int lane;      // 0..15: this lane's 4x4 block of the MB, raster order
  int row;       // 0..3: this MB's row of the wave
  size_t o;      // slot * nmb + mb
  int mx, my;    // MB position
  int bx4, by4;  // the lane's block inside the MB (samples)
  int X, Y;      // and in the picture
  // false: past the last MB, or the slot takes no part in a routed launch.  Dead rows return at
  // once, so only whole 16-lane rows stay and the DPP row sums stay row-local.
  bool live;
};

// rt / kind: routed launches (route_active); unrouted kernels pass no route
__device__ __forceinline__ MbRow mb_row(const Geom& g, const SlotRoute* rt = nullptr, int kind = -1) {
  MbRow r;
  int unit;
  xcd_unit_slot(unit, r.slot);
  r.lane = threadIdx.x & 15;
  r.row = threadIdx.x >> 4;
  r.mb = unit * kMbsPerWave + r.row;
  r.live = route_active(rt, r.slot, kind) && r.mb < g.nmb();
  r.o = static_cast<size_t>(r.slot) * g.nmb() + r.mb;
  r.mx = r.mb % g.wmb;
  r.my = r.mb / g.wmb;
  r.bx4 = (r.lane & 3) * 4;
  r.by4 = (r.lane >> 2) * 4;
  r.X = r.mx * 16 + r.bx4;
  r.Y = r.my * 16 + r.by4;
  return r;
}

// the lane's 4x4 source block as four packed rows
__device__ __forceinline__ void load_src4(const Geom& g, const MbRow& r, const uint8_t* src_y, uint32_t (&s)[4]) {
  const size_t yo = static_cast<size_t>(r.slot) * g.ysize();
#pragma unroll
  for (int y = 0; y < 4; ++y)
    s[y] = *reinterpret_cast<const uint32_t*>(src_y + yo + static_cast<size_t>(r.Y + y) * g.W + r.X);
}

// lambda of MB o = slot * nmb + mb at the slot's QP plus the MB's adaptive offset (nullable)
__device__ __forceinline__ int mb_lambda(const int* qp, const int8_t* aq, int slot, size_t o) {
  return h264::kLambda[clampi(qp[slot] + (aq ? aq[o] : 0), 0, 51)];
}

// SATD of the MB against a prediction, each lane giving its block's four packed rows: the row's
// total on every lane of the row
__device__ __forceinline__ int row_satd(const uint32_t (&src)[4], const uint32_t (&pw)[4]) {
  return sum16(satd4x4_u8(src, pw));
}

// Jacobi passes after the first: did the previous pass move this MB or a neighbour its
// candidates come from (left, above, above-right, above-left, and below-left for the HEVC merge
// list)?  chg: the slot's flags.  Row-uniform.
__device__ __forceinline__ bool moved_nearby(const Geom& g, const MbRow& r, const uint8_t* chg, bool below_left) {
  const int mb = r.mb, mx = r.mx, my = r.my;
  bool any = chg[mb];
  if (mx > 0) any = any || chg[mb - 1] || (below_left && my + 1 < g.hmb && chg[mb + g.wmb - 1]);
  if (my > 0)
    any = any || chg[mb - g.wmb] || (mx + 1 < g.wmb && chg[mb - g.wmb + 1]) || (mx > 0 && chg[mb - g.wmb - 1]);
  return any;
}

}  // namespace gpu
}  // namespace mivc
