// Rate-distortion check of an inter TU's levels against no levels (HevcParams.rd_cbf; the
// null-cost half of x265's --rd 3): after transform_quant_block the TU keeps its levels only when
// they pay for themselves,
//   cleared  <=>  256 * D0 + lamq * kRdCbf0 <= 256 * D1 + lamq * (Rb + kRdCbf1)      (int64, ties clear)
//   D0 = sum (src - pred)^2, D1 = sum (src - clip(pred + R'))^2 over the TU's samples,
//   Rb = the rate of the levels in 1 / 16 bit from the static bin costs of hevc_rdoq.h,
//   lamq = HM's SSD lambda in 1 / 16 units, one int32 per QpY from the host's table.
// A cleared TU has zero levels, a zero residual (reconstruction = prediction) and no cbf.
// tests/ref_models_hevc_rdcbf.py is the normative text and the numpy model the probe launch
// (hevc_rd_cbf_probe.hip) is compared with exactly.  Only the RDC instances of hevc_inter_cu
// include any of this.
#pragma once
#include "kcommon.h"
#include "hevc_rdoq.h"

namespace mivc {
namespace gpu {
namespace hv {

constexpr int kRdCbf0 = 8, kRdCbf1 = 18;  // cbf_luma / cbf_cb / cbf_cr 0 / 1 (design constants: the sub-block flag's)
constexpr int kRdCbfLamMax = 1 << 23;     // above lamq of rd_cbf_lambda 4 at QpY 51, 10 bits (4,781,507)

// raster index 4 y + x of scan position q of a 4x4 group (up-right diagonal, 6.5.3) in nibble q
constexpr uint64_t diag4_packed() {
  uint64_t v = 0;
  int q = 0;
  for (int d = 0; d < 7; ++d)
    for (int y = d < 4 ? d : 3; y >= 0 && d - y < 4; --y) v |= static_cast<uint64_t>(4 * y + d - y) << (4 * q++);
  return v;
}
constexpr uint64_t kDiag4 = diag4_packed();
static_assert(kDiag4 == 0xFBE7AD369C258140ull, "diagonal scan of a 4x4 group");

// Rate of a TU's levels (diagonal scan) in 1 / 16 bit, on every lane.  One lane per 4x4 group.
// With pmax the largest coder scan position of a non-zero level: rate(l, false, pmax) there,
// rate(l, true, p) at every p < pmax of a group that holds a level, and kRdoqCsbf1 / kRdoqCsbf0
// for every group strictly between group 0 and pmax's.  Every lane calls; the levels must be
// visible to the wave (wave_sync after their stores).
__device__ __forceinline__ int tu_rate(const int16_t* lev, int stride, int lg) {
  const int nsb = 1 << (lg - 2), lane = lane_id();
  const bool on = lane < nsb * nsb;
  const int gx = lane & (nsb - 1), gy = lane >> (lg - 2);
  const int gi = on ? rdoq_scan_index(0, lg - 2, gx, gy) : 0;
  const int16_t* g = lev + gy * 4 * stride + gx * 4;
  auto at = [&](int q) {  // |level| at scan position q of the group
    const int xy = static_cast<int>(kDiag4 >> (4 * q)) & 15;
    const int v = g[(xy >> 2) * stride + (xy & 3)];
    return v < 0 ? -v : v;
  };
  int last = -1;
  if (on) {
#pragma unroll 1
    for (int q = 0; q < 16; ++q)
      if (at(q)) last = q;
  }
  const int pmax = __builtin_amdgcn_readfirstlane(-min64(last < 0 ? 1 : -(16 * gi + last)));
  if (pmax < 0) return 0;
  int r = 0;
  if (last >= 0) {
    const int qe = gi == (pmax >> 4) ? (pmax & 15) : 15;
#pragma unroll 1
    for (int q = 0; q <= qe; ++q) r += rdoq_rate(at(q), 16 * gi + q < pmax, 16 * gi + q);
  }
  if (on && gi > 0 && gi < (pmax >> 4)) r += last >= 0 ? kRdoqCsbf1 : kRdoqCsbf0;
  return __builtin_amdgcn_readfirstlane(sum64(r));
}

// SSD of clip(pred + R) against the source over an n x n TU (wave reduction, on every lane).
// At most 1024 * 1023^2 < 2^31.
__device__ __forceinline__ int tu_recon_ssd(const uint16_t* pred, int pstride, const int* R, const uint16_t* src,
                                            int sstride, int lg, int maxv) {
  const int n = 1 << lg;
  int e = 0;
#pragma unroll 1
  for (int i = lane_id(); i < n * n; i += 64) {
    const int y = i >> lg, x = i & (n - 1);
    int v = pred[y * pstride + x] + R[y * 32 + x];
    v = v < 0 ? 0 : (v > maxv ? maxv : v);
    const int d = static_cast<int>(src[static_cast<size_t>(y) * sstride + x]) - v;
    e += d * d;
  }
  return __builtin_amdgcn_readfirstlane(sum64(e));
}

__device__ __forceinline__ bool rd_cbf_clears(int d0, int d1, int rb, int lamq) {
  return 256ll * d0 + static_cast<long long>(lamq) * kRdCbf0 <= 256ll * d1 + static_cast<long long>(lamq) * (rb + kRdCbf1);
}

// The check on one TU right after its transform_quant_block call returned nz: pred / src / lev
// point at the TU's first sample, R (row stride 32) holds its reconstructed residual, d0 its D0.
// Returns the TU's flag after the check; a cleared TU's levels and R are zero.  d1 / rb: the
// terms of the comparison (d0 and 0 for a TU that had no levels: it is not examined).
__device__ __forceinline__ bool rd_cbf_tu(bool nz, const uint16_t* pred, int pstride, int* R, const uint16_t* src,
                                          int sstride, int16_t* lev, int lstride, int lg, int maxv, int lamq, int d0,
                                          int& d1, int& rb) {
  d1 = d0;
  rb = 0;
  if (!nz) return false;
  d1 = tu_recon_ssd(pred, pstride, R, src, sstride, lg, maxv);
  rb = tu_rate(lev, lstride, lg);
  if (!rd_cbf_clears(d0, d1, rb, lamq)) return true;
  const int n = 1 << lg;
#pragma unroll 1
  for (int i = lane_id(); i < n * n; i += 64) {
    const int y = i >> lg, x = i & (n - 1);
    lev[y * lstride + x] = 0;
    R[y * 32 + x] = 0;
  }
  wave_sync();
  return false;
}
__device__ __forceinline__ bool rd_cbf_tu(bool nz, const uint16_t* pred, int pstride, int* R, const uint16_t* src,
                                          int sstride, int16_t* lev, int lstride, int lg, int maxv, int lamq, int d0) {
  int d1, rb;
  return rd_cbf_tu(nz, pred, pstride, R, src, sstride, lev, lstride, lg, maxv, lamq, d0, d1, rb);
}

}  // namespace hv
}  // namespace gpu
}  // namespace mivc
