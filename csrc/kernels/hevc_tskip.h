// Transform skip decision of a 4x4 TU (HevcParams.tskip, x265 --tskip): after transform_quant_block
// produced candidate A, candidate B sends the quantised residual samples themselves
// (transform_quant_block<RDOQ, true>: the residual << (13 - bd) through the same quantiser, the
// dequantised levels rescaled per 8.6.4.2 with transform_skip_flag), and B replaces A when
//   256 * D_B + lamq * (R_B + kTsFlag + kRdCbf1) < J_A                       (int64, ties keep A)
//   J_A = 256 * D_A + lamq * (R_A + kTsFlag + kRdCbf1) with levels, else 256 * D0 + lamq * kRdCbf0
// with exact SSDs, rates from the static bin costs of hevc_rdoq.h over the TU's own scan and lamq
// from the table of hevc_rdcbf.h built with tskip_lambda.  A B without levels is never chosen.
// tests/ref_models_hevc_tskip.py is the normative text and the numpy model the probe launch
// (hevc_tskip_probe.hip) is compared with exactly.  Only the transform skip instances of
// hevc_intra_recon and hevc_inter_cu include any of this.
#pragma once
#include "hevc_common.h"
#include "hevc_rdcbf.h"

namespace mivc {
namespace gpu {
namespace hv {

constexpr int kTsFlag = 16;  // transform_skip_flag: one bit (both contexts start at initValue 139)

// Rate of a 4x4 TU's levels over scan `scan` in 1 / 16 bit, on every lane: lane 4 y + x holds the
// level at (x, y).  Every lane calls; the levels must be visible to the wave.
__device__ __forceinline__ int tu_rate4(const int16_t* lev, int stride, int scan) {
  const int lane = lane_id();
  int a = 0, q = -1;
  if (lane < 16) {
    const int v = lev[(lane >> 2) * stride + (lane & 3)];
    a = v < 0 ? -v : v;
    q = rdoq_scan_index(scan, 2, lane & 3, lane >> 2);
  }
  const int pmax = __builtin_amdgcn_readfirstlane(-min64(a ? -q : 1));
  if (pmax < 0) return 0;
  const int r = (q >= 0 && q <= pmax) ? rdoq_rate(a, q < pmax, q) : 0;
  return __builtin_amdgcn_readfirstlane(sum64(r));
}

__device__ __forceinline__ bool tskip_wins(bool nz_a, int d0, int d_a, int r_a, int d_b, int r_b, int lamq) {
  const long long lam = lamq;
  const long long jb = 256ll * d_b + lam * (r_b + kTsFlag + kRdCbf1);
  const long long ja = nz_a ? 256ll * d_a + lam * (r_a + kTsFlag + kRdCbf1) : 256ll * d0 + lam * kRdCbf0;
  return jb < ja;
}

// The terms of the comparison: D_A (D0 for an A without levels), R_A, D_B, R_B (D0 and 0 for a B
// without levels: it is not examined further)
struct TskipTerms {
  int d_a, r_a, d_b, r_b;
};

// The decision on one 4x4 TU right after its transform_quant_block<RDOQ> call returned nz: pred /
// src / lev point at the TU's first sample, R (row stride 32) holds A's reconstructed residual
// (zero without levels), p the call's parameters, scan the TU's scanIdx.  On return lev and R hold
// the winner's levels and residual, ts whether that is B; returns the TU's flag.  Every lane calls.
template <bool RDOQ>
__device__ __forceinline__ bool tskip_tu(const DctLds& D, bool nz, const uint16_t* pred, int pstride, int* R, int* S,
                                         const uint16_t* src, int sstride, int16_t* lev, int lstride, const TqParams& p,
                                         int scan, int maxv, int lamq, bool& ts, TskipTerms& t) {
  const int lane = lane_id(), y = (lane >> 2) & 3, x = lane & 3;
  const bool in = lane < 16;
  // A's levels and residual stay in registers while B uses lev / R
  const int res = in ? static_cast<int>(src[static_cast<size_t>(y) * sstride + x]) - pred[y * pstride + x] : 0;
  const int d0 = __builtin_amdgcn_readfirstlane(sum64(res * res));
  t.d_a = nz ? tu_recon_ssd(pred, pstride, R, src, sstride, 2, maxv) : d0;
  t.r_a = nz ? tu_rate4(lev, lstride, scan) : 0;
  const int la = in ? lev[y * lstride + x] : 0, ra = in ? R[y * 32 + x] : 0;
  wave_sync();
  if (in) R[y * 32 + x] = res;
  wave_sync();
  const bool nzb = transform_quant_block<RDOQ, true>(D, R, S, lev, lstride, p);
  t.d_b = d0;
  t.r_b = 0;
  ts = false;
  if (nzb) {
    t.d_b = tu_recon_ssd(pred, pstride, R, src, sstride, 2, maxv);
    t.r_b = tu_rate4(lev, lstride, scan);
    ts = tskip_wins(nz, d0, t.d_a, t.r_a, t.d_b, t.r_b, lamq);
  }
  if (ts) return true;
  if (in) {
    lev[y * lstride + x] = static_cast<int16_t>(la);
    R[y * 32 + x] = ra;
  }
  wave_sync();
  return nz;
}
template <bool RDOQ>
__device__ __forceinline__ bool tskip_tu(const DctLds& D, bool nz, const uint16_t* pred, int pstride, int* R, int* S,
                                         const uint16_t* src, int sstride, int16_t* lev, int lstride, const TqParams& p,
                                         int scan, int maxv, int lamq, bool& ts) {
  TskipTerms t;
  return tskip_tu<RDOQ>(D, nz, pred, pstride, R, S, src, sstride, lev, lstride, p, scan, maxv, lamq, ts, t);
}

// Bit of a 4x4 TU in its CTB's words of the transform skip map (laid out like the sub-block
// map: word 0 luma bits by * 8 + bx, word 1 Cb bits 0-15 and Cr bits 16-31): set or cleared by
// the one wave that codes the TU, so the map does not depend on the order of the waves (the
// components' workgroups share word 1: atomics on disjoint bits).  comp 0 / 1 / 2; (bx, by): the
// TU's 4x4 position in the component's part of the CTB.  One lane calls.
__device__ __forceinline__ void tsmap_put(unsigned long long* tsmap, size_t ctb, int comp, int bx, int by, bool ts) {
  const unsigned long long bit = comp == 0 ? 1ull << (by * 8 + bx) : 1ull << ((comp - 1) * 16 + by * 4 + bx);
  unsigned long long* w = tsmap + 2 * ctb + (comp ? 1 : 0);
  if (ts) atomicOr(w, bit);
  else atomicAnd(w, ~bit);
}

}  // namespace hv
}  // namespace gpu
}  // namespace mivc
