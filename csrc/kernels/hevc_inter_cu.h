// hevc_inter_cu: motion compensation, transform / quantisation and reconstruction of the inter
// CUs of a P or B picture (one wave per 16x16 quadrant or 32x32 CU; see hevc_inter.hip).  The
// kernel template lives here because its instances are spread over two translation units:
// hevc_inter.hip holds the instances without the rate-distortion check of hevc_rdcbf.h,
// hevc_inter_rdcbf.hip those with it, so the former are compiled exactly as before the check
// existed (with all sixteen in one file the old eight came out with other registers and scratch).
#pragma once
#include "hevc_common.h"
#include "hevc_mc.h"
#include "hevc_rdcbf.h"
#include "hevc_tskip.h"

namespace mivc {
namespace gpu {

using hevc::CtuInfo;
using hevc::CuInfo;

struct HevcInterArgs {
  HevcGeom g;
  const uint16_t *src_y, *src_u, *src_v;
  const uint16_t *ref_y, *ref_u, *ref_v;
  uint16_t *rec_y, *rec_u, *rec_v;
  CtuInfo* ctu;
  CuInfo* cu;
  int16_t *coef_y, *coef_u, *coef_v;
  const int* qp;          // [B, nctb] QpY per CTB
  const int8_t* run;
  const int* cand;       // [B, nctb, kCandStride] intra analysis: best cost / mode per CU, NxN PUs
  const int16_t* mv;     // [B, nmb16, 2] quarter-sample vectors per 16x16 block (P pictures)
  const int16_t* mvb;    // [B, nmb16, 4] B pictures: (L0 x, y, L1 x, y) per 16x16 block, or null
  const uint8_t* dirb;   // [B, nmb16] B pictures: CuDir per 16x16 block
  const uint16_t *ref1_y, *ref1_u, *ref1_v;  // RefPicList1[0] (B pictures)
  const int* me_cost;    // [B, nmb16] (8-bit proxy units)
  int bd;
  int tu_split;          // inter CUs may code their residual as four quarter TUs (RD choice)
  int sdh;               // sign data hiding in the quantiser
  int intra_bias;        // lambda multiples added to the open-loop intra costs of P pictures
  // explicit weighted prediction of P pictures (x265 --weightp; pred_weight_table with
  // log2 denominators kWpLog2 for luma and chroma): [B][6] = weight, offset (8-bit units) of
  // Y, Cb, Cr; weight 0 = the slot's picture is not weighted.  Null: default weighting.
  const int16_t* wp;
  // x265 --weightb (the WB instances; B pictures): [B][2][6], the same rows for RefPicList0[0] and
  // RefPicList1[0]; a slot with a weight on either list predicts every CU by the explicit
  // formulas, a list without weight entering as (64, 0)
  const int16_t* wpb;
  // x265 --ref: RefPicList0[1 ..] reconstructions of a P picture (a motion's direction byte in
  // dirb carries its list-0 refIdx in bits 2-3; the CU records take it in pad[0]); explicit
  // weights apply to RefPicList0[0] only
  const uint16_t *xref_y[3], *xref_u[3], *xref_v[3];
  // 8x8 inter CUs (P pictures, x265's minimum CU): [B, nmb16, 4, 2] per-quadrant vectors of
  // each 16x16 block (p_part8x8 in its HEVC form; all equal = no split); null: 16x16 / 32x32 only
  const int16_t* mv8;
  int rdoq, rdoq_lam;    // x265 --rdoq-level and its lambda (hevc_rdoq.h); the RDOQ instances read them
  const int* rd_lamq;    // [52] SSD lambda per QpY in 1 / 16 units (hevc_rdcbf.h); the RDC instances read it
  // x265 --tskip (hevc_tskip.h; the TSK instances read them): the map [B, nctb, 2], the lambda
  // table [52] and the counters of TUs coded with the flag set (this kernel adds to entry 2)
  unsigned long long* tsmap;
  const int* ts_lamq;
  int* ts_count;
};

// plane c of RefPicList0[r] (constant indices only: no scratch)
__device__ __forceinline__ const uint16_t* l0_plane(const HevcInterArgs& a, int c, int r) {
  const uint16_t* const* x = c == 0 ? a.xref_y : (c == 1 ? a.xref_u : a.xref_v);
  return r == 0 ? (c == 0 ? a.ref_y : (c == 1 ? a.ref_u : a.ref_v)) : (r == 1 ? x[0] : (r == 2 ? x[1] : x[2]));
}

// rate proxy of a block's levels (bits): ~3 + 2 log2|l| per non-zero level (wave reduction)
__device__ __forceinline__ int level_bits(const int16_t* lev, int stride, int n) {
  int b = 0;
  for (int i = lane_id(); i < n * n; i += 64) {
    const int v = lev[(i / n) * stride + i % n];
    const int m = v < 0 ? -v : v;
    if (m) b += 3 + 2 * (31 - __builtin_clz(m));
  }
  return sum64(b);
}

// SSD of clip(pred + R) against the source block (wave reduction; 64-bit: 32x32 at 10 bits)
template <typename SH>
__device__ __forceinline__ long long recon_ssd(const SH& S, const int* R, const uint16_t* src, int pw, int bx,
                                               int by, int n, int maxv) {
  long long e = 0;
  for (int i = lane_id(); i < n * n; i += 64) {
    const int y = i / n, x = i - y * n;
    int v = S.pred[i] + R[y * 32 + x];
    v = v < 0 ? 0 : (v > maxv ? maxv : v);
    const int d = static_cast<int>(src[static_cast<size_t>(by + y) * pw + bx + x]) - v;
    e += d * d;
  }
  const int lo = static_cast<int>(e & 0x3FFFFFFF), hi = static_cast<int>(e >> 30);
  return (static_cast<long long>(sum64(hi)) << 30) + sum64(lo);
}


// TSPLIT: the instance with the residual-quadtree choice (its register footprint stays out of
// the default instance); RDOQ: the instances with rate-distortion optimised quantisation; WB: the
// instances of B pictures with explicit weights (x265 --weightb); RDC: the instances that check
// every TU's levels against no levels by SSD + lambda * bits (hevc_rdcbf.h)
// (the RDC instances without the quadtree ask for two waves per SIMD, not three: the check's live
// values on top of the 168 registers of three would go to scratch; the LDS allows 2.5.  The
// quadtree instances run one wave per SIMD either way); TSK: the instances with the transform
// skip decision on the chroma 4x4 TUs of 8x8 CUs (hevc_tskip.h; registers as the RDC instances)
template <bool TSPLIT, bool RDOQ, bool WB, bool RDC, bool TSK = false>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu((RDC || TSK) && !TSPLIT ? 2 : 3, 8))) void hevc_inter_cu(HevcInterArgs a) {
  __shared__ typename std::conditional<TSPLIT, InterShared, InterSharedLean>::type S;
  __shared__ hv::DctLds D;
  const HevcGeom& g = a.g;
  const int task = blockIdx.x, slot = blockIdx.y;
  if (a.run[slot] != 2) return;
  const int ci = task >> 2, q = task & 3;
  const size_t cb = static_cast<size_t>(slot) * g.nctb() + ci;
  const int kq = q * 4;  // z-index of the quadrant's first granule
  CuInfo* cu = a.cu + cb * 16;
  const int pred = cu[kq].pred;
  const int lg = 3 + ((cu[kq].flags >> 1) & 3);
  if (pred != hevc::CU_INTER) return;
  if (lg == 5 && q != 0) return;  // the 32x32 CU is handled by quadrant 0
  hv::dct_lds_init(D);
  __syncthreads();
  const int lane = lane_id();
  const int n = 1 << lg;
  const int rx = ci % g.wctb, ry = ci / g.wctb;
  const int bd = a.bd, maxv = (1 << bd) - 1;
  const int qpy = a.qp[cb], off = 6 * (bd - 8);
  const int qpl = qpy + off, qpc = hevc::chroma_qp_map(clampi(qpy, -off, 57)) + off;
  int lamq = 0;
  if constexpr (RDC) lamq = a.rd_lamq[clampi(qpy, 0, 51)];
  int ts_lamq = 0;
  if constexpr (TSK) ts_lamq = a.ts_lamq[clampi(qpy, 0, 51)];
  // a quadrant split into 8x8 inter CUs (x265's minimum CU) codes them one after another
  const int ncu = lg == 3 ? 4 : 1;
  for (int j = 0; j < ncu; ++j) {
  const int kc = kq + j;  // the CU's first granule (z-order)
  const int X0 = rx * 32 + (lg == 5 ? 0 : (q & 1) * 16 + (lg == 3 ? (j & 1) * 8 : 0));
  const int Y0 = ry * 32 + (lg == 5 ? 0 : (q >> 1) * 16 + (lg == 3 ? (j >> 1) * 8 : 0));
  const int mvx = cu[kc].mv[0], mvy = cu[kc].mv[1], mv1x = cu[kc].mv1[0], mv1y = cu[kc].mv1[1];
  const int dir = hevc::cu_dir(cu[kc]);
  const int r0 = cu[kc].pad[0] & 3;  // list-0 refIdx
  // residual quadtree: the luma residual is transformed both as one TU and as four quarter
  // TUs; the cheaper by SSD + lambda * (level-bit proxy + TU overhead) wins, and chroma
  // follows the chosen structure (max_transform_hierarchy_depth_inter 1; 16x16+ CUs)
  int cbfq[4] = {0, 0, 0, 0};  // per quarter: bit c = component c has levels in that quarter's TU
  bool split = false;
  const int h = n >> 1;
  for (int c = 0; c < 3; ++c) {
    const int pw = c ? g.W / 2 : g.W, ph = c ? g.H / 2 : g.H, bs = c ? n / 2 : n;
    const int bx = c ? X0 / 2 : X0, by = c ? Y0 / 2 : Y0;
    const size_t ps = c ? g.csize() : g.ysize();
    const uint16_t* ref = l0_plane(a, c, r0) + slot * ps;
    const uint16_t* ref1 = a.ref1_y ? (c == 0 ? a.ref1_y : (c == 1 ? a.ref1_u : a.ref1_v)) + slot * ps : ref;
    const uint16_t* src = (c == 0 ? a.src_y : (c == 1 ? a.src_u : a.src_v)) + slot * ps;
    uint16_t* rec = (c == 0 ? a.rec_y : (c == 1 ? a.rec_u : a.rec_v)) + slot * ps;
    int16_t* lev = (c == 0 ? a.coef_y : (c == 1 ? a.coef_u : a.coef_v)) + slot * ps + static_cast<size_t>(by) * pw + bx;
    if constexpr (WB) {
      const int16_t* t = a.wpb + slot * 12;
      const bool on = t[0] != 0 || t[6] != 0;  // (a weighted list weights all three components)
      const int ww = on ? (t[2 * c] ? t[2 * c] : 64) : 0, wo = t[2 * c] ? t[2 * c + 1] : 0;
      const int ww1 = on ? (t[6 + 2 * c] ? t[6 + 2 * c] : 64) : 0, wo1 = t[6 + 2 * c] ? t[6 + 2 * c + 1] : 0;
      if (c == 0) mc_block<8, true>(S, ref, ref1, pw, ph, bx, by, bs, dir, mvx, mvy, mv1x, mv1y, bd, ww, wo, ww1, wo1);
      else mc_block<4, true>(S, ref, ref1, pw, ph, bx, by, bs, dir, mvx, mvy, mv1x, mv1y, bd, ww, wo, ww1, wo1);
    } else {
      const int ww = (a.wp && dir == hevc::DIR_L0 && r0 == 0) ? a.wp[slot * 6 + 2 * c] : 0;
      const int wo = ww ? a.wp[slot * 6 + 2 * c + 1] : 0;
      if (c == 0) mc_block<8>(S, ref, ref1, pw, ph, bx, by, bs, dir, mvx, mvy, mv1x, mv1y, bd, ww, wo);
      else mc_block<4>(S, ref, ref1, pw, ph, bx, by, bs, dir, mvx, mvy, mv1x, mv1y, bd, ww, wo);
    }
    // RDC: D0 = sum (src - pred)^2 of the block (with the quadtree per quarter: d0q); a lane
    // adds at most 16 squares below 2^20
    int d0 = 0, d0q0 = 0, d0q1 = 0, d0q2 = 0, d0q3 = 0;
    if constexpr (RDC) {
      for (int i = lane; i < bs * bs; i += 64) {
        const int y = i / bs, x = i - y * bs;
        const int r = static_cast<int>(src[static_cast<size_t>(by + y) * pw + bx + x]) - S.pred[i];
        S.R[y * 32 + x] = r;
        if (TSPLIT && c == 0) S.R2[y * 32 + x] = r;
        if constexpr (TSPLIT) {
          const int k = (y >= (bs >> 1) ? 2 : 0) + (x >= (bs >> 1) ? 1 : 0);
          d0q0 += k == 0 ? r * r : 0;
          d0q1 += k == 1 ? r * r : 0;
          d0q2 += k == 2 ? r * r : 0;
          d0q3 += k == 3 ? r * r : 0;
        } else {
          d0 += r * r;
        }
      }
      if constexpr (TSPLIT) {
        d0q0 = __builtin_amdgcn_readfirstlane(sum64(d0q0));
        d0q1 = __builtin_amdgcn_readfirstlane(sum64(d0q1));
        d0q2 = __builtin_amdgcn_readfirstlane(sum64(d0q2));
        d0q3 = __builtin_amdgcn_readfirstlane(sum64(d0q3));
        d0 = d0q0 + d0q1 + d0q2 + d0q3;
      } else {
        d0 = __builtin_amdgcn_readfirstlane(sum64(d0));
      }
    } else {
      for (int i = lane; i < bs * bs; i += 64) {
        const int y = i / bs, x = i - y * bs;
        const int r = static_cast<int>(src[static_cast<size_t>(by + y) * pw + bx + x]) - S.pred[i];
        S.R[y * 32 + x] = r;
        if (TSPLIT && c == 0) S.R2[y * 32 + x] = r;
      }
    }
    wave_sync();
    const int l2 = c ? lg - 1 : lg;
    const int qc = c ? qpc : qpl;
    auto tq = [&](int l2t) {  // inter TUs scan diagonally (7.4.9.11)
      hv::TqParams t{l2t, bd, qc, false, false, a.sdh ? 0 : -1};
      if constexpr (RDOQ) {
        t.rdoq = a.rdoq;
        t.rdoq_lam = a.rdoq_lam;
      }
      return t;
    };
    // RDC: the check of the TU at offset (ox, oy) of the block, of size 1 << l2t, whose
    // transform_quant_block call returned nz (R its residual, tl its levels of row stride ts)
    auto rdc = [&](bool nz, int ox, int oy, int l2t, int* R, int16_t* tl, int ts, int d0t) {
      return hv::rd_cbf_tu(nz, S.pred + oy * bs + ox, bs, R, src + static_cast<size_t>(by + oy) * pw + bx + ox, pw, tl, ts,
                           l2t, maxv, lamq, d0t);
    };
    auto d0quarter = [&](int k) { return k == 0 ? d0q0 : (k == 1 ? d0q1 : (k == 2 ? d0q2 : d0q3)); };
    bool coded = false;
    if constexpr (TSPLIT) {
      if (lg >= 4) {
      coded = c == 0 || split;
      if (c == 0) {
        bool nz = hv::transform_quant_block<RDOQ>(D, S.R, S.S, lev, pw, tq(l2));
        if constexpr (RDC) nz = rdc(nz, 0, 0, l2, S.R, lev, pw, d0);
        for (int k = 0; k < 4; ++k) cbfq[k] = nz;
        {
          bool nzq[4];
          for (int k = 0; k < 4; ++k) {
            const int o = (k >> 1) * h * 32 + (k & 1) * h;
            nzq[k] = hv::transform_quant_block<RDOQ>(D, S.R2 + o, S.S, S.lev2 + o, 32, tq(l2 - 1));
            if constexpr (RDC) nzq[k] = rdc(nzq[k], (k & 1) * h, (k >> 1) * h, l2 - 1, S.R2 + o, S.lev2 + o, 32, d0quarter(k));
          }
          const bool any = nzq[0] || nzq[1] || nzq[2] || nzq[3];
          if (any) {
            // lambda for SSD (HM: 0.57 * 2^((QP - 12) / 3), at the coded bit depth)
            const float lam = 0.57f * exp2f((qpy - 12) / 3.0f) * static_cast<float>(1 << (2 * (bd - 8)));
            const long long d1 = recon_ssd(S, S.R, src, pw, bx, by, n, maxv);
            const long long d4 = recon_ssd(S, S.R2, src, pw, bx, by, n, maxv);
            const int b1 = level_bits(lev, pw, n) + (nz ? 2 * lg + 2 : 0);
            const int b4 = level_bits(S.lev2, 32, n) + 4 + (nzq[0] + nzq[1] + nzq[2] + nzq[3]) * (2 * lg);
            split = static_cast<float>(d4) + lam * b4 < static_cast<float>(d1) + lam * b1;
          }
          if (split) {
            for (int i = lane; i < n * n; i += 64) {
              const int y = i / n, x = i - y * n;
              lev[y * pw + x] = S.lev2[y * 32 + x];
              S.R[y * 32 + x] = S.R2[y * 32 + x];
            }
            for (int k = 0; k < 4; ++k) cbfq[k] = nzq[k];
          }
          wave_sync();
        }
      } else if (split) {
        const int hc = bs >> 1;
        for (int k = 0; k < 4; ++k) {
          const int o = (k >> 1) * hc * 32 + (k & 1) * hc;
          bool nz = hv::transform_quant_block<RDOQ>(D, S.R + o, S.S, lev + (k >> 1) * hc * pw + (k & 1) * hc, pw,
                                                    tq(l2 - 1));
          if constexpr (RDC)
            nz = rdc(nz, (k & 1) * hc, (k >> 1) * hc, l2 - 1, S.R + o, lev + (k >> 1) * hc * pw + (k & 1) * hc, pw, d0quarter(k));
          cbfq[k] |= nz << c;
        }
      }
      }
    }
    if (!coded) {
      bool nz = hv::transform_quant_block<RDOQ>(D, S.R, S.S, lev, pw, tq(l2));
      bool ts = false;
      if constexpr (TSK) {  // the chroma 4x4 TU of an 8x8 CU: transform skip against the transform
        if (c > 0 && lg == 3)
          nz = hv::tskip_tu<RDOQ>(D, nz, S.pred, bs, S.R, S.S, src + static_cast<size_t>(by) * pw + bx, pw, lev, pw, tq(l2), 0,
                                  maxv, ts_lamq, ts);
      }
      if constexpr (RDC) nz = rdc(nz, 0, 0, l2, S.R, lev, pw, d0);
      if constexpr (TSK) {
        if (c > 0 && lg == 3 && lane == 0) {  // (a TU the check cleared codes no flag)
          hv::tsmap_put(a.tsmap, cb, c, (bx & 15) >> 2, (by & 15) >> 2, ts && nz);
          if (ts && nz) atomicAdd(a.ts_count + 2, 1);
        }
      }
      for (int k = 0; k < 4; ++k) cbfq[k] |= nz << c;
    }
    // (a block without levels has an all-zero dequantised residual in R)
    for (int i = lane; i < bs * bs; i += 64) {
      const int y = i / bs, x = i - y * bs;
      int v = S.pred[i] + S.R[y * 32 + x];
      rec[static_cast<size_t>(by + y) * pw + bx + x] = static_cast<uint16_t>(v < 0 ? 0 : (v > maxv ? maxv : v));
    }
    wave_sync();
  }
  // granule records: split flag; cbf = that of the TU covering the granule
  const int ng = lg == 5 ? 16 : (lg == 4 ? 4 : 1);
  if (lane < ng) {
    const int k = lg == 5 ? lane >> 2 : lane;  // z-order: the quarter of a 32x32 CU holds 4 granules
    cu[kc + lane].cbf = static_cast<uint8_t>(split ? cbfq[k] : cbfq[0]);
    if (split) cu[kc + lane].flags |= 16;
  }
  }
}

// the RDC instances (hevc_inter_rdcbf.hip); a.rd_lamq is set
void launch_hevc_inter_cu_rdc(const HevcInterArgs& a, dim3 grid, hipStream_t s, bool tu_split, bool rdoq, bool wb);
// the TSK instances without / with the check (hevc_inter_tskip.hip, hevc_inter_tskip_rdc.hip);
// a.tsmap, a.ts_lamq and a.ts_count are set
void launch_hevc_inter_cu_tsk(const HevcInterArgs& a, dim3 grid, hipStream_t s, bool tu_split, bool rdoq, bool wb);
void launch_hevc_inter_cu_tsk_rdc(const HevcInterArgs& a, dim3 grid, hipStream_t s, bool tu_split, bool rdoq, bool wb);

}  // namespace gpu
}  // namespace mivc
