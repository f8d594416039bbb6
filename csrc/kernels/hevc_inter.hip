// HEVC P pictures on gfx950.
//
// Motion comes from the batched motion-estimation kernel (me.hip) run on 8-bit
// proxies of the source and the reference reconstruction (one vector per 16x16
// block).  Here:
//
// * hevc_p_decide (grid = CTBs x slots, one wave): per 16x16 quadrant, inter (ME
//   cost) versus the best intra choice of the open-loop analysis (16x16 or four
//   8x8); four inter quadrants with one vector become a 32x32 inter CU.  Writes the
//   CTB split and the CU records (the CABAC writer turns zero-residual CUs whose
//   vector equals a merge candidate into skip CUs).
// * hevc_inter_cu (grid = CTBs*4 x slots, one wave per 16x16 quadrant or 32x32
//   CU): normative HEVC motion compensation (8-tap luma, 4-tap chroma, separable
//   through LDS, default weighted prediction), transform / quantisation with the
//   inter rounding offset, reconstruction.  No dependency between CUs: fully
//   parallel; the intra CUs of the picture are then coded by hevc_intra_recon.
#include "hevc_inter_cu.h"
#include "launch.h"

namespace mivc {
namespace gpu {

__device__ __forceinline__ int lambda_satd_i(int qp, int bd) {
  return static_cast<int>(0.755f * exp2f((qp - 12) / 6.0f) * static_cast<float>(1 << (bd - 8)) + 0.5f);
}

// ============================================================== decision
__global__ __launch_bounds__(64) void hevc_p_decide(HevcInterArgs a) {
  const HevcGeom& g = a.g;
  const int ci = blockIdx.x, slot = blockIdx.y;
  if (a.run[slot] != 2) return;
  const int lane = threadIdx.x;
  const int rx = ci % g.wctb, ry = ci / g.wctb;
  const size_t cb = static_cast<size_t>(slot) * g.nctb() + ci;
  const int* cd = a.cand + cb * kCandStride;
  const int wmb = g.W / 16, nmb = wmb * (g.H / 16);
  const int qp = a.qp[cb];
  const int lam = lambda_satd_i(qp, a.bd);
  __shared__ int s_inter[4], s_mvx[4], s_mvy[4], s_mv1x[4], s_mv1y[4], s_dir[4], s_split8[4], s_intra[4], s_isplit[4];
  __shared__ uint32_t s_mv8[4][4];
  __shared__ int s_split;
  if (lane < 4) {
    const int q = lane;
    const int mb = (ry * 2 + (q >> 1)) * wmb + rx * 2 + (q & 1);
    const size_t o = static_cast<size_t>(slot) * nmb + mb;
    const int inter = (a.me_cost[o] << (a.bd - 8)) + lam * 3;
    int s8 = 0;
    for (int r = 0; r < 4; ++r) s8 += cd[5 + q * 4 + r];
    const int c16 = cd[1 + q];
    s_split8[q] = s8 < c16;
    s_intra[q] = (s8 < c16 ? s8 : c16) + lam * a.intra_bias;
    s_inter[q] = inter;
    if (a.dirb) {
      const int16_t* m = a.mvb + o * 4;
      s_mvx[q] = m[0];
      s_mvy[q] = m[1];
      s_mv1x[q] = m[2];
      s_mv1y[q] = m[3];
      s_dir[q] = a.dirb[o];
    } else {
      s_mvx[q] = a.mv[o * 2];
      s_mvy[q] = a.mv[o * 2 + 1];
      s_mv1x[q] = s_mv1y[q] = 0;
      s_dir[q] = hevc::DIR_L0;
    }
    // an inter quadrant split into four 8x8 inter CUs: RefPicList0[0] list-0 motion whose four
    // quadrant vectors differ
    s_isplit[q] = 0;
    if (a.mv8 && s_dir[q] == hevc::DIR_L0) {
      const uint32_t* m8 = reinterpret_cast<const uint32_t*>(a.mv8 + o * 8);
      for (int k = 0; k < 4; ++k) s_mv8[q][k] = m8[k];
      s_isplit[q] = m8[0] != m8[1] || m8[0] != m8[2] || m8[0] != m8[3];
    }
  }
  __syncthreads();
  if (lane == 0) {
    int n_inter = 0, icost = 0, tcost = 0;
    for (int q = 0; q < 4; ++q) {
      const bool inter = s_inter[q] < s_intra[q];
      n_inter += inter;
      icost += s_intra[q];
      tcost += inter ? s_inter[q] : s_intra[q];
    }
    int split;
    if (n_inter == 0) {
      // the analysis' own 32-vs-16 choice
      split = icost < cd[0] ? 1 : 0;
      for (int q = 0; q < 4; ++q) split |= (split & 1) && s_split8[q] ? 1 << (1 + q) : 0;
      for (int q = 0; q < 4; ++q) s_inter[q] = 0x7FFFFFFF;  // mark intra
    } else {
      bool same = n_inter == 4 && !s_isplit[0];
      for (int q = 1; q < 4; ++q)
        same = same && s_dir[q] == s_dir[0] && s_mvx[q] == s_mvx[0] && s_mvy[q] == s_mvy[0] && s_mv1x[q] == s_mv1x[0] &&
               s_mv1y[q] == s_mv1y[0] && !s_isplit[q];
      split = same ? 0 : 1;
      for (int q = 0; q < 4; ++q) {
        const bool inter = s_inter[q] < s_intra[q];
        if (!inter && s_split8[q]) split |= 1 << (1 + q);
        if (inter && s_isplit[q]) split |= 1 << (1 + q);
        if (!inter) s_inter[q] = 0x7FFFFFFF;
      }
    }
    s_split = split;
    a.ctu[cb].split = static_cast<uint8_t>(split);
    a.ctu[cb].qp = static_cast<int8_t>(qp);
  }
  __syncthreads();
  if (lane < 16) {
    const int k = lane;
    const int gx = (k & 1) | ((k >> 1) & 2), gy = ((k >> 1) & 1) | ((k >> 2) & 2);
    const int q = (gx >> 1) + 2 * (gy >> 1);
    const int split = s_split;
    CuInfo c{};
    int lg;
    if (!(split & 1)) lg = 5;
    else if (!((split >> (1 + q)) & 1)) lg = 4;
    else lg = 3;
    c.flags = static_cast<uint8_t>((lg - 3) << 1);
    if (s_inter[q] != 0x7FFFFFFF) {
      c.pred = hevc::CU_INTER;
      c.mv[0] = static_cast<int16_t>(s_mvx[q]);
      c.mv[1] = static_cast<int16_t>(s_mvy[q]);
      if (lg == 3) {  // an 8x8 inter CU: its quadrant's vector of the 16x16 block
        const uint32_t w = s_mv8[q][(gx & 1) | ((gy & 1) << 1)];
        c.mv[0] = static_cast<int16_t>(w & 0xFFFFu);
        c.mv[1] = static_cast<int16_t>(w >> 16);
      }
      c.mv1[0] = static_cast<int16_t>(s_mv1x[q]);
      c.mv1[1] = static_cast<int16_t>(s_mv1y[q]);
      c.dir = static_cast<uint8_t>(s_dir[q] & 3);
      c.pad[0] = static_cast<uint8_t>((s_dir[q] >> 2) & 3);  // list-0 refIdx
    } else {
      c.pred = hevc::CU_INTRA;
      const int idx = lg == 5 ? 0 : (lg == 4 ? 1 + q : 5 + k);
      c.mode = static_cast<uint8_t>(cd[21 + idx]);
      if (lg == 3 && cd[42 + k]) set_nxn(c, cd[42 + k]);
    }
    a.cu[cb * 16 + k] = c;
  }
}

}  // namespace gpu
}  // namespace mivc

using namespace mivc::gpu;

extern "C" void mivc_launch_hevc_inter(int B, int W, int H, const uint16_t* sy, const uint16_t* su, const uint16_t* sv,
                                       const uint16_t* fy, const uint16_t* fu, const uint16_t* fv, uint16_t* ry,
                                       uint16_t* ru, uint16_t* rv, void* ctu, void* cu, int16_t* cy, int16_t* cu_,
                                       int16_t* cv, const int* qp, const int8_t* run, const int* cand,
                                       const int16_t* mv, const int* me_cost, int bd, int tu_split, int sdh,
                                       int intra_bias, void* stream, const int16_t* mvb, const uint8_t* dirb,
                                       const uint16_t* f1y, const uint16_t* f1u, const uint16_t* f1v,
                                       const int16_t* wp, const uint16_t* const* xref, const int16_t* mv8, int rdoq,
                                       int rdoq_lam, const int16_t* wpb, const int* rd_lamq,
                                       unsigned long long* tsmap, const int* ts_lamq, int* ts_count) {
  HevcInterArgs a;
  a.rd_lamq = rd_lamq;
  a.tsmap = tsmap;  // all three or none (the binding checks)
  a.ts_lamq = ts_lamq;
  a.ts_count = ts_count;
  a.wp = wp;
  a.wpb = wpb;
  a.mv8 = mv8;
  for (int r = 0; r < 3; ++r) {  // xref: [3 x (y, u, v)] of RefPicList0[1 ..] (null: list-0[0])
    a.xref_y[r] = xref && xref[3 * r] ? xref[3 * r] : fy;
    a.xref_u[r] = xref && xref[3 * r + 1] ? xref[3 * r + 1] : fu;
    a.xref_v[r] = xref && xref[3 * r + 2] ? xref[3 * r + 2] : fv;
  }
  a.g = HevcGeom{B, W, H, W / 32, H / 32};
  a.src_y = sy;
  a.src_u = su;
  a.src_v = sv;
  a.ref_y = fy;
  a.ref_u = fu;
  a.ref_v = fv;
  a.rec_y = ry;
  a.rec_u = ru;
  a.rec_v = rv;
  a.ctu = static_cast<CtuInfo*>(ctu);
  a.cu = static_cast<CuInfo*>(cu);
  a.coef_y = cy;
  a.coef_u = cu_;
  a.coef_v = cv;
  a.qp = qp;
  a.run = run;
  a.cand = cand;
  a.mv = mv;
  a.mvb = mvb;
  a.dirb = dirb;
  a.ref1_y = f1y;
  a.ref1_u = f1u;
  a.ref1_v = f1v;
  a.me_cost = me_cost;
  a.bd = bd;
  a.tu_split = tu_split;
  a.sdh = sdh;
  a.rdoq = rdoq;
  a.rdoq_lam = rdoq_lam;
  a.intra_bias = intra_bias;
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(hevc_p_decide, dim3(a.g.nctb(), B), dim3(64), 0, s, a);
  const dim3 grid(a.g.nctb() * 4, B);
  if (tsmap) {  // transform skip on the chroma 4x4 TUs of 8x8 CUs: the TSK instances
    if (rd_lamq) launch_hevc_inter_cu_tsk_rdc(a, grid, s, tu_split != 0, rdoq != 0, wpb != nullptr);
    else launch_hevc_inter_cu_tsk(a, grid, s, tu_split != 0, rdoq != 0, wpb != nullptr);
    return;
  }
  if (rd_lamq) {  // every TU checked against no levels: the RDC instances
    launch_hevc_inter_cu_rdc(a, grid, s, tu_split != 0, rdoq != 0, wpb != nullptr);
    return;
  }
  if (wpb) {  // B pictures with explicit weights (the caller checks: B motion, no list-0 table)
    if (rdoq) {
      if (tu_split) hipLaunchKernelGGL((hevc_inter_cu<true, true, true, false>), grid, dim3(64), 0, s, a);
      else hipLaunchKernelGGL((hevc_inter_cu<false, true, true, false>), grid, dim3(64), 0, s, a);
    } else {
      if (tu_split) hipLaunchKernelGGL((hevc_inter_cu<true, false, true, false>), grid, dim3(64), 0, s, a);
      else hipLaunchKernelGGL((hevc_inter_cu<false, false, true, false>), grid, dim3(64), 0, s, a);
    }
  } else if (rdoq) {
    if (tu_split) hipLaunchKernelGGL((hevc_inter_cu<true, true, false, false>), grid, dim3(64), 0, s, a);
    else hipLaunchKernelGGL((hevc_inter_cu<false, true, false, false>), grid, dim3(64), 0, s, a);
  } else {
    if (tu_split) hipLaunchKernelGGL((hevc_inter_cu<true, false, false, false>), grid, dim3(64), 0, s, a);
    else hipLaunchKernelGGL((hevc_inter_cu<false, false, false, false>), grid, dim3(64), 0, s, a);
  }
}
