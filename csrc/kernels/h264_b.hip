// H.264 B-picture motion: the direct derivation and the B macroblock mode decision
// (x264's default --bframes 3 behind the reference's `-vcodec libx264`, server.go:69-70).
//
// By default the GPU codes B pictures with *temporal* direct prediction
// (direct_spatial_mv_pred_flag = 0, x264 --direct temporal): the direct motion of a macroblock
// depends only on the co-located macroblock of RefPicList1[0] and on POC distances (clause
// 8.4.1.2.3), never on its neighbours in the current picture, so every MB of every slot decides
// in parallel (spatial direct needs the neighbours' final motion: a raster-order dependency).
// That holds with a b-pyramid too: the co-located picture may then be the run's reference B
// (list-0 indices of its own, list-1-only blocks pointing at the next anchor), or a reference B
// stands in front of the anchors in list 0, so refIdxCol goes through each slot's
// MapColToList0 table (route.h col_to_list0).  A quadrant whose co-located reference is not in
// the current list 0 has no direct prediction (dref -1): its MB is never gated or coded
// B_Direct_16x16 / B_Skip, and only its other quadrants may be B_Direct_8x8 -- a stream that
// never asks the decoder for such a quadrant's direct motion is conforming.
//
//   b_direct_mv  (thread per MB)     direct MVs per list / 8x8 quadrant + the ME predictors
//   b_decide     (four MBs per wave) candidates B_L0_16x16 / B_L1_16x16 (the two ME searches),
//                                    B_Bi_16x16 (both ME vectors) and B_Direct_16x16 (B_Skip
//                                    when no residual survives): luma motion compensation from
//                                    the anchors' frame-level half-sample planes, 4x4 SATD,
//                                    cost = SATD + lambda * bits; writes the winner's MbHeader
//                                    motion fields and its luma prediction for encode_inter.
// and, for x264 --direct spatial:
//   b_spatial_decide                 the exact derivation priced in an MB wavefront
//   b_spatial_exact, b_spatial_fixup the fast path: b_decide prices an estimate, an integer
//                                    decoding-order pass makes it exact, a parallel pass re-predicts
#include "h264_mvpred.h"
#include "kcommon.h"
#include "launch.h"
#include "mb_row.h"
#include "qpel.h"

namespace mivc {
namespace gpu {

using h264::MbHeader;

constexpr int kMaxRefs = 4;  // list-0 pictures an encoder P picture may reference (x264 --ref)

struct BDirectArgs {
  Geom g;
  const MbHeader* col;      // [B, nmb] records of RefPicList1[0] (a P anchor, or a reference B)
  // per refIdxL0 = MapColToList0(refIdxCol): DistScaleFactor, ignored when direct_copy.  Without
  // cmap the map is the identity (the anchor's list 0 and the B picture's list 0 order the same
  // past anchors); with a b-pyramid (a reference B in front of the anchors in list 0, or as the
  // co-located picture with lists of its own) it is each slot's table (route.h col_to_list0)
  int dsf[kMaxRefs];
  int direct_copy[kMaxRefs];  // td == 0: mvL0 = mvCol, mvL1 = 0
  int16_t* dmv;             // [B, nmb, 2, 4, 2] direct vectors (list, quadrant, xy)
  // [B, nmb, 4] refIdxL0 of each quadrant's direct prediction (nullable: all 0); -1 = the
  // quadrant has no temporal direct prediction (its co-located reference is not in list 0:
  // zero vectors, and b_decide never codes it direct)
  int8_t* dref;
  // [B, nmb, 2] ME predictors L0 / L1: the mean (rounded half up) of the direct vectors of the
  // quadrants that have a direct prediction, zero when none has
  int16_t* pm0;
  int16_t* pm1;
  // routed (route.h): col is the record pool [B, nbuf, nmb]; B slots only, each with its own
  // co-located picture (RefPicList1[0]) and its own dsf / direct_copy (SlotRoute)
  const SlotRoute* rt;
  int nbuf;
  // spatial direct (nullable): colZeroFlag of the four quadrants (bit q; 8.4.1.2.2: the
  // co-located block is inter, its refIdxCol is 0 and both vector components are in -1..1)
  uint8_t* czero;
  const int8_t* cmap;  // [B, 2, 4] MapColToList0 offsets (route.h; nullable: identity)
};

// floor(s / n + 1/2) for n = 0..4 summands (0 for none): the ME predictor over the quadrants
// that have a direct prediction; n = 4 is (s + 2) >> 2
__device__ __forceinline__ int mean_half_up(int s, int n) {
  if (n == 4) return (s + 2) >> 2;
  if (n == 3) {
    const int x = 2 * s + 3, d = x / 6;
    return d - (x - d * 6 < 0 ? 1 : 0);
  }
  return n == 2 ? (s + 1) >> 1 : (n == 1 ? s : 0);
}

// The four quadrants' "no temporal direct prediction" bits of a dref word (bytes of -1)
__device__ __forceinline__ uint32_t dref_unavail(uint32_t drw) {
  return ((drw >> 7) & 1u) | ((drw >> 14) & 2u) | ((drw >> 21) & 4u) | ((drw >> 28) & 8u);
}

__global__ __launch_bounds__(256) void b_direct_mv(BDirectArgs a) {
  const int mb = blockIdx.x * 256 + threadIdx.x, slot = blockIdx.y;
  const int nmb = a.g.nmb();
  if (mb >= nmb || !route_active(a.rt, slot, SK_B)) return;
  const size_t o = static_cast<size_t>(slot) * nmb + mb;
  const MbHeader& c = a.col[route_index(a.rt, a.nbuf, slot, RO_L1) * nmb + mb];
  // a B picture as the co-located one (b-pyramid): a block without list-0 motion gives its
  // list-1 motion (8.4.1.2.1); a P anchor predicts from list 0 only
  const bool col_l1 = a.rt && a.rt[slot].col_l1;
  const bool intra = h264::mbk_is_intra(c.kind);
  int v[2][4][2];
  int rq[4];
  int s[2][2] = {{0, 0}, {0, 0}};
  int cz = 0, navail = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    // direct_8x8_inference: the corner 4x4 block of co-located quadrant q, i.e. its vector;
    // a P anchor predicts from list 0 only
    const int cl = (col_l1 && c.ref[0][q] < 0) ? 1 : 0;
    const bool none = intra || c.ref[cl][q] < 0;
    const int cx = none ? 0 : c.mv[cl][q][0];
    const int cy = none ? 0 : c.mv[cl][q][1];
    // refIdxCol, then MapColToList0: the index in this picture's list 0 of the picture the
    // co-located block referred to (an intra co-located block: refIdxL0 0, zero vectors)
    const int rc = none ? 0 : min(static_cast<int>(c.ref[cl][q]), kMaxRefs - 1);
    const int rm = none ? 0 : col_to_list0(a.cmap, slot, cl, rc);
    const bool una = rm < 0;  // not in list 0: no direct prediction for this quadrant
    const int r = una ? 0 : rm;
    rq[q] = rm;
    navail += una ? 0 : 1;
    if (!none && c.ref[cl][q] == 0 && abs(cx) <= 1 && abs(cy) <= 1) cz |= 1 << q;  // (on refIdxCol)
    int l0x, l0y;
    const int dcp = a.rt ? a.rt[slot].dcopy[r] : a.direct_copy[r], dsf = a.rt ? a.rt[slot].dsf[r] : a.dsf[r];
    if (dcp) {
      l0x = cx;
      l0y = cy;
    } else {
      l0x = (dsf * cx + 128) >> 8;
      l0y = (dsf * cy + 128) >> 8;
    }
    v[0][q][0] = una ? 0 : l0x;
    v[0][q][1] = una ? 0 : l0y;
    v[1][q][0] = (una || dcp) ? 0 : l0x - cx;
    v[1][q][1] = (una || dcp) ? 0 : l0y - cy;
#pragma unroll
    for (int l = 0; l < 2; ++l) {
      s[l][0] += v[l][q][0];
      s[l][1] += v[l][q][1];
    }
  }
  int16_t* d = a.dmv + o * 16;
#pragma unroll
  for (int l = 0; l < 2; ++l)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      d[l * 8 + q * 2] = static_cast<int16_t>(v[l][q][0]);
      d[l * 8 + q * 2 + 1] = static_cast<int16_t>(v[l][q][1]);
    }
  if (a.dref) {
    const uint32_t rw = (static_cast<uint32_t>(rq[0]) & 255u) | ((static_cast<uint32_t>(rq[1]) & 255u) << 8) |
                        ((static_cast<uint32_t>(rq[2]) & 255u) << 16) | (static_cast<uint32_t>(rq[3]) << 24);
    *reinterpret_cast<uint32_t*>(a.dref + o * 4) = rw;
  }
  if (a.czero) a.czero[o] = static_cast<uint8_t>(cz);
  a.pm0[o * 2] = static_cast<int16_t>(mean_half_up(s[0][0], navail));
  a.pm0[o * 2 + 1] = static_cast<int16_t>(mean_half_up(s[0][1], navail));
  a.pm1[o * 2] = static_cast<int16_t>(mean_half_up(s[1][0], navail));
  a.pm1[o * 2 + 1] = static_cast<int16_t>(mean_half_up(s[1][1], navail));
}

struct BDecideArgs {
  Geom g;
  const uint8_t* src_y;            // [B, H, W]
  const uint8_t *ref0, *ref1;      // anchors' luma (RefPicList0[0], RefPicList1[0])
  const uint8_t *hp0, *hp1;        // their b / h / j planes [B, 3, H + 8, W + 8]
  const int16_t *mv0, *mv1;        // [B, nmb, 2] ME vectors per list
  const int *cost0, *cost1;        // ME costs (SATD + lambda * mv bits)
  const uint8_t *pred0, *pred1;    // ME luma predictions [B, nmb, 256]
  const int16_t *pm0, *pm1;        // ME predictors
  const int16_t* dmv;              // [B, nmb, 2, 4, 2]
  const int* qp;                   // [B]
  const int8_t* aq;                // [B, nmb] (nullable)
  MbHeader* hdr;                   // out: kind / ref / mv
  uint8_t* pred_out;               // out: [B, nmb, 256]
  int* cost_out;                   // out: [B, nmb] the winner's cost (vs the intra estimate)
  // implicit bi-prediction weight of list 1 (32: plain average) per refIdxL0 (the list-1
  // picture is always RefPicList1[0]); the ME candidates use entry 0
  int w1[kMaxRefs];
  // direct prediction from RefPicList0[r] (r = dref per quadrant, nullable: all 0):
  // luma / half-sample planes of every list-0 picture (entry 0 = ref0 / hp0)
  const int8_t* dref;
  const uint8_t* ref0k[kMaxRefs];
  const uint8_t* hp0k[kMaxRefs];
  // direct_only: the pre-pass before the two ME searches -- only the direct candidate's cost
  // (SATD + lambda) goes to cost_out; MBs whose direct cost is already low skip the searches
  // (me.hip gate) and their list costs come back as kNoCost
  int direct_only;
  // the pre-pass ran (direct_only = 1 before the searches): pred_out / cost_out hold every MB's
  // direct prediction and cost -- unsearched MBs keep them, the others skip the direct MC
  int have_direct;
  int bparts;  // x264 --partitions b8x8: per-quadrant candidates (B_16x8 / B_8x16 / B_8x8)
  // spatial direct 1 (wavefront decision): searched MBs keep their best explicit candidate (no
  // direct MB / quadrant); b_spatial_decide weighs it against the exact spatial direct motion
  // in decoding order.  2 (fast): direct is priced in parallel with the pre-pass's estimate of
  // the spatial motion (needs the pre-pass); b_spatial_exact / b_spatial_fixup make it exact
  int spatial;
  int dbias;  // direct preferred by dbias * lambda in the 16x16 choice (cost_out stays unbiased)
  const uint8_t* czero;  // spatial == 2: colZeroFlag bits per MB (b_direct_mv)
  // routed (route.h): ref0 / ref1 / hp0 / hp1 / ref0k / hp0k are pool bases, the roles come from
  // each B slot's SlotRoute (list-0 entries, list-1 entry, implicit weights)
  const SlotRoute* rt;
  int nbuf;
};

// x264 --partitions b8x8: every quadrant picks its own candidate among the MB's motion
// (direct quadrant, L0, L1, bi with the two searched vectors): B_16x8 / B_8x16 when the
// halves agree and no quadrant is direct, else B_8x8 (direct quadrants as B_Direct_8x8).
// Bits: sub_mb_type (direct 1, L0 / L1 3, bi 5 bins), one full mvd per list in use, 1 bin
// per later partition repeating it, and the B_8x8 mb_type (~6 bins) / 16x8 pair codes.
// qsat: [candidate 0 direct, 1 bi, 2 L0, 3 L1][quadrant]; best / qm / kind: the 16x16 choice,
// replaced when the split wins.  no_direct: bit q = quadrant q may not be B_Direct_8x8 (all
// four: spatial direct decided later; some: no temporal direct prediction there, dref -1)
__device__ __forceinline__ void b_part_choice(const int (&qsat)[4][4], int lambda, uint32_t no_direct, int mvb0, int mvb1,
                                              int& best, int (&qm)[4], int& kind) {
  int sum = 0, used0 = 0, used1 = 0, pm[4];
#pragma unroll
  for (int qq = 0; qq < 4; ++qq) {
    const int cd = ((no_direct >> qq) & 1u) ? kNoCost : qsat[0][qq] + lambda * 1, cb = qsat[1][qq] + lambda * 7;
    const int c0q = qsat[2][qq] + lambda * 4, c1q = qsat[3][qq] + lambda * 4;
    int m = 0, bc = cd;
    if (cb < bc) { m = 1; bc = cb; }
    if (c0q < bc) { m = 2; bc = c0q; }
    if (c1q < bc) { m = 3; bc = c1q; }
    pm[qq] = m;
    sum += bc;
    used0 |= m == 1 || m == 2;
    used1 |= m == 1 || m == 3;
  }
  const bool anyd = pm[0] == 0 || pm[1] == 0 || pm[2] == 0 || pm[3] == 0;
  const bool h2 = pm[0] == pm[1] && pm[2] == pm[3], v2 = pm[0] == pm[2] && pm[1] == pm[3];
  const bool uni = h2 && v2;
  if (!uni) {
    const int shape_bits = (!anyd && (h2 || v2)) ? 7 : 6;
    const int c_part = sum + lambda * (shape_bits + (used0 ? mvb0 : 0) + (used1 ? mvb1 : 0));
    if (c_part < best) {
      best = c_part;
#pragma unroll
      for (int qq = 0; qq < 4; ++qq) qm[qq] = pm[qq];
      kind = (!anyd && h2) ? h264::MBK_B16x8 : ((!anyd && v2) ? h264::MBK_B8x16 : h264::MBK_B8x8);
    }
  }
}

// The main pass of b_decide after the direct-only pre-pass, for a searched MB (the caller
// returned for gated ones): the same candidates, costs and decisions as the general path,
// computed with one candidate's rows live at a time.
template <class W1>
__device__ __forceinline__ void b_decide_main(const BDecideArgs& a, const MbRow& r, const uint32_t (&src)[4], int q,
                                              uint8_t* pout, MbHeader* hrec, uint32_t drw, const int16_t* dm,
                                              const uint8_t* G0, const uint8_t* G1, const uint8_t* H0,
                                              const uint8_t* H1, W1 w1of) {
  const Geom& g = a.g;
  const int W = g.W, H = g.H;
  const size_t o = r.o;
  const int lane = r.lane, wrow = r.row, X = r.X, Y = r.Y;
  const int m0x = a.mv0[o * 2], m0y = a.mv0[o * 2 + 1];
  const int m1x = a.mv1[o * 2], m1y = a.mv1[o * 2 + 1];
  const uint8_t* pr0 = a.pred0 + o * 256 + r.by4 * 16 + r.bx4;
  const uint8_t* pr1 = a.pred1 + o * 256 + r.by4 * 16 + r.bx4;
  __shared__ int s_pair[kMbsPerWave][4][16];
  uint32_t pb[4];
  {
    uint32_t t[4];
#pragma unroll
    for (int y = 0; y < 4; ++y) t[y] = *reinterpret_cast<const uint32_t*>(pout + 16 * y);
    const int s0 = satd4x4_u8(src, t);
    s_pair[wrow][0][lane] = s0 + dpp<kDppQuadXor1>(s0);
#pragma unroll
    for (int y = 0; y < 4; ++y) t[y] = *reinterpret_cast<const uint32_t*>(pr0 + 16 * y);
    const int s2 = satd4x4_u8(src, t);
    s_pair[wrow][2][lane] = s2 + dpp<kDppQuadXor1>(s2);
#pragma unroll
    for (int y = 0; y < 4; ++y) t[y] = *reinterpret_cast<const uint32_t*>(pr1 + 16 * y);
    const int s3 = satd4x4_u8(src, t);
    s_pair[wrow][3][lane] = s3 + dpp<kDppQuadXor1>(s3);
  }
  const int w10 = w1of(0);
  {
    uint32_t p1[4];
    mc4x4(G0, H0, W, H, X, Y, m0x, m0y, pb);
    mc4x4(G1, H1, W, H, X, Y, m1x, m1y, p1);
#pragma unroll
    for (int y = 0; y < 4; ++y) pb[y] = wavg4b(pb[y], p1[y], w10);
  }
  {
    const int s1 = satd4x4_u8(src, pb);
    s_pair[wrow][1][lane] = s1 + dpp<kDppQuadXor1>(s1);
  }
  wave_sync();
  int qsat[4][4];  // [candidate][quadrant]
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int qq = 0; qq < 4; ++qq) {
      const int l0 = (qq >> 1) * 8 + (qq & 1) * 2;
      qsat[c][qq] = s_pair[wrow][c][l0] + s_pair[wrow][c][l0 + 4];
    }
  const int satd_direct = qsat[0][0] + qsat[0][1] + qsat[0][2] + qsat[0][3];
  const int satd_bi = qsat[1][0] + qsat[1][1] + qsat[1][2] + qsat[1][3];
  const int lambda = mb_lambda(a.qp, a.aq, r.slot, o);
  const int c_direct = satd_direct + lambda * 1;
  const int c_l0 = a.cost0[o] + lambda * 3;
  const int c_l1 = a.cost1[o] + lambda * 3;
  const int mvb0 = mvbits_se(m0x - a.pm0[o * 2]) + mvbits_se(m0y - a.pm0[o * 2 + 1]);
  const int mvb1 = mvbits_se(m1x - a.pm1[o * 2]) + mvbits_se(m1y - a.pm1[o * 2 + 1]);
  const int c_bi = satd_bi + lambda * (6 + mvb0 + mvb1);
  // quadrants that may not be direct: all with spatial == 1 (searched), else those without a
  // temporal direct prediction -- B_Direct_16x16 / B_Skip needs all four
  const uint32_t no_direct = a.spatial == 1 ? 15u : (a.spatial == 2 ? 0u : dref_unavail(drw));
  const int dbias = no_direct ? 0 : a.dbias * lambda;
  int mode = 0, best = no_direct ? kNoCost : c_direct - dbias;  // 0 direct, 1 L0, 2 L1, 3 Bi
  if (c_l0 < best) { mode = 1; best = c_l0; }
  if (c_l1 < best) { mode = 2; best = c_l1; }
  if (c_bi < best) { mode = 3; best = c_bi; }
  int qm[4] = {mode == 0 ? 0 : (mode == 3 ? 1 : mode + 1), 0, 0, 0};  // per quadrant: 0 D, 1 Bi, 2 L0, 3 L1
  qm[1] = qm[2] = qm[3] = qm[0];
  int kind = mode == 0 ? h264::MBK_BDIRECT : h264::MBK_B16x16;
  if (a.bparts) b_part_choice(qsat, lambda, no_direct, mvb0, mvb1, best, qm, kind);
  // the winner's prediction of this lane's block (direct: pred_out holds it already)
  const int lm = qm[q];
  if (lm != 0) {
    const uint8_t* srcp = lm == 2 ? pr0 : pr1;
#pragma unroll
    for (int y = 0; y < 4; ++y)
      *reinterpret_cast<uint32_t*>(pout + 16 * y) = lm == 1 ? pb[y] : *reinterpret_cast<const uint32_t*>(srcp + 16 * y);
  }
  if (lane == 0) {
    // direct motion per quadrant: temporal from b_direct_mv's vectors (dref: refIdxL0), the
    // fast spatial path's estimate from the record the pre-pass wrote
    uint32_t dw[2][4];
    uint32_t dr8[2];
    if (a.spatial == 2) {
      const uint2 hr = *reinterpret_cast<const uint2*>(&hrec->ref[0][0]);
      const uint4 hm0 = *reinterpret_cast<const uint4*>(&hrec->mv[0][0][0]);
      const uint4 hm1 = *reinterpret_cast<const uint4*>(&hrec->mv[1][0][0]);
      dr8[0] = hr.x;
      dr8[1] = hr.y;
      dw[0][0] = hm0.x; dw[0][1] = hm0.y; dw[0][2] = hm0.z; dw[0][3] = hm0.w;
      dw[1][0] = hm1.x; dw[1][1] = hm1.y; dw[1][2] = hm1.z; dw[1][3] = hm1.w;
    } else {
      const uint4 d0 = reinterpret_cast<const uint4*>(dm)[0], d1 = reinterpret_cast<const uint4*>(dm)[1];
      dr8[0] = drw;
      dr8[1] = 0;
      dw[0][0] = d0.x; dw[0][1] = d0.y; dw[0][2] = d0.z; dw[0][3] = d0.w;
      dw[1][0] = d1.x; dw[1][1] = d1.y; dw[1][2] = d1.z; dw[1][3] = d1.w;
    }
    MbHeader* h = hrec;
    h->kind = static_cast<uint8_t>(kind);
    int sd_ = 0;
    uint32_t w[2][4];
    uint32_t rfw[2] = {0, 0};
    const uint32_t v0 = (static_cast<uint32_t>(m0x) & 0xFFFFu) | (static_cast<uint32_t>(m0y) << 16);
    const uint32_t v1 = (static_cast<uint32_t>(m1x) & 0xFFFFu) | (static_cast<uint32_t>(m1y) << 16);
#pragma unroll
    for (int qq = 0; qq < 4; ++qq) {
      const int m = qm[qq];
      uint32_t r0, r1;
      if (m == 0) {  // direct (the whole MB or a B_Direct_8x8 quadrant)
        w[0][qq] = dw[0][qq];
        w[1][qq] = dw[1][qq];
        r0 = (dr8[0] >> (8 * qq)) & 255u;
        r1 = (dr8[1] >> (8 * qq)) & 255u;
        sd_ |= 1 << qq;
      } else {
        const bool u0 = m != 3, u1 = m != 2;
        w[0][qq] = u0 ? v0 : 0u;
        w[1][qq] = u1 ? v1 : 0u;
        r0 = u0 ? 0u : 255u;
        r1 = u1 ? 0u : 255u;
      }
      rfw[0] |= r0 << (8 * qq);
      rfw[1] |= r1 << (8 * qq);
    }
    h->sub_direct = static_cast<uint8_t>(kind == h264::MBK_B8x8 ? sd_ : 0);
    *reinterpret_cast<uint2*>(&h->ref[0][0]) = make_uint2(rfw[0], rfw[1]);
    uint4* mvp = reinterpret_cast<uint4*>(&h->mv[0][0][0]);  // 16-byte aligned
    mvp[0] = make_uint4(w[0][0], w[0][1], w[0][2], w[0][3]);
    mvp[1] = make_uint4(w[1][0], w[1][1], w[1][2], w[1][3]);
    a.cost_out[o] = best + (kind == h264::MBK_BDIRECT ? dbias : 0);
  }
}

// K: 0 general (any flags), 1 the direct-only pre-pass, 2 the main pass after the pre-pass
// (have_direct: the default configuration).  K = 2 keeps only the bi-predicted candidate in
// registers -- direct's prediction is already in pred_out, the list predictions are re-read
// from the ME's buffers for the winner, and the direct motion is re-read for the record -- so
// the kernel fits 64 VGPRs (8 waves per SIMD instead of 4 for this chain of dependent loads).
template <int K>
__global__ __launch_bounds__(64) void b_decide(BDecideArgs a) {
  const Geom& g = a.g;
  const MbRow r = mb_row(g, a.rt, SK_B);
  if (!r.live) return;
  const int nmb = g.nmb(), slot = r.slot, mb = r.mb, lane = r.lane, wrow = r.row;
  const size_t o = r.o;
  const int mx = r.mx, my = r.my, bx4 = r.bx4, by4 = r.by4, X = r.X, Y = r.Y;
  const int W = g.W, H = g.H;
  const int q = (by4 >> 3) * 2 + (bx4 >> 3);  // 8x8 quadrant of this lane's block
  const size_t hps = hp_plane_bytes(W, H);
  const size_t s0 = route_index(a.rt, a.nbuf, slot, RO_L0), s1 = route_index(a.rt, a.nbuf, slot, RO_L1);
  const uint8_t *G0 = a.ref0 + s0 * g.ysize(), *G1 = a.ref1 + s1 * g.ysize(), *H0 = a.hp0 + s0 * hps,
                *H1 = a.hp1 + s1 * hps;
  const int16_t* w1t = a.rt ? a.rt[slot].w1 : nullptr;
  auto w1of = [&](int rr) { return w1t ? static_cast<int>(w1t[rr & 3]) : a.w1[rr & 3]; };
  const int16_t* dm = a.dmv + o * 16;
  const bool donly = (K == 1 || K == 3) ? true : (K == 2 ? false : static_cast<bool>(a.direct_only));
  const bool have_direct = K == 2 ? true : ((K == 1 || K == 3) ? false : static_cast<bool>(a.have_direct));
  const bool sfast = a.spatial == 2;
  MbHeader* hrec = a.hdr + o;
  uint32_t drw = 0;  // refIdxL0 of the four temporal-direct quadrants (bytes; -1: no direct prediction)
  if (a.dref) drw = *reinterpret_cast<const uint32_t*>(a.dref + o * 4);
  // quadrants without a temporal direct prediction (b-pyramid: the co-located reference is not
  // in list 0).  Such an MB is never gated (the pre-passes leave kNoCost, so both searches run)
  // and is direct only in its other quadrants (B_Direct_8x8)
  const uint32_t una = sfast ? 0u : dref_unavail(drw);
  // gated MB (the search left kNoCost): B_Direct_16x16 with the pre-pass's prediction and cost
  auto direct_record = [&]() {
    if (lane == 0) {
      hrec->kind = h264::MBK_BDIRECT;
      hrec->sub_direct = 0;
      if (!sfast) {  // (spatial: the estimate is in the record already)
        *reinterpret_cast<uint2*>(&hrec->ref[0][0]) = make_uint2(drw, 0u);
        uint4* mvp = reinterpret_cast<uint4*>(&hrec->mv[0][0][0]);
        const uint4* dv = reinterpret_cast<const uint4*>(dm);  // [list][quadrant][xy] int16
        mvp[0] = dv[0];
        mvp[1] = dv[1];
      }
    }
  };
  if constexpr (K == 2) {
    // nearly every MB of the main pass is gated: find that out before the vectors and the
    // source rows are loaded for nothing
    if (!(a.cost0[o] < kNoCost && a.cost1[o] < kNoCost)) {
      direct_record();
      return;
    }
  }
  const int m0x = donly ? 0 : a.mv0[o * 2], m0y = donly ? 0 : a.mv0[o * 2 + 1];
  const int m1x = donly ? 0 : a.mv1[o * 2], m1y = donly ? 0 : a.mv1[o * 2 + 1];
  uint32_t src[4];
  load_src4(g, r, a.src_y, src);
  // The direct candidate per quadrant and list: refIdx (-1: list unused) and vector.
  //   temporal: the co-located block's scaled motion (b_direct_mv), list 1 from RefPicList1[0];
  //   spatial (fast, spatial == 2): the pre-pass estimates 8.4.1.2.2 from the neighbours'
  //     temporal-direct motion standing in for their final motion (colZeroFlag exact) and
  //     leaves it in the record; the main pass prices it; b_spatial_exact later derives the
  //     exact motion in decoding order and b_spatial_fixup re-predicts where it differs.
  int dref_[2][4], dvx[2][4], dvy[2][4];
  if (K == 2 || K == 3) {
    // the lean passes: nothing here (each lane reads its own quadrant's direct motion, lane 0
    // re-reads it for the record)
  } else if (!sfast) {
#pragma unroll
    for (int qq = 0; qq < 4; ++qq) {
      dref_[0][qq] = static_cast<int8_t>((drw >> (8 * qq)) & 255u);  // (-1: priced from list 1 alone, never chosen)
      dref_[1][qq] = 0;
      dvx[0][qq] = dm[qq * 2];
      dvy[0][qq] = dm[qq * 2 + 1];
      dvx[1][qq] = dm[8 + qq * 2];
      dvy[1][qq] = dm[8 + qq * 2 + 1];
    }
  } else if (donly) {
    auto tmot = [&](int n, int l, int qq, bool avail) -> NbMv16 {
      NbMv16 m{avail, -1, {0, 0}};
      if (!avail) return m;
      const size_t on = static_cast<size_t>(slot) * nmb + n;
      m.ref = l == 0 ? (a.dref ? static_cast<int>(a.dref[on * 4 + qq]) : 0) : 0;
      m.mv[0] = a.dmv[on * 16 + l * 8 + qq * 2];
      m.mv[1] = a.dmv[on * 16 + l * 8 + qq * 2 + 1];
      return m;
    };
    const bool aA = mx > 0, aB = my > 0, aC = my > 0 && mx + 1 < g.wmb, aD = mx > 0 && my > 0;
    int sref[2], spx[2], spy[2];
#pragma unroll
    for (int l = 0; l < 2; ++l) {
      const NbMv16 A = tmot(mb - 1, l, 1, aA);
      const NbMv16 Bn = tmot(mb - g.wmb, l, 2, aB);
      const NbMv16 C = aC ? tmot(mb - g.wmb + 1, l, 2, true) : tmot(mb - g.wmb - 1, l, 3, aD);
      spatial_pmv(A, Bn, C, sref[l], spx[l], spy[l]);
    }
    const bool zero = sref[0] < 0 && sref[1] < 0;
    const int cz = a.czero ? a.czero[o] : 0;
#pragma unroll
    for (int qq = 0; qq < 4; ++qq)
#pragma unroll
      for (int l = 0; l < 2; ++l) {
        int rf = sref[l], vx = spx[l], vy = spy[l];
        if (zero) {
          rf = 0;
          vx = vy = 0;
        } else if (rf < 0 || (rf == 0 && ((cz >> qq) & 1))) {
          vx = vy = 0;
        }
        dref_[l][qq] = rf;
        dvx[l][qq] = vx;
        dvy[l][qq] = vy;
      }
  } else {  // the pre-pass's estimate, left in the record
    const uint2 hr = *reinterpret_cast<const uint2*>(&hrec->ref[0][0]);
    const uint4 hm0 = *reinterpret_cast<const uint4*>(&hrec->mv[0][0][0]);
    const uint4 hm1 = *reinterpret_cast<const uint4*>(&hrec->mv[1][0][0]);
    const uint32_t w0[4] = {hm0.x, hm0.y, hm0.z, hm0.w}, w1_[4] = {hm1.x, hm1.y, hm1.z, hm1.w};
#pragma unroll
    for (int qq = 0; qq < 4; ++qq) {
      dref_[0][qq] = static_cast<int8_t>((hr.x >> (8 * qq)) & 255u);
      dref_[1][qq] = static_cast<int8_t>((hr.y >> (8 * qq)) & 255u);
      dvx[0][qq] = static_cast<int16_t>(w0[qq] & 0xFFFFu);
      dvy[0][qq] = static_cast<int16_t>(w0[qq] >> 16);
      dvx[1][qq] = static_cast<int16_t>(w1_[qq] & 0xFFFFu);
      dvy[1][qq] = static_cast<int16_t>(w1_[qq] >> 16);
    }
  }
  const bool searched = K == 2 ? true : (!donly && a.cost0[o] < kNoCost && a.cost1[o] < kNoCost);
  uint8_t* pout = a.pred_out + o * 256 + by4 * 16 + bx4;   // row y at pout + 16 * y
  if (!donly && !searched && have_direct) {
    direct_record();
    return;
  }
  if constexpr (K == 2) {
    b_decide_main(a, r, src, q, pout, hrec, drw, dm, G0, G1, H0, H1, w1of);
    return;
  }
  if constexpr (K == 3) {
    // the temporal-direct pre-pass: this lane's quadrant only
    // (a quadrant without a direct prediction: entry 0 with its zero vectors, never chosen)
    const int dr = max(static_cast<int>(static_cast<int8_t>((drw >> (8 * q)) & 255u)), 0) & 3;
    const int dvx0 = dm[q * 2], dvy0 = dm[q * 2 + 1], dvx1 = dm[8 + q * 2], dvy1 = dm[8 + q * 2 + 1];
    const size_t sd = route_index(a.rt, a.nbuf, slot, RO_L0 + (dr & 3));
    const uint8_t *GD = dr ? a.ref0k[dr] + (a.rt ? sd : slot) * g.ysize() : G0,
                  *HD = dr ? a.hp0k[dr] + (a.rt ? sd : slot) * hps : H0;
    const int w1 = w1of(dr);
    uint32_t pd[4], p1[4];
    mc4x4(GD, HD, W, H, X, Y, dvx0, dvy0, pd);
    mc4x4(G1, H1, W, H, X, Y, dvx1, dvy1, p1);
#pragma unroll
    for (int y = 0; y < 4; ++y) {
      pd[y] = wavg4b(pd[y], p1[y], w1);
      *reinterpret_cast<uint32_t*>(pout + 16 * y) = pd[y];
    }
    const int sat = row_satd(src, pd);
    if (lane == 0) a.cost_out[o] = (drw & 0x80808080u) ? kNoCost : sat + mb_lambda(a.qp, a.aq, slot, o) * 1;
    return;
  }
  const int dr = dref_[0][q] < 0 ? 0 : dref_[0][q];  // this lane's quadrant
  const bool du0 = dref_[0][q] >= 0, du1 = dref_[1][q] >= 0;
  const size_t sd = route_index(a.rt, a.nbuf, slot, RO_L0 + (dr & 3));
  const uint8_t *GD = dr ? a.ref0k[dr] + (a.rt ? sd : slot) * g.ysize() : G0,
                *HD = dr ? a.hp0k[dr] + (a.rt ? sd : slot) * hps : H0;
  uint32_t pd[4], pb[4], p0w[4], p1w[4];
#pragma unroll
  for (int y = 0; y < 4; ++y) {
    if (!donly && have_direct) {
      pd[y] = *reinterpret_cast<const uint32_t*>(pout + 16 * y);
    } else {
      const uint32_t pl0 = du0 ? mc4(GD, HD, W, H, X, Y + y, dvx[0][q], dvy[0][q]) : 0u;
      const uint32_t pl1 = du1 ? mc4(G1, H1, W, H, X, Y + y, dvx[1][q], dvy[1][q]) : 0u;
      pd[y] = (du0 && du1) ? wavg4b(pl0, pl1, w1of(dr)) : (du0 ? pl0 : pl1);
    }
    if (donly) *reinterpret_cast<uint32_t*>(pout + 16 * y) = pd[y];
    pb[y] = donly ? pd[y]
                  : wavg4b(mc4(G0, H0, W, H, X, Y + y, m0x, m0y), mc4(G1, H1, W, H, X, Y + y, m1x, m1y), w1of(0));
    // candidates: 0 direct, 1 bi (the two ME vectors), 2 L0, 3 L1 (the ME predictions; not
    // needed by the direct-only pre-pass or for MBs the gate left unsearched)
    p0w[y] = searched ? *reinterpret_cast<const uint32_t*>(a.pred0 + o * 256 + (by4 + y) * 16 + bx4) : pd[y];
    p1w[y] = searched ? *reinterpret_cast<const uint32_t*>(a.pred1 + o * 256 + (by4 + y) * 16 + bx4) : pd[y];
  }
  // per 8x8 quadrant and candidate: horizontal block pairs by DPP, then the two pair rows of
  // each quadrant from LDS (pair sums at lanes 8 * qy + 4 * {0, 1} + 2 * qx)
  __shared__ int s_pair[kMbsPerWave][4][16];
  const int ncand = donly ? 1 : 4;  // the pre-pass prices direct only
  {
    const int s0 = satd4x4_u8(src, pd);
    s_pair[wrow][0][lane] = s0 + dpp<kDppQuadXor1>(s0);
    if (!donly) {
      const int s1 = satd4x4_u8(src, pb), s2 = satd4x4_u8(src, p0w), s3 = satd4x4_u8(src, p1w);
      s_pair[wrow][1][lane] = s1 + dpp<kDppQuadXor1>(s1);
      s_pair[wrow][2][lane] = s2 + dpp<kDppQuadXor1>(s2);
      s_pair[wrow][3][lane] = s3 + dpp<kDppQuadXor1>(s3);
    }
  }
  wave_sync();
  int qsat[4][4];  // [candidate][quadrant] (the pre-pass: candidate 0 only)
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int qq = 0; qq < 4; ++qq) {
      const int l0 = (qq >> 1) * 8 + (qq & 1) * 2;
      qsat[c][qq] = c < ncand ? s_pair[wrow][c][l0] + s_pair[wrow][c][l0 + 4] : 0;
    }
  const int satd_direct = qsat[0][0] + qsat[0][1] + qsat[0][2] + qsat[0][3];
  const int satd_bi = qsat[1][0] + qsat[1][1] + qsat[1][2] + qsat[1][3];
  const int lambda = mb_lambda(a.qp, a.aq, slot, o);
  // mb_type / motion bits (CABAC-ish): direct "0"; L0 / L1 "10x"; Bi "110000" + two mvds
  const int c_direct = satd_direct + lambda * 1;
  if (donly) {
    if (lane == 0) {
      if (a.spatial == 1) {
        // spatial direct decided in the wavefront (b_spatial_decide): only MBs whose co-located
        // motion is static in every quadrant (temporal direct vectors within +-1, refIdxL0 0)
        // may skip the searches -- there spatial direct predicts zero motion too (colZeroFlag)
        bool stat = drw == 0;  // (so every quadrant has its direct prediction)
#pragma unroll
        for (int k = 0; k < 16; ++k) stat = stat && dm[k] >= -1 && dm[k] <= 1;
        a.cost_out[o] = stat ? c_direct : kNoCost;
      } else {
        a.cost_out[o] = una ? kNoCost : c_direct;
      }
      if (sfast) {  // the estimate, for the main pass (and for gated MBs: their motion)
#pragma unroll
        for (int l = 0; l < 2; ++l)
#pragma unroll
          for (int qq = 0; qq < 4; ++qq) {
            hrec->ref[l][qq] = static_cast<int8_t>(dref_[l][qq]);
            hrec->mv[l][qq][0] = static_cast<int16_t>(dvx[l][qq]);
            hrec->mv[l][qq][1] = static_cast<int16_t>(dvy[l][qq]);
          }
      }
    }
    return;
  }
  const int c_l0 = a.cost0[o] + lambda * 3;
  const int c_l1 = a.cost1[o] + lambda * 3;
  const int mvb0 = mvbits_se(m0x - a.pm0[o * 2]) + mvbits_se(m0y - a.pm0[o * 2 + 1]);
  const int mvb1 = mvbits_se(m1x - a.pm1[o * 2]) + mvbits_se(m1y - a.pm1[o * 2 + 1]);
  const int c_bi = satd_bi + lambda * (6 + mvb0 + mvb1);
  const uint32_t no_direct = (a.spatial == 1 && searched) ? 15u : una;
  const int dbias = no_direct ? 0 : a.dbias * lambda;
  int mode = 0, best = no_direct ? kNoCost : c_direct - dbias;  // 0 direct, 1 L0, 2 L1, 3 Bi
  if (c_l0 < best) { mode = 1; best = c_l0; }
  if (c_l1 < best) { mode = 2; best = c_l1; }
  if (searched && c_bi < best) { mode = 3; best = c_bi; }
  int qm[4] = {mode == 0 ? 0 : (mode == 3 ? 1 : mode + 1), 0, 0, 0};  // per quadrant: 0 D, 1 Bi, 2 L0, 3 L1
  qm[1] = qm[2] = qm[3] = qm[0];
  int kind = mode == 0 ? h264::MBK_BDIRECT : h264::MBK_B16x16;
  if (a.bparts && searched) b_part_choice(qsat, lambda, no_direct, mvb0, mvb1, best, qm, kind);
  const int lm = qm[q];  // this lane's quadrant
#pragma unroll
  for (int y = 0; y < 4; ++y)
    *reinterpret_cast<uint32_t*>(pout + 16 * y) = lm == 0 ? pd[y] : (lm == 1 ? pb[y] : (lm == 2 ? p0w[y] : p1w[y]));
  if (lane == 0) {
    MbHeader* h = hrec;
    h->kind = static_cast<uint8_t>(kind);
    int sd_ = 0;
    uint32_t w[2][4];
    int8_t rf[2][4];
#pragma unroll
    for (int qq = 0; qq < 4; ++qq) {
      const int m = qm[qq];
      int x0 = 0, y0 = 0, x1 = 0, y1 = 0;
      if (m == 0) {  // direct (the whole MB or a B_Direct_8x8 quadrant)
        x0 = dvx[0][qq]; y0 = dvy[0][qq]; x1 = dvx[1][qq]; y1 = dvy[1][qq];
        rf[0][qq] = static_cast<int8_t>(dref_[0][qq]);
        rf[1][qq] = static_cast<int8_t>(dref_[1][qq]);
        sd_ |= 1 << qq;
      } else {
        const bool u0 = m != 3, u1 = m != 2;
        if (u0) { x0 = m0x; y0 = m0y; }
        if (u1) { x1 = m1x; y1 = m1y; }
        rf[0][qq] = u0 ? 0 : -1;
        rf[1][qq] = u1 ? 0 : -1;
      }
      w[0][qq] = (static_cast<uint32_t>(x0) & 0xFFFFu) | (static_cast<uint32_t>(y0) << 16);
      w[1][qq] = (static_cast<uint32_t>(x1) & 0xFFFFu) | (static_cast<uint32_t>(y1) << 16);
    }
    h->sub_direct = static_cast<uint8_t>(kind == h264::MBK_B8x8 ? sd_ : 0);
#pragma unroll
    for (int l = 0; l < 2; ++l)
#pragma unroll
      for (int qq = 0; qq < 4; ++qq) h->ref[l][qq] = rf[l][qq];
    uint4* mvp = reinterpret_cast<uint4*>(&h->mv[0][0][0]);  // 16-byte aligned
    mvp[0] = make_uint4(w[0][0], w[0][1], w[0][2], w[0][3]);
    mvp[1] = make_uint4(w[1][0], w[1][1], w[1][2], w[1][3]);
    a.cost_out[o] = best + (kind == h264::MBK_BDIRECT ? dbias : 0);
  }
}

// ---------------------------------------------------------------- spatial direct (x264 --direct spatial)
// 8.4.1.2.2: the direct motion of a macroblock follows its neighbours A (left), B (above) and
// C (above-right, else D above-left) in the *current* picture: refIdxLX = MinPositive over
// them, the 16x16 motion-vector predictor of that reference, zeroed per 8x8 quadrant where the
// co-located block of RefPicList1[0] is static (colZeroFlag).  Neighbours' final motion exists
// only in decoding order, so the direct-vs-explicit decision runs in an MB wavefront (one wave
// per MB row, the row above two MBs ahead): b_decide (spatial = 1) leaves each searched
// MB's best explicit candidate (B_L0/L1/Bi 16x16, 16x8, 8x16, B_8x8 without direct quadrants)
// with its cost, and b_spatial_decide derives the exact direct motion from the final
// neighbours, prices it (SATD of its bi-prediction + lambda) and takes it when not dearer.
// MBs the gate left unsearched (b_decide wrote them B_Direct) are always direct.
struct BSpatialArgs {
  Geom g;
  MbHeader* hdr;         // [B, nmb] current picture (in / out)
  const MbHeader* col;   // [B, nmb] RefPicList1[0]'s records
  int* err;
  // encode_inter turns an MB intra when intra_cost < cost (the final decision): such MBs are
  // intra neighbours for the derivation
  const int* intra_cost;
  int* cost;             // in: the explicit candidate's cost (unsearched: the temporal estimate); out: final
  const uint8_t* src_y;
  const uint8_t *ref1, *hp1;
  const uint8_t* ref0k[kMaxRefs];
  const uint8_t* hp0k[kMaxRefs];
  int w1[kMaxRefs];
  uint8_t* pred_out;     // [B, nmb, 256] rewritten for MBs that become direct
  const int* qp;
  const int8_t* aq;
  int bias;              // direct taken when cost_d <= cost_e + bias * lambda
  const SlotRoute* rt;   // routed (route.h): pools for col / ref1 / hp1 / ref0k / hp0k, B slots only
  int nbuf;
};


constexpr int kSpatialWaves = 16;  // 16 row chains per slot: the chain (wmb + 2 hmb MBs) bounds it, not the MB count

// packed motion of one quadrant and list: ref (low 8 bits, signed) | mvx << 8 (12 bits) |
// mvy << 20 -- the encoder's vectors stay within +-2048 quarter samples
__device__ __forceinline__ int pk_ref(int v) { return static_cast<int8_t>(v & 255); }
__device__ __forceinline__ int pk_mx(int v) { return (v << 12) >> 20; }
__device__ __forceinline__ int pk_my(int v) { return v >> 20; }

__device__ __forceinline__ NbMv16 nb_packed(bool avail, bool intra, int v) {
  NbMv16 n{avail, -1, {0, 0}};
  if (!avail || intra) return n;
  n.ref = pk_ref(v);
  if (n.ref >= 0) {
    n.mv[0] = pk_mx(v);
    n.mv[1] = pk_my(v);
  }
  return n;
}

// The row above hands its final motion on through LDS, never through global memory: per MB
// column the intra flag and the bottom quadrants (2, 3) of both lists, double-buffered by row
// parity (row y + 1 overwrites column x of row y - 1's entries only after row y has passed
// column x + 1, the last step that reads it).  The left neighbour stays in registers.
// Each wave runs two MB rows in lock step (half-waves: row 2w + 32k in lanes 0..31, the row
// below in lanes 32..63 two MBs behind), 8 samples per lane, so 16 waves cover 32 rows and
// the per-wave serial work (not the wavefront chain) stops bounding the kernel.
__global__ __launch_bounds__(64 * kSpatialWaves) void b_spatial_decide(BSpatialArgs a) {
  const Geom& g = a.g;
  const int slot = blockIdx.x, nmb = g.nmb();
  if (!route_active(a.rt, slot, SK_B)) return;  // uniform per workgroup
  __shared__ int prog[kMaxRows];
  __shared__ int s_res[kSpatialWaves][2][256];
  __shared__ int nbq[2][kMaxCols][5];  // [row parity][column]: intra, L0 q2, L0 q3, L1 q2, L1 q3
  for (int i = threadIdx.x; i < g.hmb; i += blockDim.x) prog[i] = 0;
  __syncthreads();
  const int w = wave_id(), lane = lane_id();
  const int half = lane >> 5, hl = lane & 31;
  const int r = hl >> 1, c0 = (hl & 1) * 8, q = (r >> 3) * 2 + (c0 >> 3);
  const int W = g.W, Hh = g.H, wmb = g.wmb, hmb = g.hmb;
  const size_t yo = static_cast<size_t>(slot) * g.ysize();
  const size_t hps = hp_plane_bytes(W, Hh);
  size_t sk[kMaxRefs];
#pragma unroll
  for (int k = 0; k < kMaxRefs; ++k) sk[k] = route_index(a.rt, a.nbuf, slot, RO_L0 + k);
  const size_t s1 = route_index(a.rt, a.nbuf, slot, RO_L1);
  const int16_t* w1t = a.rt ? a.rt[slot].w1 : nullptr;
  const bool col_l1 = a.rt && a.rt[slot].col_l1;
  MbHeader* H = a.hdr + static_cast<size_t>(slot) * nmb;
  const MbHeader* C0 = a.col + s1 * nmb;
  const int* IC = a.intra_cost + static_cast<size_t>(slot) * nmb;
  int* CB = a.cost + static_cast<size_t>(slot) * nmb;
  int* res = s_res[w][half];
  const int lam_base = a.qp[slot];  // (loaded once: the loop below is the serial chain)
  for (int yu = 2 * w; yu < hmb; yu += 2 * kSpatialWaves) {
    const int y = yu + half;
    const bool row_ok = y < hmb;
    int* cur_row = &nbq[y & 1][0][0];
    const int* up_row = &nbq[(y & 1) ^ 1][0][0];
    int left_intra = 0, left_q1[2] = {0, 0};  // lanes 0 / 32: the left MB's intra flag / quadrant 1
    for (int step = 0; step < wmb + 2; ++step) {
      const int x = half ? step - 2 : step;
      const bool act = row_ok && x >= 0 && x < wmb;
      const int xs = act ? x : 0, ys = act ? y : 0;  // in-range addresses for idle halves
      const int mb = ys * wmb + xs;
      const size_t o = static_cast<size_t>(slot) * nmb + mb;
      // chain-independent inputs first (in flight during the wait)
      const int ic = IC[mb];
      const int cost_e = CB[mb];
      const bool forced = H[mb].kind == h264::MBK_BDIRECT;
      // b_decide's explicit record (kept when direct loses)
      const uint2 href = *reinterpret_cast<const uint2*>(&H[mb].ref[0][0]);
      const uint4 hmv0 = *reinterpret_cast<const uint4*>(&H[mb].mv[0][0][0]);
      const uint4 hmv1 = *reinterpret_cast<const uint4*>(&H[mb].mv[1][0][0]);
      const int lambda = h264::kLambda[clampi(lam_base + (a.aq ? a.aq[o] : 0), 0, 51)];
      const MbHeader& c = C0[mb];
      const uint2 cref = *reinterpret_cast<const uint2*>(&c.ref[0][0]);  // ref[2][4]
      const uint4 cmv = *reinterpret_cast<const uint4*>(&c.mv[0][0][0]);  // list-0 vectors
      const uint4 cmv1 = col_l1 ? *reinterpret_cast<const uint4*>(&c.mv[1][0][0]) : make_uint4(0u, 0u, 0u, 0u);
      const int ckind = c.kind;
      const int X = xs * 16 + c0, Y = ys * 16 + r;
      const uint2 src = *reinterpret_cast<const uint2*>(a.src_y + yo + static_cast<size_t>(Y) * W + X);
      // the upper row waits on the row above (the previous wave's lower row); the lower row's
      // dependency, the upper half two MBs ahead, is met by the lock step
      if (yu > 0) row_wait_lds(prog, yu - 1, min(step + 2, wmb), a.err);
      int pk[4][2] = {{0, 0}, {0, 0}, {0, 0}, {0, 0}};
      if (hl == 0 && act) {
        const bool aA = x > 0, aB = y > 0, aC = y > 0 && x + 1 < wmb, aD = x > 0 && y > 0;
        const int* uB = up_row + x * 5;
        const int* uC = up_row + (x + 1) * 5;
        const int* uD = up_row + (x - 1) * 5;
        int refs[2], pmv[2][2];
        for (int l = 0; l < 2; ++l) {
          const NbMv16 A = nb_packed(aA, left_intra, left_q1[l]);
          const NbMv16 B = aB ? nb_packed(true, uB[0], uB[1 + 2 * l]) : NbMv16{false, -1, {0, 0}};
          const NbMv16 C = aC ? nb_packed(true, uC[0], uC[1 + 2 * l])
                        : (aD ? nb_packed(true, uD[0], uD[2 + 2 * l]) : NbMv16{false, -1, {0, 0}});
          spatial_pmv(A, B, C, refs[l], pmv[l][0], pmv[l][1]);
        }
        const bool zero = refs[0] < 0 && refs[1] < 0;
        const bool cintra = h264::mbk_is_intra(ckind);
        const uint32_t cmw[4] = {cmv.x, cmv.y, cmv.z, cmv.w};
        const uint32_t cmw1[4] = {cmv1.x, cmv1.y, cmv1.z, cmv1.w};
#pragma unroll
        for (int qq = 0; qq < 4; ++qq) {
          // 8.4.1.2.1: the co-located block's list-0 motion, or its list-1 motion when it has
          // none (only a B picture -- b-pyramid -- can be list-1 only)
          const int cr0 = static_cast<int8_t>((cref.x >> (8 * qq)) & 255u);
          const bool use1 = col_l1 && cr0 < 0;
          const int cr = use1 ? static_cast<int8_t>((cref.y >> (8 * qq)) & 255u) : cr0;
          const uint32_t cw_ = use1 ? cmw1[qq] : cmw[qq];
          const int cx = static_cast<int16_t>(cw_ & 0xFFFFu), cy = static_cast<int16_t>(cw_ >> 16);
          const bool col_zero = !cintra && cr == 0 && abs(cx) <= 1 && abs(cy) <= 1;
#pragma unroll
          for (int l = 0; l < 2; ++l) {
            int rf = refs[l], mx = pmv[l][0], my = pmv[l][1];
            if (zero) {
              rf = 0;
              mx = my = 0;
            } else if (rf < 0 || (rf == 0 && col_zero)) {
              mx = my = 0;
            }
            pk[qq][l] = (rf & 255) | ((mx & 4095) << 8) | (my << 20);
          }
        }
      }
      int mine[2] = {0, 0};
#pragma unroll
      for (int qq = 0; qq < 4; ++qq)
#pragma unroll
        for (int l = 0; l < 2; ++l) {
          const int vu = __builtin_amdgcn_readlane(pk[qq][l], 0), vl = __builtin_amdgcn_readlane(pk[qq][l], 32);
          if (qq == q) mine[l] = half ? vl : vu;
        }
      const int r0 = pk_ref(mine[0]), r1 = pk_ref(mine[1]);
      uint32_t pw[2];
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        uint32_t p0 = 0, p1 = 0;
        if (r0 >= 0)
          p0 = mc4(a.ref0k[r0 & 3] + sk[r0 & 3] * g.ysize(), a.hp0k[r0 & 3] + sk[r0 & 3] * hps, W, Hh, X + 4 * k, Y,
                   pk_mx(mine[0]), pk_my(mine[0]));
        if (r1 >= 0) p1 = mc4(a.ref1 + s1 * g.ysize(), a.hp1 + s1 * hps, W, Hh, X + 4 * k, Y, pk_mx(mine[1]), pk_my(mine[1]));
        pw[k] = (r0 >= 0 && r1 >= 0) ? wavg4b(p0, p1, w1t ? static_cast<int>(w1t[r0 & 3]) : a.w1[r0 & 3])
                                     : (r0 >= 0 ? p0 : p1);
      }
      const uint32_t sw[2] = {src.x, src.y};
#pragma unroll
      for (int k = 0; k < 8; ++k)
        res[r * 16 + c0 + k] = static_cast<int>((sw[k >> 2] >> (8 * (k & 3))) & 255u) -
                               static_cast<int>((pw[k >> 2] >> (8 * (k & 3))) & 255u);
      wave_sync();
      int satd = 0;
      if (hl < 16) {  // block hl of this half's MB; rows of 16 lanes sum below
        const int bx = (hl & 3) * 4, by = (hl >> 2) * 4;
        int rr[16];
#pragma unroll
        for (int yy = 0; yy < 4; ++yy)
#pragma unroll
          for (int xx = 0; xx < 4; ++xx) rr[yy * 4 + xx] = res[(by + yy) * 16 + bx + xx];
        satd = h264::satd4x4(rr);
      }
      const int ssum = sum16(satd);
      const int su = __builtin_amdgcn_readlane(ssum, 0), sl = __builtin_amdgcn_readlane(ssum, 32);
      const int cost_d = (half ? sl : su) + lambda;
      const bool take = act && (forced || cost_d <= cost_e + a.bias * lambda);
      const int final_cost = take ? cost_d : cost_e;
      const bool intra = ic < final_cost;  // encode_inter's rule
      if (take) *reinterpret_cast<uint2*>(a.pred_out + o * 256 + r * 16 + c0) = make_uint2(pw[0], pw[1]);
      if (hl == 0 && act) {
        // this MB's final motion: the direct one, else the explicit record b_decide wrote
        int fin[4][2];
        if (take) {
#pragma unroll
          for (int qq = 0; qq < 4; ++qq) {
            fin[qq][0] = pk[qq][0];
            fin[qq][1] = pk[qq][1];
          }
        } else {
          const uint32_t hm[2][4] = {{hmv0.x, hmv0.y, hmv0.z, hmv0.w}, {hmv1.x, hmv1.y, hmv1.z, hmv1.w}};
          const uint32_t hr[2] = {href.x, href.y};
#pragma unroll
          for (int qq = 0; qq < 4; ++qq)
#pragma unroll
            for (int l = 0; l < 2; ++l) {
              const int mx = static_cast<int16_t>(hm[l][qq] & 0xFFFFu), my = static_cast<int16_t>(hm[l][qq] >> 16);
              fin[qq][l] = static_cast<int>((hr[l] >> (8 * qq)) & 255u) | ((mx & 4095) << 8) | (my << 20);
            }
        }
        int* e = cur_row + x * 5;
        e[0] = intra;
        e[1] = fin[2][0];
        e[2] = fin[3][0];
        e[3] = fin[2][1];
        e[4] = fin[3][1];
        left_intra = intra;
        left_q1[0] = fin[1][0];
        left_q1[1] = fin[1][1];
        if (take) {
          MbHeader& h = H[mb];
          h.kind = h264::MBK_BDIRECT;
          h.sub_direct = 0;
#pragma unroll
          for (int qq = 0; qq < 4; ++qq)
#pragma unroll
            for (int l = 0; l < 2; ++l) {
              h.ref[l][qq] = static_cast<int8_t>(pk_ref(pk[qq][l]));
              h.mv[l][qq][0] = static_cast<int16_t>(pk_mx(pk[qq][l]));
              h.mv[l][qq][1] = static_cast<int16_t>(pk_my(pk[qq][l]));
            }
          CB[mb] = cost_d;
        }
      }
      // publish: the lower half's own next step reads the upper half's LDS entries in program
      // order; the next wave's upper row waits on this wave's lower row (prog)
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
      wave_sync();
      if (hl == 0 && act) __hip_atomic_store(prog + y, x + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
  }
}

// ---------------------------------------------------------------- spatial direct, fast path
// b_decide (spatial = 2) prices direct in parallel with an estimate of the spatial motion and
// decides every MB; what it cannot know is the neighbours' *final* motion, which 8.4.1.2.2
// derives the direct motion from.  b_spatial_exact walks each slot's MBs in decoding order --
// integer work only, one lane per MB row (row y two MBs behind row y - 1, all rows of a slot in
// one workgroup in lock step, a barrier per step) -- and writes the exact motion of every
// direct MB / B_Direct_8x8 quadrant into its record, flagging the MBs whose motion changed;
// b_spatial_fixup then re-predicts those (fully parallel).  The decisions and costs stay as
// b_decide made them (encode_inter's intra-vs-inter rule, which the derivation must agree on,
// reads the same costs), so the bitstream is exact while the serial chain costs microseconds
// instead of b_spatial_decide's SATD per MB on the chain.
struct BSpatialExactArgs {
  Geom g;
  MbHeader* hdr;          // [B, nmb] in / out
  const int* intra_cost;  // [B, nmb]: an MB turns intra when intra_cost < cost (encode_inter)
  const int* cost;        // [B, nmb]
  const uint8_t* czero;   // [B, nmb] colZeroFlag bits (b_direct_mv)
  uint8_t* fix;           // [B, nmb] out: 1 = the direct motion changed, re-predict; 2 = made explicit
  const SlotRoute* rt;
  int slice_rows;         // MB rows per slice (0: one slice): no neighbours above a slice's first row
  // quarter-sample tolerance: a direct quadrant whose exact motion is further than this from
  // the estimate b_decide priced keeps the estimate as explicit motion; -1 = never (the direct
  // MB is always re-predicted with the exact motion)
  int tol;
};

__global__ __launch_bounds__(64 * kExactWaves) void b_spatial_exact(BSpatialExactArgs a) {
  const Geom& g = a.g;
  const int slot = blockIdx.x, nmb = g.nmb(), wmb = g.wmb, hmb = g.hmb;
  if (!route_active(a.rt, slot, SK_B)) return;  // uniform per workgroup
  __shared__ int nbq[2][kMaxCols][5];      // [row parity][column]: intra, L0 q2, L0 q3, L1 q2, L1 q3
  const int y = threadIdx.x;
  const bool row_ok = y < hmb;
  MbHeader* H = a.hdr + static_cast<size_t>(slot) * nmb;
  const int* IC = a.intra_cost + static_cast<size_t>(slot) * nmb;
  const int* CB = a.cost + static_cast<size_t>(slot) * nmb;
  const uint8_t* CZ = a.czero + static_cast<size_t>(slot) * nmb;
  uint8_t* FX = a.fix + static_cast<size_t>(slot) * nmb;
  int* cur_row = &nbq[y & 1][0][0];
  const int* up_row = &nbq[(y & 1) ^ 1][0][0];
  int left_intra = 0, left_q1[2] = {0, 0};
  const int nsteps = wmb + 2 * (hmb - 1);
  for (int step = 0; step < nsteps; ++step) {
    const int x = step - 2 * y;
    if (row_ok && x >= 0 && x < wmb) {
      const int mb = y * wmb + x;
      MbHeader& h = H[mb];
      const int kind = h.kind;
      const bool intra = IC[mb] < CB[mb];
      const int sdir = kind == h264::MBK_BDIRECT ? 15 : (kind == h264::MBK_B8x8 ? h.sub_direct : 0);
      int fin[4][2];
#pragma unroll
      for (int qq = 0; qq < 4; ++qq)
#pragma unroll
        for (int l = 0; l < 2; ++l)
          fin[qq][l] = (h.ref[l][qq] & 255) | ((h.mv[l][qq][0] & 4095) << 8) | (h.mv[l][qq][1] << 20);
      bool changed = false, converted = false;
      if (!intra && sdir) {
        const bool top = y > 0 && (a.slice_rows <= 0 || y % a.slice_rows != 0);
        const bool aA = x > 0, aB = top, aC = top && x + 1 < wmb, aD = x > 0 && top;
        int refs[2], pmv[2][2];
#pragma unroll
        for (int l = 0; l < 2; ++l) {
          const NbMv16 A = nb_packed(aA, left_intra, left_q1[l]);
          const NbMv16 Bn = aB ? nb_packed(true, up_row[x * 5], up_row[x * 5 + 1 + 2 * l]) : NbMv16{false, -1, {0, 0}};
          const NbMv16 C = aC ? nb_packed(true, up_row[(x + 1) * 5], up_row[(x + 1) * 5 + 1 + 2 * l])
                              : (aD ? nb_packed(true, up_row[(x - 1) * 5], up_row[(x - 1) * 5 + 2 + 2 * l])
                                    : NbMv16{false, -1, {0, 0}});
          spatial_pmv(A, Bn, C, refs[l], pmv[l][0], pmv[l][1]);
        }
        const bool zero = refs[0] < 0 && refs[1] < 0;
        const int cz = CZ[mb];
        int ex[4][2][3];    // exact motion of the direct quadrants: ref, mvx, mvy per list
        int conv = 0;       // quadrants whose exact motion is off the estimate by more than tol
        int moved = 0;      // quadrants whose exact motion differs at all
#pragma unroll
        for (int qq = 0; qq < 4; ++qq) {
          if (!((sdir >> qq) & 1)) continue;
#pragma unroll
          for (int l = 0; l < 2; ++l) {
            int rf = refs[l], vx = pmv[l][0], vy = pmv[l][1];
            if (zero) {
              rf = 0;
              vx = vy = 0;
            } else if (rf < 0 || (rf == 0 && ((cz >> qq) & 1))) {
              vx = vy = 0;
            }
            ex[qq][l][0] = rf;
            ex[qq][l][1] = vx;
            ex[qq][l][2] = vy;
            const int er = h.ref[l][qq], evx = h.mv[l][qq][0], evy = h.mv[l][qq][1];
            if (((rf & 255) | ((vx & 4095) << 8) | (vy << 20)) != fin[qq][l]) moved |= 1 << qq;
            if (rf != er || (rf >= 0 && (abs(vx - evx) > a.tol || abs(vy - evy) > a.tol))) conv |= 1 << qq;
          }
        }
        if (conv && a.tol >= 0) {
          converted = true;
          // The prediction b_decide priced (and encode_inter will subtract) is the estimate's:
          // instead of re-predicting with motion nobody priced, the MB keeps the estimated
          // motion and codes it explicitly -- B_L0 / L1 / Bi partitions of the shape the
          // quadrant motion allows (B_Direct_16x16) or explicit 8x8 sub-blocks (B_8x8).  Its
          // final motion (what later MBs derive from) is then the estimate, already in `fin`.
          if (kind == h264::MBK_BDIRECT) {
            auto same = [&](int p, int q) { return fin[p][0] == fin[q][0] && fin[p][1] == fin[q][1]; };
            h.kind = (same(0, 1) && same(2, 3)) ? (same(0, 2) ? h264::MBK_B16x16 : h264::MBK_B16x8)
                                                : ((same(0, 2) && same(1, 3)) ? h264::MBK_B8x16 : h264::MBK_B8x8);
            h.sub_direct = 0;
            moved = 0;  // no quadrant keeps direct
          } else {
            h.sub_direct = static_cast<uint8_t>(h.sub_direct & ~conv);
            moved &= ~conv;
          }
        }
        // the remaining direct quadrants take the exact motion (re-predicted by b_spatial_fixup)
#pragma unroll
        for (int qq = 0; qq < 4; ++qq) {
          if (!((moved >> qq) & 1)) continue;
          changed = true;
#pragma unroll
          for (int l = 0; l < 2; ++l) {
            const int rf = ex[qq][l][0], vx = ex[qq][l][1], vy = ex[qq][l][2];
            fin[qq][l] = (rf & 255) | ((vx & 4095) << 8) | (vy << 20);
            h.ref[l][qq] = static_cast<int8_t>(rf);
            h.mv[l][qq][0] = static_cast<int16_t>(vx);
            h.mv[l][qq][1] = static_cast<int16_t>(vy);
          }
        }
      }
      FX[mb] = changed ? 1 : (converted ? 2 : 0);  // 2: explicit now, prediction unchanged
      int* e = cur_row + x * 5;
      e[0] = intra;
      e[1] = fin[2][0];
      e[2] = fin[3][0];
      e[3] = fin[2][1];
      e[4] = fin[3][1];
      left_intra = intra;
      left_q1[0] = fin[1][0];
      left_q1[1] = fin[1][1];
    }
    __syncthreads();
  }
}

// Re-prediction of the direct quadrants whose exact motion differs from b_decide's estimate.
struct BSpatialFixArgs {
  Geom g;
  const MbHeader* hdr;
  const uint8_t* fix;
  const uint8_t *ref0, *hp0;  // pools [B, nbuf, plane] (every list-0 entry, by route)
  const uint8_t *ref1, *hp1;
  uint8_t* pred_out;
  const SlotRoute* rt;
  int nbuf;
};

__global__ __launch_bounds__(64) void b_spatial_fixup(BSpatialFixArgs a) {
  const Geom& g = a.g;
  const int nmb = g.nmb();
  int mb, slot;
  xcd_unit_slot(mb, slot);
  if (!route_active(a.rt, slot, SK_B)) return;
  const size_t o = static_cast<size_t>(slot) * nmb + mb;
  if (a.fix[o] != 1) return;  // wave-uniform
  const int lane = threadIdx.x;
  const int mx = mb % g.wmb, my = mb / g.wmb;
  const int W = g.W, H = g.H;
  const int r = lane >> 2, c0 = (lane & 3) * 4;
  const int X = mx * 16 + c0, Y = my * 16 + r;
  const int q = (r >> 3) * 2 + (c0 >> 3);
  const MbHeader& h = a.hdr[o];
  const bool dq = h.kind == h264::MBK_BDIRECT || (h.kind == h264::MBK_B8x8 && ((h.sub_direct >> q) & 1));
  if (!dq) return;  // (lane-divergent exit after the last wave-wide step)
  const size_t hps = hp_plane_bytes(W, H);
  const int r0 = h.ref[0][q], r1 = h.ref[1][q];
  uint32_t p0 = 0, p1 = 0;
  if (r0 >= 0) {
    const size_t s0 = route_index(a.rt, a.nbuf, slot, RO_L0 + (r0 & 3));
    p0 = mc4(a.ref0 + s0 * g.ysize(), a.hp0 + s0 * hps, W, H, X, Y, h.mv[0][q][0], h.mv[0][q][1]);
  }
  if (r1 >= 0) {
    const size_t s1 = route_index(a.rt, a.nbuf, slot, RO_L1);
    p1 = mc4(a.ref1 + s1 * g.ysize(), a.hp1 + s1 * hps, W, H, X, Y, h.mv[1][q][0], h.mv[1][q][1]);
  }
  const int w1 = a.rt ? a.rt[slot].w1[r0 & 3] : 32;
  *reinterpret_cast<uint32_t*>(a.pred_out + o * 256 + r * 16 + c0) =
      (r0 >= 0 && r1 >= 0) ? wavg4b(p0, p1, w1) : (r0 >= 0 ? p0 : p1);
}

}  // namespace gpu
}  // namespace mivc

using namespace mivc::gpu;

extern "C" void mivc_launch_b_direct(int B, int wmb, int hmb, const void* col, const int* dsf, const int* direct_copy,
                                     int nref, int16_t* dmv, int8_t* dref, int16_t* pm0, int16_t* pm1, void* stream,
                                     const void* route, int nbuf, uint8_t* czero, const int8_t* cmap) {
  BDirectArgs a;
  a.czero = czero;
  a.cmap = cmap;
  a.rt = static_cast<const SlotRoute*>(route);
  a.nbuf = nbuf;
  a.g = Geom{B, wmb, hmb, wmb * 16, hmb * 16};
  a.col = static_cast<const MbHeader*>(col);
  for (int r = 0; r < kMaxRefs; ++r) {  // refIdxCol beyond the list: the last entry (never produced)
    const int rr = r < nref ? r : nref - 1;
    a.dsf[r] = dsf[rr];
    a.direct_copy[r] = direct_copy[rr];
  }
  a.dmv = dmv;
  a.dref = dref;
  a.pm0 = pm0;
  a.pm1 = pm1;
  hipLaunchKernelGGL(b_direct_mv, dim3((wmb * hmb + 255) / 256, B), dim3(256), 0, static_cast<hipStream_t>(stream), a);
}

extern "C" void mivc_launch_b_decide(int B, int wmb, int hmb, const uint8_t* src_y, const uint8_t* ref0,
                                     const uint8_t* ref1, const uint8_t* hp0, const uint8_t* hp1, const int16_t* mv0,
                                     const int16_t* mv1, const int* cost0, const int* cost1, const uint8_t* pred0,
                                     const uint8_t* pred1, const int16_t* pm0, const int16_t* pm1, const int16_t* dmv,
                                     const int* qp, const int8_t* aq, void* hdr, uint8_t* pred_out, int* cost_out,
                                     void* stream, const int* w1, int nref, const int8_t* dref,
                                     const uint8_t* const* ref0k, const uint8_t* const* hp0k, int direct_only, int bparts, int have_direct,
                                     int spatial, int dbias, const void* route, int nbuf, const uint8_t* czero) {
  BDecideArgs a;
  a.czero = czero;
  a.rt = static_cast<const SlotRoute*>(route);
  a.nbuf = nbuf;
  a.spatial = spatial;
  a.dbias = dbias;
  a.direct_only = direct_only;
  a.have_direct = have_direct;
  a.bparts = bparts;
  for (int r = 0; r < kMaxRefs; ++r) {
    const int rr = r < nref ? r : nref - 1;
    a.w1[r] = w1[rr];
    a.ref0k[r] = rr == 0 ? ref0 : ref0k[rr];
    a.hp0k[r] = rr == 0 ? hp0 : hp0k[rr];
  }
  a.dref = dref;
  a.g = Geom{B, wmb, hmb, wmb * 16, hmb * 16};
  a.src_y = src_y;
  a.ref0 = ref0;
  a.ref1 = ref1;
  a.hp0 = hp0;
  a.hp1 = hp1;
  a.mv0 = mv0;
  a.mv1 = mv1;
  a.cost0 = cost0;
  a.cost1 = cost1;
  a.pred0 = pred0;
  a.pred1 = pred1;
  a.pm0 = pm0;
  a.pm1 = pm1;
  a.dmv = dmv;
  a.qp = qp;
  a.aq = aq;
  a.hdr = static_cast<MbHeader*>(hdr);
  a.pred_out = pred_out;
  a.cost_out = cost_out;
  const dim3 grid(mb_row_grid(wmb * hmb), B);
  const hipStream_t st = static_cast<hipStream_t>(stream);
  if (direct_only && spatial == 0)
    hipLaunchKernelGGL(b_decide<3>, grid, dim3(64), 0, st, a);
  else if (direct_only)
    hipLaunchKernelGGL(b_decide<1>, grid, dim3(64), 0, st, a);
  else if (have_direct)
    hipLaunchKernelGGL(b_decide<2>, grid, dim3(64), 0, st, a);
  else
    hipLaunchKernelGGL(b_decide<0>, grid, dim3(64), 0, st, a);
}

extern "C" void mivc_launch_b_spatial(int B, int wmb, int hmb, void* hdr, const void* col, const uint8_t* src_y,
                                      const uint8_t* ref1, const uint8_t* hp1, const uint8_t* const* ref0k,
                                      const uint8_t* const* hp0k, const int* w1, int nref, uint8_t* pred_out, int* err,
                                      void* stream, const int* intra_cost, int* cost, const int* qp, const int8_t* aq,
                                      int bias, const void* route, int nbuf) {
  BSpatialArgs a;
  a.rt = static_cast<const SlotRoute*>(route);
  a.nbuf = nbuf;
  a.bias = bias;
  a.g = Geom{B, wmb, hmb, wmb * 16, hmb * 16};
  a.hdr = static_cast<MbHeader*>(hdr);
  a.col = static_cast<const MbHeader*>(col);
  a.err = err;
  a.intra_cost = intra_cost;
  a.cost = cost;
  a.src_y = src_y;
  a.ref1 = ref1;
  a.hp1 = hp1;
  for (int r = 0; r < kMaxRefs; ++r) {
    const int rr = r < nref ? r : nref - 1;
    a.ref0k[r] = ref0k[rr];
    a.hp0k[r] = hp0k[rr];
    a.w1[r] = w1[rr];
  }
  a.pred_out = pred_out;
  a.qp = qp;
  a.aq = aq;
  hipLaunchKernelGGL(b_spatial_decide, dim3(B), dim3(64 * kSpatialWaves), 0, static_cast<hipStream_t>(stream), a);
}

extern "C" void mivc_launch_b_spatial_exact(int B, int wmb, int hmb, void* hdr, const int* intra_cost, const int* cost,
                                            const uint8_t* czero, uint8_t* fix, void* stream, const void* route,
                                            int slice_rows, int tol) {
  BSpatialExactArgs a;
  a.slice_rows = slice_rows;
  a.tol = tol;
  a.g = Geom{B, wmb, hmb, wmb * 16, hmb * 16};
  a.hdr = static_cast<MbHeader*>(hdr);
  a.intra_cost = intra_cost;
  a.cost = cost;
  a.czero = czero;
  a.fix = fix;
  a.rt = static_cast<const SlotRoute*>(route);
  const int waves = (hmb + 63) / 64;
  hipLaunchKernelGGL(b_spatial_exact, dim3(B), dim3(64 * waves), 0, static_cast<hipStream_t>(stream), a);
}

extern "C" void mivc_launch_b_spatial_fixup(int B, int wmb, int hmb, const void* hdr, const uint8_t* fix,
                                            const uint8_t* ref0, const uint8_t* hp0, const uint8_t* ref1,
                                            const uint8_t* hp1, uint8_t* pred_out, void* stream, const void* route,
                                            int nbuf) {
  BSpatialFixArgs a;
  a.g = Geom{B, wmb, hmb, wmb * 16, hmb * 16};
  a.hdr = static_cast<const MbHeader*>(hdr);
  a.fix = fix;
  a.ref0 = ref0;
  a.hp0 = hp0;
  a.ref1 = ref1;
  a.hp1 = hp1;
  a.pred_out = pred_out;
  a.rt = static_cast<const SlotRoute*>(route);
  a.nbuf = nbuf;
  hipLaunchKernelGGL(b_spatial_fixup, dim3(wmb * hmb, B), dim3(64), 0, static_cast<hipStream_t>(stream), a);
}
