// HEVC merge-aware motion choice on the 16x16 grid, after the searches (me.hip):
//   hevc_merge_refine (four blocks per wave)  P pictures, the spatial neighbours' vectors
//   hevc_b_choose     (four blocks per wave)  B pictures: L0 / L1 / bi from the two searches
//   hevc_b_init_p     (thread per block)      P pictures enter the merge passes in B form
//   hevc_b_merge      (four blocks per wave)  the writer's exact merge list per block (Jacobi)
#include "kcommon.h"
#include "launch.h"
#include "mb_row.h"
#include "qpel.h"
#include "../common/hevc_tables.h"

namespace mivc {
namespace gpu {

// ---- HEVC merge-aware vector choice (the H.265 analogue of p_mv_refine): after the 16x16
// search each block is offered the current vectors of its spatial merge neighbours (A1 left,
// B1 above, B0 above-right, A0 below-left, B2 above-left; 8.5.3.2.3) and the zero vector;
// the cheapest by SATD + lambda * (merge_idx bits) replaces the searched vector when it beats
// the search's SATD + lambda * mvd bits, so the CABAC writer can code the CU as merge / skip.
// Jacobi pass: reads mv_in, writes mv_out.  (The candidates approximate the normative merge
// list on the 16x16 grid; the writer codes AMVP whenever the vector is not in the real list.)
// With several slices per picture a slice's first block row has no neighbours above.

// first 16x16 block row of the slice that holds block row my (sh = log2(CTU size / 16); slices
// are whole CTU rows, hevc_tables.h slice_of_row)
__device__ __forceinline__ int slice_top16(const Geom& g, int sh, int slices, int my) {
  if (slices <= 1) return 0;
  const int hu = (g.hmb + (1 << sh) - 1) >> sh;
  return hevc::slice_first_row(hevc::slice_of_row(my >> sh, slices, hu), slices, hu) << sh;
}

struct MergeRefineArgs {
  Geom g;
  const uint8_t* src_y;
  const uint8_t* ref;       // 8-bit proxy of the reference
  const uint8_t* hp;        // its half-sample planes
  const int16_t* mv_in;     // [B, nmb, 2]
  int16_t* mv_out;          // [B, nmb, 2]
  int* cost;                // [B, nmb] ME cost (SATD + lambda * bits vs pm), updated in place
  const int16_t* pm;        // [B, nmb, 2] the ME's predictor (to recover the SATD part of cost)
  const int* qp;
  const int8_t* aq;
  int ctu_shift;            // log2(CTU size / 16): 1 for 32x32 CTBs, 2 for 64x64 CTUs
  int slices;               // slices per picture
};

__global__ __launch_bounds__(64) void hevc_merge_refine(MergeRefineArgs a) {
  const Geom& g = a.g;
  const MbRow r = mb_row(g);
  if (!r.live) return;
  const int nmb = g.nmb(), slot = r.slot, mb = r.mb, lane = r.lane, mx = r.mx, my = r.my;
  const size_t o = r.o;
  const int16_t* mv = a.mv_in + static_cast<size_t>(slot) * nmb * 2;
  const int cx = mv[mb * 2], cy = mv[mb * 2 + 1];
  int kx[6], ky[6], nk = 0;
  auto add = [&](bool ok, int n) {
    if (!ok) return;
    const int vx = mv[n * 2], vy = mv[n * 2 + 1];
    for (int j = 0; j < nk; ++j)
      if (kx[j] == vx && ky[j] == vy) return;
    kx[nk] = vx;
    ky[nk] = vy;
    ++nk;
  };
  const int top = slice_top16(g, a.ctu_shift, a.slices, my);  // the slice's first block row
  add(mx > 0, mb - 1);                              // A1
  add(my > top, mb - g.wmb);                        // B1
  add(my > top && mx < g.wmb - 1, mb - g.wmb + 1);  // B0
  add(mx > 0 && my < g.hmb - 1, mb + g.wmb - 1);    // A0
  add(mx > 0 && my > top, mb - g.wmb - 1);          // B2
  {
    bool z = false;
    for (int j = 0; j < nk; ++j) z |= kx[j] == 0 && ky[j] == 0;
    if (!z) {
      kx[nk] = 0;
      ky[nk] = 0;
      ++nk;
    }
  }
  const int lambda = mb_lambda(a.qp, a.aq, slot, o);
  const int pmx = a.pm ? a.pm[o * 2] : 0, pmy = a.pm ? a.pm[o * 2 + 1] : 0;
  const int c_me = a.cost[o];  // SATD + lambda * mvd bits against the search predictor
  const int W = g.W, H = g.H, X = r.X, Y = r.Y;
  const uint8_t* G0 = a.ref + static_cast<size_t>(slot) * g.ysize();
  const uint8_t* H0 = a.hp + static_cast<size_t>(slot) * hp_plane_bytes(W, H);
  uint32_t src[4];
  load_src4(g, r, a.src_y, src);
  int best = c_me, bx_ = cx, by_ = cy;
  for (int j = 0; j < nk; ++j) {
    if (kx[j] == cx && ky[j] == cy) {  // the searched vector is itself a merge candidate
      const int cst = c_me - lambda * (mvbits_se(cx - pmx) + mvbits_se(cy - pmy)) + lambda * (1 + j);
      if (cst < best) {  // also against an earlier candidate that had beaten the search: the vector goes with its price
        best = cst;
        bx_ = cx;
        by_ = cy;
      }
      continue;
    }
    uint32_t ps[4];
#pragma unroll
    for (int y = 0; y < 4; ++y) ps[y] = mc4(G0, H0, W, H, X, Y + y, kx[j], ky[j]);
    const int satd = row_satd(src, ps);
    const int cst = satd + lambda * (1 + j);  // merge_flag + truncated-unary merge_idx
    if (cst < best) {
      best = cst;
      bx_ = kx[j];
      by_ = ky[j];
    }
  }
  if (lane == 0) {
    a.mv_out[o * 2] = static_cast<int16_t>(bx_);
    a.mv_out[o * 2 + 1] = static_cast<int16_t>(by_);
    a.cost[o] = best;
  }
}

// ---- HEVC B pictures (x265 --bframes): the two searches (list 0 against the previous
// anchor, list 1 against the next) become one motion per 16x16 block -- L0, L1 or bi --
// and then merge-aware passes like hevc_merge_refine, over B motion (direction + two
// vectors).  Motion per block: mvb [B, nmb, 4] = (L0 x, y, L1 x, y), dir [B, nmb] (CuDir),
// cost = SATD + lambda * bits and bits (so a pass can recover the SATD part).
struct HevcBArgs {
  Geom g;
  const uint8_t* src_y;
  const uint8_t *ref0, *ref1;   // 8-bit proxies of RefPicList0[0] / RefPicList1[0]
  const uint8_t *hp0, *hp1;     // their half-sample planes
  const int16_t *mv0, *mv1;     // [B, nmb, 2] searched vectors
  const int *cost0, *cost1;     // their costs against pm0 / pm1
  const int16_t *pm0, *pm1;     // search predictors
  const int16_t* tmv;           // [B, nmb, 4] temporal merge candidate (both lists)
  const uint8_t* tdir;          // [B, nmb] its direction (0: none)
  const int16_t* mvb_in;        // [B, nmb, 4]
  const uint8_t* dir_in;        // [B, nmb]
  int16_t* mvb_out;
  uint8_t* dir_out;
  int* cost;                    // [B, nmb]
  int* bits;                    // [B, nmb]
  const int* qp;
  const int8_t* aq;
  int bslice;                   // 0: P picture (list 0 only)
  int max_merge;                // MaxNumMergeCand
  int ctu_shift;                // log2(CTU size / 16): 1 for 32x32 CTBs, 2 for 64x64 CTUs
  int slices;                   // slices per picture: a slice's first block row has no neighbours above
  // merge passes: blocks whose motion the previous pass changed (nullable: every block is
  // re-evaluated); a block whose own and whose neighbours' motion stayed put would rebuild the
  // same list at the same costs, so it only copies its motion through
  const uint8_t* chg_in;
  uint8_t* chg_out;
  // x265 --ref: P pictures with nref0 > 1 active list-0 pictures.  A motion's direction byte
  // carries its list-0 refIdx in bits 2-3 (CuDir in bits 0-1); xref / xhp are the proxies and
  // half-sample planes of RefPicList0[1 ..], and the P init pass picks per block among the
  // list-0[0] search (mv0 / cost0 / pm0) and the farther searches xmv / xcost / xpm
  // ([nref0 - 1, B, nmb, ...]; xcost kNoCost = not searched) at cost + lambda * ref_idx bins
  int nref0;
  const uint8_t* xref[3];
  const uint8_t* xhp[3];
  const int16_t* xmv;
  const int* xcost;
  const int16_t* xpm;
};

// RefPicList0[r]'s 8-bit proxy / half-sample planes (constant indices only: no scratch)
__device__ __forceinline__ const uint8_t* l0_ref(const HevcBArgs& a, int r) {
  return r == 0 ? a.ref0 : (r == 1 ? a.xref[0] : (r == 2 ? a.xref[1] : a.xref[2]));
}
__device__ __forceinline__ const uint8_t* l0_hp(const HevcBArgs& a, int r) {
  return r == 0 ? a.hp0 : (r == 1 ? a.xhp[0] : (r == 2 ? a.xhp[1] : a.xhp[2]));
}
// ref_idx_l0 bins (TR, cMax nref - 1)
__device__ __forceinline__ int ref_bins(int r, int nref) { return nref <= 1 ? 0 : min(r + 1, nref - 1); }

// z-scan availability (6.4.1) of the 16x16 block (nx, ny) for the block (mx, my) on the 16x16
// grid: CTUs in raster order, blocks inside a CTU in z-order; top = first block row of the
// current block's slice (slice_top16)
__device__ __forceinline__ bool avail16(const Geom& g, int sh, int nx, int ny, int mx, int my, int top) {
  if (nx < 0 || ny < top || nx >= g.wmb || ny >= g.hmb) return false;
  const int ux = nx >> sh, uy = ny >> sh, cx = mx >> sh, cy = my >> sh;
  if (ux != cx || uy != cy) return uy < cy || (uy == cy && ux < cx);
  const int m = (1 << sh) - 1;
  auto z = [](int x, int y) { return (x & 1) | ((y & 1) << 1) | ((x & 2) << 1) | ((y & 2) << 2); };
  return z(nx & m, ny & m) < z(mx & m, my & m);
}

// luma prediction (4 samples of row Y, columns X..X+3) of a B motion
__device__ __forceinline__ uint32_t mc4_b(const HevcBArgs& a, const uint8_t* G0, const uint8_t* H0, const uint8_t* G1,
                                          const uint8_t* H1, int X, int Y, int dir, int x0, int y0, int x1, int y1) {
  const int W = a.g.W, H = a.g.H;
  if (dir == 1) return mc4(G0, H0, W, H, X, Y, x0, y0);
  if (dir == 2) return mc4(G1, H1, W, H, X, Y, x1, y1);
  return avg4b(mc4(G0, H0, W, H, X, Y, x0, y0), mc4(G1, H1, W, H, X, Y, x1, y1));
}

__global__ __launch_bounds__(64) void hevc_b_choose(HevcBArgs a) {
  const Geom& g = a.g;
  const MbRow r = mb_row(g);
  if (!r.live) return;
  const int slot = r.slot, lane = r.lane;
  const size_t o = r.o;
  const size_t yo = static_cast<size_t>(slot) * g.ysize(), ho = static_cast<size_t>(slot) * hp_plane_bytes(g.W, g.H);
  const uint8_t *G0 = a.ref0 + yo, *G1 = a.ref1 + yo, *H0 = a.hp0 + ho, *H1 = a.hp1 + ho;
  const int x0 = a.mv0[o * 2], y0 = a.mv0[o * 2 + 1], x1 = a.mv1[o * 2], y1 = a.mv1[o * 2 + 1];
  uint32_t src[4], pw[4];
  load_src4(g, r, a.src_y, src);
#pragma unroll
  for (int y = 0; y < 4; ++y) pw[y] = mc4_b(a, G0, H0, G1, H1, r.X, r.Y + y, 3, x0, y0, x1, y1);
  const int satd_bi = row_satd(src, pw);
  const int lam = mb_lambda(a.qp, a.aq, slot, o);
  const int b0 = mvbits_se(x0 - a.pm0[o * 2]) + mvbits_se(y0 - a.pm0[o * 2 + 1]);
  const int b1 = mvbits_se(x1 - a.pm1[o * 2]) + mvbits_se(y1 - a.pm1[o * 2 + 1]);
  // inter_pred_idc: "1" bi, "00" / "01" single list
  const int c_l0 = a.cost0[o] + 2 * lam, c_l1 = a.cost1[o] + 2 * lam;
  const int c_bi = satd_bi + lam * (b0 + b1 + 1);
  int dir = 1, best = c_l0, bits = b0 + 2;
  if (c_l1 < best) { dir = 2; best = c_l1; bits = b1 + 2; }
  if (c_bi < best) { dir = 3; best = c_bi; bits = b0 + b1 + 1; }
  if (lane == 0) {
    int16_t* m = a.mvb_out + o * 4;
    m[0] = static_cast<int16_t>(dir & 1 ? x0 : 0);
    m[1] = static_cast<int16_t>(dir & 1 ? y0 : 0);
    m[2] = static_cast<int16_t>(dir & 2 ? x1 : 0);
    m[3] = static_cast<int16_t>(dir & 2 ? y1 : 0);
    a.dir_out[o] = static_cast<uint8_t>(dir);
    a.cost[o] = best;
    a.bits[o] = bits;
  }
}

// P pictures enter the merge passes in the same form: the list-0 search, bits = its mvd bits;
// with several list-0 pictures the cheapest search at cost + lambda * ref_idx bins
__global__ __launch_bounds__(256) void hevc_b_init_p(HevcBArgs a) {
  const int nmb = a.g.nmb();
  const int i = blockIdx.x * 256 + threadIdx.x, slot = blockIdx.y;
  if (i >= nmb) return;
  const size_t o = static_cast<size_t>(slot) * nmb + i;
  int x0 = a.mv0[o * 2], y0 = a.mv0[o * 2 + 1];
  int best = a.cost0[o], bits = mvbits_se(x0 - a.pm0[o * 2]) + mvbits_se(y0 - a.pm0[o * 2 + 1]), br = 0;
  if (a.nref0 > 1) {
    const int lam = mb_lambda(a.qp, a.aq, slot, o);
    best += lam * ref_bins(0, a.nref0);
    bits += ref_bins(0, a.nref0);
    const size_t plane = static_cast<size_t>(a.g.B) * nmb;
    for (int r = 1; r < a.nref0; ++r) {
      const size_t xo = (r - 1) * plane + o;
      const int c = a.xcost[xo];
      if (c >= kNoCost) continue;
      const int rb = ref_bins(r, a.nref0);
      if (c + lam * rb < best) {
        best = c + lam * rb;
        br = r;
        x0 = a.xmv[xo * 2];
        y0 = a.xmv[xo * 2 + 1];
        bits = mvbits_se(x0 - a.xpm[xo * 2]) + mvbits_se(y0 - a.xpm[xo * 2 + 1]) + rb;
      }
    }
  }
  int16_t* m = a.mvb_out + o * 4;
  m[0] = static_cast<int16_t>(x0);
  m[1] = static_cast<int16_t>(y0);
  m[2] = m[3] = 0;
  a.dir_out[o] = static_cast<uint8_t>(1 | (br << 2));
  a.cost[o] = best;
  a.bits[o] = bits;
}

// Jacobi pass.  Each block is offered the merge list the CABAC writer would build for it as a
// 16x16 CU (8.5.3.2.2-8.5.3.2.5 on the 16x16 grid of current motions, z-scan availability in
// a 32x32 CTB: the below-left neighbour exists only for quadrant 0, the above-right one not for
// quadrant 3; pruning A1-B1, B1-B0, A1-A0, A1/B1-B2; the temporal candidate, combined
// bi-predictive and zero candidates; MaxNumMergeCand entries); the cheapest by SATD + lambda *
// (merge_flag + merge_idx bins) replaces the block's motion when it beats its cost.
__global__ __launch_bounds__(64) void hevc_b_merge(HevcBArgs a) {
  const Geom& g = a.g;
  const MbRow r = mb_row(g);
  if (!r.live) return;
  const int nmb = g.nmb(), slot = r.slot, mb = r.mb, lane = r.lane, mx = r.mx, my = r.my;
  const size_t o = r.o;
  const size_t sb = static_cast<size_t>(slot) * nmb;
  const int maxc = a.max_merge;
  if (a.chg_in && !moved_nearby(g, r, a.chg_in + sb, true)) {
    if (lane == 0) {
      *reinterpret_cast<uint2*>(a.mvb_out + o * 4) = *reinterpret_cast<const uint2*>(a.mvb_in + o * 4);
      a.dir_out[o] = a.dir_in[o];
      if (a.chg_out) a.chg_out[o] = 0;
    }
    return;
  }
  int kd[6], kv[6][4], nk = 0;
  auto load = [&](int n, int* d, int* w) {
    const int dd = a.dir_in[sb + n];
    const int16_t* v = a.mvb_in + (sb + n) * 4;
    *d = dd;
    w[0] = dd & 1 ? v[0] : 0;
    w[1] = dd & 1 ? v[1] : 0;
    w[2] = dd & 2 ? v[2] : 0;
    w[3] = dd & 2 ? v[3] : 0;
  };
  auto same = [](int da, const int* wa, int db, const int* wb) {
    return da == db && wa[0] == wb[0] && wa[1] == wb[1] && wa[2] == wb[2] && wa[3] == wb[3];
  };
  int dA1 = 0, dB1 = 0, dB0 = 0, dA0 = 0, dB2 = 0, wA1[4], wB1[4], wB0[4], wA0[4], wB2[4];
  const int top = slice_top16(g, a.ctu_shift, a.slices, my);
  const bool a1 = mx > 0, av_b1 = my > top;
  // above-right / below-left: z-scan order inside the CTU (32x32: B0 unavailable for quadrant 3,
  // A0 available for quadrant 0 only)
  bool b0 = avail16(g, a.ctu_shift, mx + 1, my - 1, mx, my, top);
  bool a0 = avail16(g, a.ctu_shift, mx - 1, my + 1, mx, my, top);
  bool b2 = mx > 0 && my > top;
  if (a1) load(mb - 1, &dA1, wA1);
  if (av_b1) load(mb - g.wmb, &dB1, wB1);
  if (b0) load(mb - g.wmb + 1, &dB0, wB0);
  if (a0) load(mb + g.wmb - 1, &dA0, wA0);
  if (b2) load(mb - g.wmb - 1, &dB2, wB2);
  const bool b1 = av_b1 && !(a1 && same(dA1, wA1, dB1, wB1));
  if (b0 && av_b1 && same(dB1, wB1, dB0, wB0)) b0 = false;
  if (a0 && a1 && same(dA1, wA1, dA0, wA0)) a0 = false;
  if (b2 && ((a1 && same(dA1, wA1, dB2, wB2)) || (av_b1 && same(dB1, wB1, dB2, wB2)))) b2 = false;
  if (static_cast<int>(a0) + a1 + b0 + b1 == 4) b2 = false;
  // the list lives in registers: every index below is a compile-time one (selects over the
  // six entries), so no scratch memory
  auto push = [&](int d, const int* w) {
#pragma unroll
    for (int t = 0; t < 6; ++t) {
      if (t == nk) {
        kd[t] = d;
#pragma unroll
        for (int c = 0; c < 4; ++c) kv[t][c] = w[c];
      }
    }
    nk += nk < 6;
  };
  if (a1) push(dA1, wA1);
  if (b1) push(dB1, wB1);
  if (b0) push(dB0, wB0);
  if (a0) push(dA0, wA0);
  if (b2) push(dB2, wB2);
  if (nk < maxc && a.tdir && a.tdir[o]) {
    const int td = a.bslice ? 3 : 1;
    const int16_t* t = a.tmv + o * 4;
    const int w[4] = {t[0], t[1], a.bslice ? t[2] : 0, a.bslice ? t[3] : 0};
    push(td, w);
  }
  const int orig = nk;
  if (a.bslice && orig > 1 && orig < maxc) {
    const int l0i[12] = {0, 1, 0, 2, 1, 2, 0, 3, 1, 3, 2, 3};
    const int l1i[12] = {1, 0, 2, 0, 2, 1, 3, 0, 3, 1, 3, 2};
#pragma unroll
    for (int c = 0; c < 12; ++c) {
      if (c >= orig * (orig - 1) || nk >= maxc) break;
      const int i0 = l0i[c], i1 = l1i[c];  // compile-time after unrolling
      if ((kd[i0] & 1) && (kd[i1] & 2)) {
        const int w[4] = {kv[i0][0], kv[i0][1], kv[i1][2], kv[i1][3]};
        push(3, w);
      }
    }
  }
  {
    // zero candidates: refIdx 0, 1, .. through the active list-0 size (P), then 0
    const int z[4] = {0, 0, 0, 0};
    for (int zi = 0; nk < maxc; ++zi) push(a.bslice ? 3 : (1 | ((zi < a.nref0 ? zi : 0) << 2)), z);
  }
  if (nk > maxc) nk = maxc;
  const int cd = a.dir_in[o];
  const int16_t* cvp = a.mvb_in + o * 4;
  const int cw[4] = {cd & 1 ? cvp[0] : 0, cd & 1 ? cvp[1] : 0, cd & 2 ? cvp[2] : 0, cd & 2 ? cvp[3] : 0};
  const int lam = mb_lambda(a.qp, a.aq, slot, o);
  const int c_cur = a.cost[o];
  const int satd_cur = c_cur - lam * a.bits[o];
  const int X = r.X, Y = r.Y;
  const size_t yo = static_cast<size_t>(slot) * g.ysize(), ho = static_cast<size_t>(slot) * hp_plane_bytes(g.W, g.H);
  const uint8_t *G1 = a.bslice ? a.ref1 + yo : a.ref0 + yo, *H1 = a.bslice ? a.hp1 + ho : a.hp0 + ho;
  uint32_t src[4];
  load_src4(g, r, a.src_y, src);
  int best = c_cur, bbits = a.bits[o], bj = -1;
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    if (j >= nk) break;
    bool dup = false;  // the same motion earlier in the list: never cheaper
#pragma unroll
    for (int i = 0; i < j; ++i) dup = dup || same(kd[i], kv[i], kd[j], kv[j]);
    if (dup) continue;
    int sat = satd_cur;
    if (!same(kd[j], kv[j], cd, cw)) {
      uint32_t pw[4];
      const int r0 = (kd[j] >> 2) & 3;  // list-0 refIdx (P pictures with several list-0 pictures)
      const uint8_t *G0 = l0_ref(a, r0) + yo, *H0 = l0_hp(a, r0) + ho;
#pragma unroll
      for (int y = 0; y < 4; ++y)
        pw[y] = mc4_b(a, G0, H0, G1, H1, X, Y + y, kd[j] & 3, kv[j][0], kv[j][1], kv[j][2], kv[j][3]);
      sat = row_satd(src, pw);
    }
    const int nb = 1 + (maxc > 1 ? min(j + 1, maxc - 1) : 0);  // merge_flag + truncated-unary merge_idx
    const int cst = sat + lam * nb;
    if (cst < best) {
      best = cst;
      bbits = nb;
      bj = j;
    }
  }
  if (lane == 0) {
    int16_t* m = a.mvb_out + o * 4;
    if (a.chg_out) {  // the motion (not just its cost) differs from the pass's input
      bool moved = false;
#pragma unroll
      for (int t = 0; t < 6; ++t)
        if (t == bj) moved = !same(kd[t], kv[t], cd, cw);
      a.chg_out[o] = moved;
    }
    if (bj >= 0) {
      int bd = 0, bw[4] = {0, 0, 0, 0};
#pragma unroll
      for (int t = 0; t < 6; ++t) {
        if (t == bj) {
          bd = kd[t];
#pragma unroll
          for (int c = 0; c < 4; ++c) bw[c] = kv[t][c];
        }
      }
      for (int c = 0; c < 4; ++c) m[c] = static_cast<int16_t>(bw[c]);
      a.dir_out[o] = static_cast<uint8_t>(bd);
    } else {
      for (int c = 0; c < 4; ++c) m[c] = cvp[c];
      a.dir_out[o] = static_cast<uint8_t>(cd);
    }
    a.cost[o] = best;
    a.bits[o] = bbits;
  }
}

}  // namespace gpu
}  // namespace mivc

using namespace mivc::gpu;

extern "C" void mivc_launch_hevc_merge_refine(int B, int wmb, int hmb, const uint8_t* src_y, const uint8_t* ref,
                                              const uint8_t* hp, const int16_t* mv_in, int16_t* mv_out, int* cost,
                                              const int16_t* pm, const int* qp, const int8_t* aq, void* stream,
                                              int ctu64, int slices) {
  MergeRefineArgs a;
  a.ctu_shift = ctu64 ? 2 : 1;
  a.slices = slices;
  a.g = Geom{B, wmb, hmb, wmb * 16, hmb * 16};
  a.src_y = src_y;
  a.ref = ref;
  a.hp = hp;
  a.mv_in = mv_in;
  a.mv_out = mv_out;
  a.cost = cost;
  a.pm = pm;
  a.qp = qp;
  a.aq = aq;
  hipLaunchKernelGGL(hevc_merge_refine, dim3(mb_row_grid(wmb * hmb), B), dim3(64), 0,
                     static_cast<hipStream_t>(stream), a);
}

extern "C" void mivc_launch_hevc_b(int mode, int B, int wmb, int hmb, const uint8_t* src_y, const uint8_t* ref0,
                                   const uint8_t* ref1, const uint8_t* hp0, const uint8_t* hp1, const int16_t* mv0,
                                   const int16_t* mv1, const int* cost0, const int* cost1, const int16_t* pm0,
                                   const int16_t* pm1, const int16_t* tmv, const uint8_t* tdir, const int16_t* mvb_in,
                                   const uint8_t* dir_in, int16_t* mvb_out, uint8_t* dir_out, int* cost, int* bits,
                                   const int* qp, const int8_t* aq, void* stream, int bslice, int max_merge,
                                   int ctu64, const uint8_t* chg_in, uint8_t* chg_out, int nref0,
                                   const uint8_t* const* xref, const uint8_t* const* xhp, const int16_t* xmv,
                                   const int* xcost, const int16_t* xpm, int slices) {
  HevcBArgs a;
  a.slices = slices;
  a.nref0 = nref0 < 1 ? 1 : nref0;
  for (int r = 0; r < 3; ++r) {
    a.xref[r] = r + 1 < a.nref0 ? xref[r] : ref0;
    a.xhp[r] = r + 1 < a.nref0 ? xhp[r] : hp0;
  }
  a.xmv = xmv;
  a.xcost = xcost;
  a.xpm = xpm;
  a.chg_in = chg_in;
  a.chg_out = chg_out;
  a.ctu_shift = ctu64 ? 2 : 1;
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
  a.pm0 = pm0;
  a.pm1 = pm1;
  a.tmv = tmv;
  a.tdir = tdir;
  a.mvb_in = mvb_in;
  a.dir_in = dir_in;
  a.mvb_out = mvb_out;
  a.dir_out = dir_out;
  a.cost = cost;
  a.bits = bits;
  a.qp = qp;
  a.aq = aq;
  a.bslice = bslice;
  a.max_merge = max_merge;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 rows(mb_row_grid(wmb * hmb), B);
  if (mode == 0) hipLaunchKernelGGL(hevc_b_choose, rows, dim3(64), 0, st, a);
  else if (mode == 1) hipLaunchKernelGGL(hevc_b_merge, rows, dim3(64), 0, st, a);
  else hipLaunchKernelGGL(hevc_b_init_p, dim3((wmb * hmb + 255) / 256, B), dim3(256), 0, st, a);
}
