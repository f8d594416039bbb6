// H.264 P pictures, mixed references per 8x8 partition (x264 --mixed-refs): p_mixed_refs, the
// reference selection of a P macroblock with a third candidate beside me_ref_select's two
// (me.hip).  It runs in place of me_ref_select, after p_part8x8 and the 16x16 searches of the
// farther list-0 pictures, and decides between
//   (a) the list-0[0] decision as it stands (mv / mv8 / cost / pred): cost + lambda;
//   (b) farther picture k as one 16x16 partition: xcost[k - 1] + lambda * (k + 2);
//   (c) a reference per 8x8 quadrant.
// (a) against (b) is me_ref_select's choice, statement for statement.  (c) is priced for an MB
// that had at least one farther picture searched (it passed the search gate) and whose list-0[0]
// SATD, the sum of its quadrants' SATDs at mv8 against src0, is above min_satd:
//   * quadrant q on reference 0 keeps mv8[q]: SATD against src0 (the inverse-weighted source
//     when RefPicList0[0] is weighted) + lambda * (mvd bits + 1);
//   * on a searched picture k >= 1 it searches four candidates -- xmv[k - 1], mv8[q] and the
//     MB's vector scaled by the distance ratio, zero -- then a half- and a quarter-sample ring,
//     as p_part8x8 does: SATD against src + lambda * (mvd bits + k + 2);
//   * the quadrant takes the cheapest, the nearer picture on a tie; the MB costs their sum +
//     lambda * overhead.
// The mvd bits are an estimate: every quadrant is priced against one vector pm per MB (scaled by
// the distance ratio for a farther picture), where the writer codes the exact predictor of clause
// 8.4.1.3 from the final records.  The encoder passes as pm the vectors the farther searches were
// priced against, which are the MBs' own final 16x16 list-0[0] vectors -- not the predictor
// p_part8x8 priced its split against, so a reference-0 quadrant is priced differently here than
// in cost.  For that reason (c) counts only when at least one quadrant leaves reference 0 (four
// quadrants on reference 0 are p_part8x8's business, whatever their vectors) and its quadrants
// do not share one (reference, vector); and it has to beat the better of (a) and (b) strictly.
// Scaling is integer: (s * v + 128) >> 8 with s in 1/256 units, clamped like every vector here
// to [-2048, 2047] x [-512, 511].
//
// A wave per run of 64 MBs of a slot (me_ref_select's grid): a lane per MB decides (a) / (b) and
// tests whether a farther picture was searched, the wave then prices (c) for those MBs in turn
// in p_part8x8's layout -- lane = quadrant (2 bits) x 4x4 block (2 bits) x candidate (2 bits) --
// and at the end a lane per MB writes what (c) did not win, the wave copying the predictions of
// (b)'s winners.  No LDS.
#include "kcommon.h"
#include "launch.h"
#include "qpel.h"

namespace mivc {
namespace gpu {

struct PMixedArgs {
  Geom g;
  int nref;
  int16_t* mv;           // [B, nmb, 2]
  int16_t* mv8;          // [B, nmb, 4, 2]
  int* cost;             // [B, nmb]
  uint8_t* pred;         // [B, nmb, 256]
  const int16_t* xmv;    // [nref - 1, B, nmb, 2]
  const int* xcost;      // [nref - 1, B, nmb] (kNoCost: not searched)
  const uint8_t* xpred;  // [nref - 1, B, nmb, 256]
  int8_t* mref;          // [B, nmb] the reference of quadrant 0
  int8_t* mref4;         // [B, nmb, 4] the reference of every quadrant
  const int* qp;         // [B]
  const int8_t* aq;      // [B, nmb] (nullable)
  const uint8_t* src0;   // the source the list-0[0] searches saw
  const uint8_t* src;    // the source
  const uint8_t* ref;    // reference pool [B, nbuf, plane]
  const uint8_t* hp;     // its half-sample planes
  const int16_t* pm;     // [B, nmb, 2] the vector the mvds are priced against (the encoder: the MB's own 16x16 vector)
  const int16_t* scale;  // [nref - 1, B] distance of picture k over that of picture 0, 1/256 units
  int overhead;          // bits charged to (c) beyond mvds and references
  int min_satd;          // list-0[0] SATD at or below this: (c) is not priced
  const SlotRoute* rt;   // P slots only, each with its own active list-0 size
  int nbuf;
};

__device__ __forceinline__ int mixed_scale(int s, int v, int lo, int hi) { return clampi((s * v + 128) >> 8, lo, hi); }

// (c) of one MB by the whole wave: true (wave-uniform) when it wins, its outputs then written
__device__ __forceinline__ bool mixed_mb(const PMixedArgs& a, int slot, int mb, int nref, int lambda, int best, int bk,
                                         int bc) {
  const Geom& g = a.g;
  const int nmb = g.nmb(), W = g.W, H = g.H;
  int lane = threadIdx.x;
  asm volatile("" : "+v"(lane));  // keeps the lane-derived values of one MB out of the survivor loop's live set
  const int q = lane >> 4, blk = (lane >> 2) & 3, c = lane & 3;
  const size_t o = static_cast<size_t>(slot) * nmb + mb;
  const size_t plane = static_cast<size_t>(g.B) * nmb;
  const int mx = mb % g.wmb, my = mb / g.wmb;
  const int X = mx * 16 + (q & 1) * 8 + (blk & 1) * 4, Y = my * 16 + (q >> 1) * 8 + (blk >> 1) * 4;
  const size_t yo = static_cast<size_t>(slot) * g.ysize() + static_cast<size_t>(Y) * W + X;
  uint32_t srow[4];
  auto qsum = [](int s) {  // over the quadrant's four blocks
    s += __shfl_xor(s, 4, 64);
    return s + __shfl_xor(s, 8, 64);
  };
  auto qmin = [](int k) {  // over the quad's four candidates
    k = min(k, __shfl_xor(k, 1, 64));
    return min(k, __shfl_xor(k, 2, 64));
  };
  const int pmx = a.pm[o * 2], pmy = a.pm[o * 2 + 1];
  const int m16x = a.mv[o * 2], m16y = a.mv[o * 2 + 1];
  const int v0x = a.mv8[o * 8 + q * 2], v0y = a.mv8[o * 8 + q * 2 + 1];
  // reference 0 at the quadrant's vector
  int qc, qr = 0, qx = v0x, qy = v0y;
  {
    const size_t s0 = route_index(a.rt, a.nbuf, slot, RO_L0);
    const uint8_t* G0 = a.ref + s0 * g.ysize();
    const uint8_t* H0 = a.hp + s0 * hp_plane_bytes(W, H);
    uint32_t p4[4];
#pragma unroll
    for (int y = 0; y < 4; ++y) {
      srow[y] = *reinterpret_cast<const uint32_t*>(a.src0 + yo + static_cast<size_t>(y) * W);
      p4[y] = mc4(G0, H0, W, H, X, Y + y, v0x, v0y);
    }
    const int s = qsum(satd4x4_u8(srow, p4));
    qc = s + lambda * (mvbits_se(v0x - pmx) + mvbits_se(v0y - pmy) + 1);
    const int satd0 = __builtin_amdgcn_readlane(s, 0) + __builtin_amdgcn_readlane(s, 16) +
                      __builtin_amdgcn_readlane(s, 32) + __builtin_amdgcn_readlane(s, 48);
    if (satd0 <= a.min_satd) return false;
  }
#pragma unroll
  for (int y = 0; y < 4; ++y) srow[y] = *reinterpret_cast<const uint32_t*>(a.src + yo + static_cast<size_t>(y) * W);
  for (int k = 1; k < nref; ++k) {
    const size_t xo = (k - 1) * plane + o;
    if (__builtin_amdgcn_readfirstlane(a.xcost[xo]) >= kNoCost) continue;  // wave-uniform
    const int sc = a.scale[(k - 1) * g.B + slot];
    const size_t sk = route_index(a.rt, a.nbuf, slot, RO_L0 + k);
    const uint8_t* Gk = a.ref + sk * g.ysize();
    const uint8_t* Hk = a.hp + sk * hp_plane_bytes(W, H);
    const int spx = mixed_scale(sc, pmx, -2048, 2047), spy = mixed_scale(sc, pmy, -512, 511);
    auto price = [&](int x, int y) -> int {
      uint32_t p4[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) p4[r] = mc4(Gk, Hk, W, H, X, Y + r, x, y);
      return qsum(satd4x4_u8(srow, p4)) + lambda * (mvbits_se(x - spx) + mvbits_se(y - spy) + k + 2);
    };
    // the candidates, one per lane of the quad
    const int fx = a.xmv[xo * 2], fy = a.xmv[xo * 2 + 1];
    const int ix = c == 0 ? fx : (c == 1 ? mixed_scale(sc, v0x, -2048, 2047) : (c == 2 ? mixed_scale(sc, m16x, -2048, 2047) : 0));
    const int iy = c == 0 ? fy : (c == 1 ? mixed_scale(sc, v0y, -512, 511) : (c == 2 ? mixed_scale(sc, m16y, -512, 511) : 0));
    const int cx = clampi(ix, -2048, 2047), cy = clampi(iy, -512, 511);
    const int key = qmin((price(cx, cy) << 2) | c);
    const int wl = (lane & ~3) | (key & 3);
    int kx = __shfl(cx, wl, 64), ky = __shfl(cy, wl, 64), kc = key >> 2;
    // half- then quarter-sample ring around the best
#pragma unroll
    for (int step = 2; step >= 1; --step) {
      const int ox = kx, oy = ky;
      int kbest = 0x7FFFFFFF;
#pragma unroll
      for (int it = 0; it < 2; ++it) {
        const int i = it * 4 + c;  // 0..7: the ring without its centre
        const int idx = i < 4 ? i : i + 1;
        const int x = clampi(ox + (idx % 3 - 1) * step, -2048, 2047), y = clampi(oy + (idx / 3 - 1) * step, -512, 511);
        kbest = min(kbest, qmin((price(x, y) << 3) | i));
      }
      if ((kbest >> 3) < kc) {
        kc = kbest >> 3;
        const int i = kbest & 7, idx = i < 4 ? i : i + 1;
        kx = clampi(ox + (idx % 3 - 1) * step, -2048, 2047);
        ky = clampi(oy + (idx / 3 - 1) * step, -512, 511);
      }
    }
    if (kc < qc) {  // the nearer picture keeps a tie
      qc = kc;
      qr = k;
      qx = kx;
      qy = ky;
    }
  }
  // every lane: the four quadrants' choices (uniform per 16 lanes)
  int rx[4], ry[4], rr[4], costc = lambda * a.overhead;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    rx[k] = __builtin_amdgcn_readlane(qx, 16 * k);
    ry[k] = __builtin_amdgcn_readlane(qy, 16 * k);
    rr[k] = __builtin_amdgcn_readlane(qr, 16 * k);
    costc += __builtin_amdgcn_readlane(qc, 16 * k);
  }
  bool same = true;
#pragma unroll
  for (int k = 1; k < 4; ++k) same = same && rx[k] == rx[0] && ry[k] == ry[0] && rr[k] == rr[0];
  if (same || (rr[0] | rr[1] | rr[2] | rr[3]) == 0 || !(costc < best)) return false;
  if (qr > 0) {
    // lane (q, blk, c) rewrites row c of its block with the farther picture's prediction
    const size_t sk = route_index(a.rt, a.nbuf, slot, RO_L0 + qr);
    const uint32_t p = mc4(a.ref + sk * g.ysize(), a.hp + sk * hp_plane_bytes(W, H), W, H, X, Y + c, qx, qy);
    const int lx = (q & 1) * 8 + (blk & 1) * 4, ly = (q >> 1) * 8 + (blk >> 1) * 4 + c;
    *reinterpret_cast<uint32_t*>(a.pred + o * 256 + ly * 16 + lx) = p;
  }
  if (lane == 0) {
    auto w = [](int x, int y) { return (static_cast<uint32_t>(x) & 0xFFFFu) | (static_cast<uint32_t>(y) << 16); };
    *reinterpret_cast<uint4*>(a.mv8 + o * 8) = make_uint4(w(rx[0], ry[0]), w(rx[1], ry[1]), w(rx[2], ry[2]), w(rx[3], ry[3]));
    *reinterpret_cast<uint32_t*>(a.mv + o * 2) = w(rx[0], ry[0]);
    *reinterpret_cast<uint32_t*>(a.mref4 + o * 4) = static_cast<uint32_t>(rr[0]) | (static_cast<uint32_t>(rr[1]) << 8) |
                                                    (static_cast<uint32_t>(rr[2]) << 16) | (static_cast<uint32_t>(rr[3]) << 24);
    a.mref[o] = static_cast<int8_t>(rr[0]);
    // the cost the better of (a) and (b) would have left, shifted by the gain (as p_part8x8 does)
    a.cost[o] = (bk > 0 ? bc : a.cost[o]) + costc - best;
  }
  return true;
}

__global__ __launch_bounds__(64) void p_mixed_refs(PMixedArgs a) {
  const int nmb = a.g.nmb();
  const int mb0 = blockIdx.x * 64, slot = blockIdx.y, lane = threadIdx.x;
  if (!route_active(a.rt, slot, SK_P)) return;
  const int nref = min(a.nref, static_cast<int>(a.rt[slot].n0));
  const size_t o0 = static_cast<size_t>(slot) * nmb + mb0;
  const size_t plane = static_cast<size_t>(a.g.B) * nmb;
  const bool live = mb0 + lane < nmb;
  // (a) against (b), as me_ref_select; searched: a farther picture's cost is there
  int bk = 0, bc = 0, best = 0, lambda = 0;
  bool searched = false;
  if (live) {
    const size_t o = o0 + lane;
    const int qp = clampi(a.qp[slot] + (a.aq ? a.aq[o] : 0), 0, 51);
    lambda = h264::kLambda[qp];
    best = a.cost[o] + lambda;
    for (int k = 1; k < nref; ++k) {
      const int c = a.xcost[(k - 1) * plane + o];
      if (c >= kNoCost) continue;
      searched = true;
      const int ck = c + lambda * (k + 2);
      if (ck < best) {
        best = ck;
        bk = k;
        bc = c;
      }
    }
  }
  bool mixed = false;
  unsigned long long todo = __ballot(searched);
  while (todo) {  // wave-uniform
    const int i = __builtin_ctzll(todo);
    todo &= todo - 1;
    const bool won = mixed_mb(a, slot, mb0 + i, nref, __builtin_amdgcn_readlane(lambda, i),
                              __builtin_amdgcn_readlane(best, i), __builtin_amdgcn_readlane(bk, i),
                              __builtin_amdgcn_readlane(bc, i));
    mixed = (threadIdx.x == i && won) || mixed;
  }
  if (live && !mixed) {
    const size_t o = o0 + lane;
    if (bk > 0) {
      const size_t xo = (bk - 1) * plane + o;
      const int16_t vx = a.xmv[xo * 2], vy = a.xmv[xo * 2 + 1];
      a.mv[o * 2] = vx;
      a.mv[o * 2 + 1] = vy;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        a.mv8[o * 8 + q * 2] = vx;
        a.mv8[o * 8 + q * 2 + 1] = vy;
      }
      a.cost[o] = bc;
    }
    a.mref[o] = static_cast<int8_t>(bk);
    *reinterpret_cast<uint32_t*>(a.mref4 + o * 4) = static_cast<uint32_t>(bk) * 0x01010101u;
  }
  unsigned long long win = __ballot(bk > 0 && !mixed);
  while (win) {  // wave-uniform: the predictions of (b)'s winners, 256 bytes each
    const int i = __builtin_ctzll(win);
    win &= win - 1;
    const size_t o = o0 + i;
    const size_t xo = (__builtin_amdgcn_readlane(bk, i) - 1) * plane + o;
    reinterpret_cast<uint32_t*>(a.pred + o * 256)[lane] = reinterpret_cast<const uint32_t*>(a.xpred + xo * 256)[lane];
  }
}

}  // namespace gpu
}  // namespace mivc

using namespace mivc::gpu;

extern "C" void mivc_launch_p_mixed_refs(int B, int wmb, int hmb, int nref, int16_t* mv, int16_t* mv8, int* cost,
                                         uint8_t* pred, const int16_t* xmv, const int* xcost, const uint8_t* xpred,
                                         int8_t* mref, int8_t* mref4, const int* qp, const int8_t* aq,
                                         const uint8_t* src0, const uint8_t* src, const uint8_t* ref, const uint8_t* hp,
                                         const int16_t* pm, const int16_t* scale, int overhead, int min_satd,
                                         void* stream, const void* route, int nbuf) {
  PMixedArgs a;
  a.g = Geom{B, wmb, hmb, wmb * 16, hmb * 16};
  a.nref = nref;
  a.mv = mv;
  a.mv8 = mv8;
  a.cost = cost;
  a.pred = pred;
  a.xmv = xmv;
  a.xcost = xcost;
  a.xpred = xpred;
  a.mref = mref;
  a.mref4 = mref4;
  a.qp = qp;
  a.aq = aq;
  a.src0 = src0;
  a.src = src;
  a.ref = ref;
  a.hp = hp;
  a.pm = pm;
  a.scale = scale;
  a.overhead = overhead;
  a.min_satd = min_satd;
  a.rt = static_cast<const SlotRoute*>(route);
  a.nbuf = nbuf;
  hipLaunchKernelGGL(p_mixed_refs, dim3((wmb * hmb + 63) / 64, B), dim3(64), 0, static_cast<hipStream_t>(stream), a);
}
