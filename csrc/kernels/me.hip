// Motion estimation launchers and the kernels around the search (me_search.h): the frame-level
// half-sample planes, the ungated search instances and the reference selection of P macroblocks.
#include "launch.h"
#include "me_search.h"

#include <cstdio>
#include <cstdlib>

namespace mivc {
namespace gpu {

// Frame-level half-sample planes of a reference batch (clause 8.4.2.2.1): for every
// integer position (x, y) of a (W + 8) x (H + 8) grid (margin kHpMargin, coordinates of the
// reference clamped to the picture = the normative edge extension):
//   b = half between x and x+1, h = half between y and y+1, j = centre.
// Values outside the margin equal the margin's (all 6 taps replicate), so a consumer
// clamps coordinates into [-4, W+3] x [-4, H+3] exactly.
// Grid (column quads / 64, row groups / 4, slot); a thread produces 4 columns x kHpRows
// rows, sliding a 6-row window of source rows and horizontal intermediates down.
constexpr int kHpRows = 8;

__device__ __forceinline__ void hp_load_row(const uint8_t* fr, int W, int H, int y, int x0, bool xin, int* p) {
  const uint8_t* row = fr + static_cast<size_t>(clampi(y, 0, H - 1)) * W;
  if (xin) {
    const uint32_t w0 = *reinterpret_cast<const uint32_t*>(row + x0 - 4);
    const uint32_t w1 = *reinterpret_cast<const uint32_t*>(row + x0);
    const uint32_t w2 = *reinterpret_cast<const uint32_t*>(row + x0 + 4);
    p[0] = __builtin_amdgcn_ubfe(w0, 16, 8);
    p[1] = __builtin_amdgcn_ubfe(w0, 24, 8);
#pragma unroll
    for (int k = 0; k < 4; ++k) p[2 + k] = __builtin_amdgcn_ubfe(w1, 8 * k, 8);
#pragma unroll
    for (int k = 0; k < 3; ++k) p[6 + k] = __builtin_amdgcn_ubfe(w2, 8 * k, 8);
  } else {
#pragma unroll
    for (int c = 0; c < 9; ++c) p[c] = row[clampi(x0 - 2 + c, 0, W - 1)];
  }
}

// routed (rt): the current picture of every slot coding a reference picture (SF_REF), from and
// into the pools [B, nbuf, plane]
__global__ __launch_bounds__(256) void me_halfpel_planes(const uint8_t* __restrict__ ref, int W, int H,
                                                         uint8_t* __restrict__ hp, const SlotRoute* rt, int nbuf) {
  const int PW = W + 2 * kHpMargin, PH = H + 2 * kHpMargin;
  const int q = blockIdx.x * 64 + (threadIdx.x & 63);
  const int py0 = (blockIdx.y * 4 + (threadIdx.x >> 6)) * kHpRows;
  if (q >= PW / 4 || py0 >= PH) return;
  const int slot = blockIdx.z;
  if (rt && (rt[slot].kind < 0 || !(rt[slot].flags & SF_REF))) return;
  const size_t pslot = route_index(rt, nbuf, slot, RO_CUR);
  const int x0 = 4 * q - kHpMargin, y0 = py0 - kHpMargin;
  const uint8_t* fr = ref + pslot * W * H;
  const bool xin = x0 - 4 >= 0 && x0 + 8 <= W;
  // window: source rows y-2 .. y+3 (p) and their horizontal 6-tap sums (b1)
  int p[6][9], b1[6][4];
#pragma unroll
  for (int r = 0; r < 5; ++r) {
    hp_load_row(fr, W, H, y0 - 2 + r, x0, xin, p[r + 1]);
#pragma unroll
    for (int k = 0; k < 4; ++k)
      b1[r + 1][k] = h264::tap6(p[r + 1][k], p[r + 1][k + 1], p[r + 1][k + 2], p[r + 1][k + 3], p[r + 1][k + 4],
                                p[r + 1][k + 5]);
  }
  const size_t plane = static_cast<size_t>(PW) * PH;
  uint8_t* o = hp + pslot * 3 * plane + static_cast<size_t>(py0) * PW + 4 * q;
#pragma unroll
  for (int t = 0; t < kHpRows; ++t) {
#pragma unroll
    for (int r = 0; r < 5; ++r) {
#pragma unroll
      for (int c = 0; c < 9; ++c) p[r][c] = p[r + 1][c];
#pragma unroll
      for (int k = 0; k < 4; ++k) b1[r][k] = b1[r + 1][k];
    }
    hp_load_row(fr, W, H, y0 + t + 3, x0, xin, p[5]);
#pragma unroll
    for (int k = 0; k < 4; ++k)
      b1[5][k] = h264::tap6(p[5][k], p[5][k + 1], p[5][k + 2], p[5][k + 3], p[5][k + 4], p[5][k + 5]);
    int bv[4], hv[4], jv[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      bv[k] = h264::clip1((b1[2][k] + 16) >> 5);
      hv[k] = h264::clip1((h264::tap6(p[0][k + 2], p[1][k + 2], p[2][k + 2], p[3][k + 2], p[4][k + 2],
                                      p[5][k + 2]) + 16) >> 5);
      jv[k] = h264::clip1((h264::tap6(b1[0][k], b1[1][k], b1[2][k], b1[3][k], b1[4][k], b1[5][k]) + 512) >> 10);
    }
    // byte packing through v_perm: a shift/or packing of clip((x + r) >> n) values gets
    // selected to gfx950's v_ashr_pk_u8_i32, whose high half the backend assumes is zero
    // (it is not): bytes 2-3 came out 255 on some inputs (test_me_halfpel_planes_match_numpy)
    if (py0 + t < PH) {
      *reinterpret_cast<uint32_t*>(o) = pack4_u8(bv);
      *reinterpret_cast<uint32_t*>(o + plane) = pack4_u8(hv);
      *reinterpret_cast<uint32_t*>(o + 2 * plane) = pack4_u8(jv);
    }
    o += PW;
  }
}

// Reference selection of P macroblocks (x264 --ref N): the list-0[0] decision (16x16 search,
// P_Skip-aware refinement and 8x8 partitions: mv / mv8 / cost / pred) against the 16x16
// searches of RefPicList0[1 .. nref-1]; cost + lambda * ref_idx bits (CABAC unary: about 1,
// 3, 4, 5 bits).  A farther picture that wins overwrites the decision with its vector (one
// partition), cost and luma prediction and records its index in mref.  A lane per MB decides
// (a wave per 64 MBs of a slot); the wave then copies the winners' predictions, 64 lanes each.
struct RefSelArgs {
  Geom g;
  int nref;
  int16_t* mv;                 // [B, nmb, 2]
  int16_t* mv8;                // [B, nmb, 4, 2] (nullable)
  int* cost;                   // [B, nmb]
  uint8_t* pred;               // [B, nmb, 256]
  const int16_t* xmv;          // [nref - 1, B, nmb, 2]
  const int* xcost;            // [nref - 1, B, nmb] (kNoCost: not searched)
  const uint8_t* xpred;        // [nref - 1, B, nmb, 256]
  int8_t* mref;                // [B, nmb]
  const int* qp;               // [B]
  const int8_t* aq;            // [B, nmb] (nullable)
  const SlotRoute* rt;         // routed: P slots only, each with its own active list-0 size
};

__global__ __launch_bounds__(64) void me_ref_select(RefSelArgs a) {
  const int nmb = a.g.nmb();
  const int mb0 = blockIdx.x * 64, slot = blockIdx.y, lane = threadIdx.x;
  if (!route_active(a.rt, slot, SK_P)) return;
  const int nref = a.rt ? min(a.nref, static_cast<int>(a.rt[slot].n0)) : a.nref;
  const size_t o0 = static_cast<size_t>(slot) * nmb + mb0;
  const size_t plane = static_cast<size_t>(a.g.B) * nmb;
  int bk = 0;
  if (mb0 + lane < nmb) {
    const size_t o = o0 + lane;
    const int qp = clampi(a.qp[slot] + (a.aq ? a.aq[o] : 0), 0, 51);
    const int lambda = h264::kLambda[qp];
    int best = a.cost[o] + lambda, bc = 0;
    for (int k = 1; k < nref; ++k) {
      const int c = a.xcost[(k - 1) * plane + o];
      if (c >= kNoCost) continue;
      const int ck = c + lambda * (k + 2);
      if (ck < best) {
        best = ck;
        bk = k;
        bc = c;
      }
    }
    if (bk > 0) {
      const size_t xo = (bk - 1) * plane + o;
      const int16_t vx = a.xmv[xo * 2], vy = a.xmv[xo * 2 + 1];
      a.mv[o * 2] = vx;
      a.mv[o * 2 + 1] = vy;
      if (a.mv8) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          a.mv8[o * 8 + q * 2] = vx;
          a.mv8[o * 8 + q * 2 + 1] = vy;
        }
      }
      a.cost[o] = bc;
    }
    a.mref[o] = static_cast<int8_t>(bk);
  }
  unsigned long long win = __ballot(bk > 0);
  while (win) {  // wave-uniform: the winners' predictions, 256 bytes each
    const int i = __builtin_ctzll(win);
    win &= win - 1;
    const size_t o = o0 + i;
    const size_t xo = (__builtin_amdgcn_readlane(bk, i) - 1) * plane + o;
    reinterpret_cast<uint32_t*>(a.pred + o * 256)[lane] = reinterpret_cast<const uint32_t*>(a.xpred + xo * 256)[lane];
  }
}

#ifdef MIVC_ME_PROFILE
extern "C" void mivc_me_prof_read(unsigned long long* out) {
  hipMemcpyFromSymbol(out, HIP_SYMBOL(g_me_prof), sizeof(unsigned long long) * 64 * 12);
}
#endif

}  // namespace gpu
}  // namespace mivc

using namespace mivc::gpu;

// b / h / j planes of B reference pictures into hp ([B, 3, H + 8, W + 8], margin 4)
// b / h / j planes of B reference pictures into hp ([B, 3, H + 8, W + 8], margin 4)
extern "C" void mivc_launch_me_halfpel(int B, int W, int H, const uint8_t* ref_y, uint8_t* hp, void* stream,
                                       const void* route, int nbuf) {
  const int PW = W + 2 * kHpMargin, PH = H + 2 * kHpMargin;
  const dim3 grid((PW / 4 + 63) / 64, (PH + 4 * kHpRows - 1) / (4 * kHpRows), B);
  hipLaunchKernelGGL(me_halfpel_planes, grid, dim3(256), 0, static_cast<hipStream_t>(stream), ref_y, W, H, hp,
                     static_cast<const SlotRoute*>(route), nbuf);
}

extern "C" void mivc_launch_me(int B, int wmb, int hmb, const uint8_t* src_y, const uint8_t* ref_y,
                               const int16_t* pred_mv, int16_t* out_mv, int* out_cost, uint8_t* out_pred,
                               int* out_intra_cost, const int* qp, int range, int subpel, uint8_t* hp_buf,
                               const int8_t* aq, int planes_ready, int early_sad, void* stream,
                               const int* gate_cost, int gate_thresh, const int16_t* cost_mv, const void* route,
                               int nbuf, int role, int want, const int16_t* seed_mv) {
  // hp_buf: caller-owned [B, 3, H + 8, W + 8] (+64 bytes slack) half-sample plane scratch,
  // resident across frames; nullptr -> stream-ordered scratch for this call only.
  // planes_ready: hp_buf already holds ref_y's planes (an anchor's planes are built once
  // and shared by the P picture and the B pictures that reference it).
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int W = wmb * 16, H = hmb * 16;
  uint8_t* hp = hp_buf;
  if (!hp) {
    const size_t hp_bytes = static_cast<size_t>(B) * 3 * (W + 2 * kHpMargin) * (H + 2 * kHpMargin) + 64;
    keep_async_pool();
    if (hipMallocAsync(reinterpret_cast<void**>(&hp), hp_bytes, s) != hipSuccess) {
      fprintf(stderr, "mivc_launch_me: hipMallocAsync(%zu) failed\n", hp_bytes);
      abort();
    }
  }
  if (route && !(planes_ready && hp_buf)) {
    fprintf(stderr, "mivc_launch_me: a routed search needs the resident half-sample pool\n");
    abort();
  }
  // the search reads a vector pair as one dword
  if ((reinterpret_cast<uintptr_t>(pred_mv) | reinterpret_cast<uintptr_t>(cost_mv) | reinterpret_cast<uintptr_t>(seed_mv)) & 3) {
    fprintf(stderr, "mivc_launch_me: pred_mv / cost_mv / seed_mv must be 4-byte aligned\n");
    abort();
  }
  if (!(planes_ready && hp_buf)) mivc_launch_me_halfpel(B, W, H, ref_y, hp, stream, nullptr, 0);
  MeArgs a;
  a.g = Geom{B, wmb, hmb, W, H};
  a.src_y = src_y;
  a.ref_y = ref_y;
  a.pred_mv = pred_mv;
  a.out_mv = out_mv;
  a.out_cost = out_cost;
  a.out_pred = out_pred;
  a.out_intra_cost = out_intra_cost;
  a.qp = qp;
  a.range = range < kMaxR ? range : kMaxR;
  a.subpel = subpel;
  a.hp = hp;
  a.aq = aq;
  a.early_sad = early_sad;
  a.gate_cost = gate_cost;
  a.gate_thresh = gate_thresh;
  a.cost_mv = cost_mv;
  a.rt = static_cast<const SlotRoute*>(route);
  a.nbuf = nbuf;
  a.role = role;
  a.want = want;
  a.seed_mv = seed_mv;
  // a gate leaves few MBs to search: a wave per run of kGateSpan MBs instead of one per MB
  if (gate_cost) launch_me_gated(a, s);
  else if (a.range <= 8) hipLaunchKernelGGL((me_p16x16<8, 1>), dim3(wmb * hmb, B), dim3(64), 0, s, a);
  else hipLaunchKernelGGL((me_p16x16<kMaxR, 1>), dim3(wmb * hmb, B), dim3(64), 0, s, a);
  if (!hp_buf) (void)hipFreeAsync(hp, s);
}

extern "C" void mivc_launch_me_ref_select(int B, int wmb, int hmb, int nref, int16_t* mv, int16_t* mv8, int* cost,
                                          uint8_t* pred, const int16_t* xmv, const int* xcost, const uint8_t* xpred,
                                          int8_t* mref, const int* qp, const int8_t* aq, void* stream,
                                          const void* route) {
  RefSelArgs a;
  a.rt = static_cast<const SlotRoute*>(route);
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
  a.qp = qp;
  a.aq = aq;
  hipLaunchKernelGGL(me_ref_select, dim3((wmb * hmb + 63) / 64, B), dim3(64), 0, static_cast<hipStream_t>(stream), a);
}

