// Adaptive quantisation for the H.264 encoder (SURVEY.md K-C11, x264 --aq-mode 1, the
// libx264 default of the reference's "264" preset, server.go:69-70).
//
//   h264_aq_offsets   per-MB QP offsets from the AC energy of the source MB:
//                     energy = var(Y 16x16) + var(Cb 8x8) + var(Cr 8x8) (sum of squares minus
//                     squared sum / n, x264 ac_energy_var), offset = round(strength * 1.0397 *
//                     (log2(energy) - 14.427)), the x264 formula for 8-bit video.
//                     (+ the MB-tree offset of the MB when given, mbtree.hip)
//   prep_aq_rows      the same offsets written while the source picture is padded to the coded
//                     size (frame_prep.hip's copy and h264_aq_offsets in one pass: the source
//                     is read once instead of read, written and read again)
//   h264_aq_offsets<true>, prep_aq_rows<true>
//                     x264 --aq-mode 2 / 3 (auto-variance, aq_auto.h): the same two passes over
//                     the source storing each MB's term a = (energy + 1)^(1/8) as float32
//   h264_aq_auto_finish  one workgroup per slot that sums the terms of its picture in a fixed
//                     order and writes the offsets (+ MB-tree, rounding and clamp as above)
//   h264_qp_flags     per MB: does it carry mb_qp_delta (coded residual, or Intra16x16)?
//                     (luma from the encoder's non-zero flags, which hold for every MB kind
//                     but Intra16x16, whose flag is set regardless)
//   h264_qp_fixup     an MB without mb_qp_delta inherits QP_pred (the QP of the previous MB
//                     in decoding order, the slice QP for the first): clause 7.4.5.  Its
//                     decision record gets that QP so that deblocking (which reads QP_Y of
//                     every MB) matches a decoder.  Per slot: segmented scan over raster order.
#include <cmath>

#include "aq_auto.h"
#include "kcommon.h"
#include "launch.h"

namespace mivc {
namespace gpu {

using h264::MbHeader;

// The AC energy of one MB from its sample sums and sums of squares (luma 256, Cb and Cr 64
// samples each).
__device__ __forceinline__ uint32_t aq_energy(int s, int ss, int cb_s, int cb_ss, int cr_s, int cr_ss) {
  // the squared luma sum exceeds INT_MAX once the MB mean passes 181: unsigned products
  const uint32_t us = static_cast<uint32_t>(s);
  return (static_cast<uint32_t>(ss) - ((us * us) >> 8)) + static_cast<uint32_t>(cb_ss - ((cb_s * cb_s) >> 6)) +
         static_cast<uint32_t>(cr_ss - ((cr_s * cr_s) >> 6));
}

// The offset of one MB from those sums; `extra` (nullable): the MB-tree offset at extra[xi],
// added before rounding.
__device__ __forceinline__ int8_t aq_offset(int s, int ss, int cb_s, int cb_ss, int cr_s, int cr_ss, float strength,
                                            const float* extra, long long xi) {
  const uint32_t e = aq_energy(s, ss, cb_s, cb_ss, cr_s, cr_ss);
  float adj = strength * 1.0397f * (log2f(static_cast<float>(e > 1u ? e : 1u)) - 14.427f);
  if (extra) adj += extra[xi];  // MB-tree offset of this frame
  return static_cast<int8_t>(clampi(static_cast<int>(rintf(adj)), -24, 24));
}

// 16 lanes per MB (4 MBs per wave, 16 per 256-thread workgroup): lane l of a group sums
// luma row l (4 dwords) and, for l < 8 Cb row l / for l >= 8 Cr row l - 8 (2 dwords); the
// group reductions are DPP row sums.  A workgroup walks kAqSpan groups of 16 MBs (one launch
// of ~nmb / 16 tiny workgroups per slot was dispatch-bound: 0.56 TB/s).
// kTerm: the auto-variance term pass (h264_aq_offsets<true>) -- `terms` gets aq_term of the MB's
// energy, and strength, extra, out and rt are not read.
constexpr int kAqSpan = 8;

template <bool kTerm>
__global__ __launch_bounds__(256) void h264_aq_offsets(Geom g, const uint8_t* __restrict__ sy,
                                                       const uint8_t* __restrict__ su, const uint8_t* __restrict__ sv,
                                                       float strength, const float* __restrict__ extra,
                                                       long long extra_stride, int8_t* __restrict__ out,
                                                       const SlotRoute* rt, float* __restrict__ terms) {
  const int l = lane_id() & 15;
  const int nmb = g.nmb();
  const int slot = blockIdx.y;
  // routed: `extra` is the batch's [B, F, nmb] MB-tree table; a slot coding a reference
  // picture takes the row of its display index, other pictures get variance AQ only
  if (!kTerm && extra && rt) {
    const SlotRoute& r = rt[slot];
    extra = (r.kind >= 0 && r.disp >= 0 && (r.flags & SF_REF)) ? extra + static_cast<size_t>(r.disp) * nmb : nullptr;
  }
  for (int it = 0; it < kAqSpan; ++it) {
  const int mb = (blockIdx.x * kAqSpan + it) * 16 + (threadIdx.x >> 4);
  if ((blockIdx.x * kAqSpan + it) * 16 >= nmb) break;  // (uniform)
  const bool live = mb < nmb;
  const int mbc = live ? mb : nmb - 1;
  const int mx = mbc % g.wmb, my = mbc / g.wmb;
  const uint4 wy = *reinterpret_cast<const uint4*>(sy + slot * g.ysize() + static_cast<size_t>(my * 16 + l) * g.W + mx * 16);
  const uint8_t* c = (l < 8 ? su : sv) + slot * g.csize();
  const uint2 wc = *reinterpret_cast<const uint2*>(c + static_cast<size_t>(my * 8 + (l & 7)) * g.cw() + mx * 8);
  int s = 0, ss = 0, cs = 0, css = 0;
  const uint32_t ly[4] = {wy.x, wy.y, wy.z, wy.w}, lc[2] = {wc.x, wc.y};
#pragma unroll
  for (int w = 0; w < 4; ++w)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int p = __builtin_amdgcn_ubfe(ly[w], 8 * k, 8);
      s += p;
      ss += p * p;
    }
#pragma unroll
  for (int w = 0; w < 2; ++w)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int q = __builtin_amdgcn_ubfe(lc[w], 8 * k, 8);
      cs += q;
      css += q * q;
    }
  // Cb in lanes 0..7, Cr in 8..15 of the group: reduce each half-row separately
  const int cb_s = sum8(cs), cb_ss = sum8(css);
  s = sum16(s);
  ss = sum16(ss);
  const int cr_s = __shfl(cb_s, (lane_id() & ~15) + 8, 64), cr_ss = __shfl(cb_ss, (lane_id() & ~15) + 8, 64);
  if (live && l == 0) {
    if constexpr (kTerm)
      terms[static_cast<size_t>(slot) * nmb + mb] = aq_term(static_cast<float>(aq_energy(s, ss, cb_s, cb_ss, cr_s, cr_ss)));
    else
      out[static_cast<size_t>(slot) * nmb + mb] = aq_offset(s, ss, cb_s, cb_ss, cr_s, cr_ss, strength, extra, slot * extra_stride + mb);
  }
  }
}

// Padding and adaptive quantisation in one pass over the source (the fast path of
// mivc_launch_prep_aq: display width == coded width, 16-byte rows): a lane takes one MB
// column, a wave the 16 luma and 2 x 8 chroma rows of up to 64 neighbouring MBs of an MB
// row.  Every row is loaded once (rows past the display height from its last row), stored
// to the coded-size planes and summed in place, so an MB's sums live in one lane.  All
// loads of a plane are issued before its first store (16 x 16 bytes in flight per lane,
// 1 KiB contiguous per wave and row).  Offsets: aq_offset, as h264_aq_offsets; kTerm: the
// auto-variance term pass, as there.
constexpr int kPrepAqWaves = 4;  // MB-row units per workgroup

template <bool kTerm>
__global__ __launch_bounds__(64 * kPrepAqWaves) void prep_aq_rows(
    const uint8_t* __restrict__ in_y, const uint8_t* __restrict__ in_u, const uint8_t* __restrict__ in_v, int h,
    int64_t in_stride_y, int64_t in_stride_c, const int* __restrict__ fsel, int64_t fstep_y, int64_t fstep_c, Geom g,
    uint8_t* __restrict__ out_y, uint8_t* __restrict__ out_u, uint8_t* __restrict__ out_v, float strength,
    const float* __restrict__ extra, long long extra_stride, int8_t* __restrict__ out, const SlotRoute* rt,
    float* __restrict__ terms) {
  const int slot = blockIdx.y;
  const int groups = (g.wmb + 63) >> 6;  // 64-column groups of an MB row
  const int unit = blockIdx.x * kPrepAqWaves + wave_id();
  if (unit >= g.hmb * groups) return;  // (wave-uniform)
  const int my = unit / groups, mx = (unit - my * groups) * 64 + lane_id();
  if (mx >= g.wmb) return;  // no cross-lane step below
  const int nmb = g.nmb(), mb = my * g.wmb + mx;
  if (!kTerm && extra && rt) {  // as h264_aq_offsets
    const SlotRoute& r = rt[slot];
    extra = (r.kind >= 0 && r.disp >= 0 && (r.flags & SF_REF)) ? extra + static_cast<size_t>(r.disp) * nmb : nullptr;
  }
  const int64_t f = fsel ? fsel[slot] : 0;
  const int W = g.W, cw = g.cw(), hc = h >> 1;
  uint32_t s = 0, ss = 0;
  {
    const uint8_t* src = in_y + slot * in_stride_y + f * fstep_y + mx * 16;
    uint8_t* dst = out_y + slot * g.ysize() + static_cast<size_t>(my * 16) * W + mx * 16;
    uint4 v[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) v[r] = *reinterpret_cast<const uint4*>(src + static_cast<size_t>(min(my * 16 + r, h - 1)) * W);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      *reinterpret_cast<uint4*>(dst + static_cast<size_t>(r) * W) = v[r];
      const uint32_t w[4] = {v[r].x, v[r].y, v[r].z, v[r].w};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        s = __builtin_amdgcn_udot4(w[k], 0x01010101u, s, false);
        ss = __builtin_amdgcn_udot4(w[k], w[k], ss, false);
      }
    }
  }
  uint32_t cs[2] = {0, 0}, css[2] = {0, 0};
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const uint8_t* src = (c ? in_v : in_u) + slot * in_stride_c + f * fstep_c + mx * 8;
    uint8_t* dst = (c ? out_v : out_u) + slot * g.csize() + static_cast<size_t>(my * 8) * cw + mx * 8;
    uint2 v[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) v[r] = *reinterpret_cast<const uint2*>(src + static_cast<size_t>(min(my * 8 + r, hc - 1)) * cw);
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      *reinterpret_cast<uint2*>(dst + static_cast<size_t>(r) * cw) = v[r];
      cs[c] = __builtin_amdgcn_udot4(v[r].x, 0x01010101u, cs[c], false);
      cs[c] = __builtin_amdgcn_udot4(v[r].y, 0x01010101u, cs[c], false);
      css[c] = __builtin_amdgcn_udot4(v[r].x, v[r].x, css[c], false);
      css[c] = __builtin_amdgcn_udot4(v[r].y, v[r].y, css[c], false);
    }
  }
  if constexpr (kTerm)
    terms[static_cast<size_t>(slot) * nmb + mb] =
        aq_term(static_cast<float>(aq_energy(static_cast<int>(s), static_cast<int>(ss), static_cast<int>(cs[0]),
                                             static_cast<int>(css[0]), static_cast<int>(cs[1]), static_cast<int>(css[1]))));
  else
  out[static_cast<size_t>(slot) * nmb + mb] = aq_offset(static_cast<int>(s), static_cast<int>(ss), static_cast<int>(cs[0]),
                                                        static_cast<int>(css[0]), static_cast<int>(cs[1]),
                                                        static_cast<int>(css[1]), strength, extra, slot * extra_stride + mb);
}

// The finish pass of auto-variance AQ (aq_auto.h): workgroup `slot` reads the nmb terms of its
// picture twice (the second time from cache) and nothing else of the source.  extra,
// extra_stride, rt: as h264_aq_offsets.
__global__ __launch_bounds__(kAqFinishThreads) void h264_aq_auto_finish(int nmb, const float* __restrict__ terms,
                                                                        int mode, float strength,
                                                                        const float* __restrict__ extra,
                                                                        long long extra_stride,
                                                                        int8_t* __restrict__ out, const SlotRoute* rt) {
  __shared__ double red[2 * kAqFinishThreads];
  const int slot = blockIdx.x;
  if (extra && rt) {
    const SlotRoute& r = rt[slot];
    extra = (r.kind >= 0 && r.disp >= 0 && (r.flags & SF_REF)) ? extra + static_cast<size_t>(r.disp) * nmb : nullptr;
  }
  const float* t = terms + static_cast<size_t>(slot) * nmb;
  const AqAutoStats st = aq_auto_stats(t, nmb, mode, strength, red);
  for (int i = threadIdx.x; i < nmb; i += kAqFinishThreads) {
    float adj = aq_auto_adj(st, t[i]);
    if (extra) adj += extra[slot * extra_stride + i];
    out[static_cast<size_t>(slot) * nmb + i] = static_cast<int8_t>(clampi(static_cast<int>(rintf(adj)), -24, 24));
  }
}

// 16 lanes per MB (16 MBs per 256-thread workgroup).  The MB carries mb_qp_delta iff it
// is Intra16x16 or has a non-zero level (coded_block_pattern != 0): luma from the encoder's
// per-block non-zero flags (lane 9, 16 bytes), chroma AC from coefficient 1 (lanes 0..7),
// chroma DC (lane 8), the MB kind (lane 10).
// pre / rt (nullable, both or none): the byte encode_inter_mb left per MB of the slots that
// code a P or B picture this step (0 / 1: the answer for an inter MB; 2: handed to the intra
// kernels, which decide its levels later).  Only the route says whether a slot's bytes are of
// this step; an MB with 2, the other slots and launches without `pre` read the levels.
__global__ __launch_bounds__(256) void h264_qp_flags(Geom g, const MbHeader* __restrict__ hdr,
                                                     const int16_t* __restrict__ coef, const uint8_t* __restrict__ nzf,
                                                     uint8_t* __restrict__ flags, const uint8_t* __restrict__ pre,
                                                     const SlotRoute* rt) {
  const int lane = lane_id(), sub = lane & 15, grp = lane >> 4;
  const int nmb = g.nmb();
  const int mb = blockIdx.x * 16 + (threadIdx.x >> 4), slot = blockIdx.y;
  const bool live = mb < nmb;
  const size_t o = static_cast<size_t>(slot) * nmb + (live ? mb : 0);
  if (pre && rt && live && (rt[slot].kind == SK_P || rt[slot].kind == SK_B)) {
    const uint8_t p = pre[o];
    if (p < 2) {  // the MB's whole 16-lane group leaves: the ballot below is read per group
      if (sub == 0) flags[o] = p;
      return;
    }
  }
  const int16_t* c = coef + o * h264::kCoefPerMb;
  bool nz = false;
  if (live && sub < 8) {
    const uint4* p = reinterpret_cast<const uint4*>(c + h264::COEF_CHROMA_AC + sub * 16);
    const uint4 q0 = p[0], q1 = p[1];
    nz = ((q0.x & 0xFFFF0000u) | q0.y | q0.z | q0.w | q1.x | q1.y | q1.z | q1.w) != 0;  // position 0 unused
  } else if (live && sub == 8) {
    const uint4 q = *reinterpret_cast<const uint4*>(c + h264::COEF_CHROMA_DC);
    nz = (q.x | q.y | q.z | q.w) != 0;
  } else if (live && sub == 9) {
    const uint4 q = *reinterpret_cast<const uint4*>(nzf + o * 16);
    nz = (q.x | q.y | q.z | q.w) != 0;
  } else if (live && sub == 10) {
    nz = hdr[o].kind == h264::MBK_I16x16;
  }
  const uint64_t bal = __ballot(nz);
  if (live && sub == 0) flags[o] = ((bal >> (16 * grp)) & 0xFFFFu) != 0 ? 1 : 0;
}

// One workgroup per slice (slot-major, `per_slot` slices of `slice_mbs` MBs each): chunked
// segmented scan of "last MB with mb_qp_delta"; QP_pred starts from the slice QP at every
// slice's first MB (7.4.5).
__global__ __launch_bounds__(1024) void h264_qp_fixup(Geom g, MbHeader* __restrict__ hdr,
                                                      const uint8_t* __restrict__ flags, const int* __restrict__ slice_qp,
                                                      int slice_mbs, int per_slot) {
  const int slot = blockIdx.x / per_slot, sl = blockIdx.x - slot * per_slot;
  const int first = sl * slice_mbs;
  const int n = min(g.nmb() - first, slice_mbs);
  const size_t base = static_cast<size_t>(slot) * g.nmb() + first;
  __shared__ int s_last[1024];
  const int per = (n + blockDim.x - 1) / blockDim.x;
  const int i0 = threadIdx.x * per, i1 = min(n, i0 + per);
  int last = -1;
  for (int i = i0; i < i1; ++i)
    if (flags[base + i]) last = i;
  s_last[threadIdx.x] = last;
  __syncthreads();
  for (int off = 1; off < blockDim.x; off <<= 1) {  // inclusive max-scan (Hillis-Steele)
    const int v = threadIdx.x >= off ? s_last[threadIdx.x - off] : -1;
    __syncthreads();
    s_last[threadIdx.x] = max(s_last[threadIdx.x], v);
    __syncthreads();
  }
  last = threadIdx.x > 0 ? s_last[threadIdx.x - 1] : -1;
  int qp = last >= 0 ? hdr[base + last].qp : slice_qp[slot];
  for (int i = i0; i < i1; ++i) {
    if (flags[base + i]) qp = hdr[base + i].qp;
    else hdr[base + i].qp = static_cast<int8_t>(qp);
  }
}

}  // namespace gpu
}  // namespace mivc

using namespace mivc::gpu;

// extra: optional per-MB float QP offsets added before rounding (MB-tree), slot s of this
// frame at extra + s * extra_stride
extern "C" void mivc_launch_aq_offsets(int B, int wmb, int hmb, const uint8_t* sy, const uint8_t* su,
                                       const uint8_t* sv, float strength, const float* extra, long long extra_stride,
                                       int8_t* out, void* stream, const void* route) {
  const Geom g{B, wmb, hmb, wmb * 16, hmb * 16};
  hipLaunchKernelGGL(HIP_KERNEL_NAME(h264_aq_offsets<false>), dim3((wmb * hmb + 16 * kAqSpan - 1) / (16 * kAqSpan), B),
                     dim3(256), 0, static_cast<hipStream_t>(stream), g, sy, su, sv, strength, extra, extra_stride, out,
                     static_cast<const SlotRoute*>(route), static_cast<float*>(nullptr));
}

extern "C" void mivc_launch_aq_terms(int B, int wmb, int hmb, const uint8_t* sy, const uint8_t* su, const uint8_t* sv,
                                     float* terms, void* stream) {
  const Geom g{B, wmb, hmb, wmb * 16, hmb * 16};
  hipLaunchKernelGGL(HIP_KERNEL_NAME(h264_aq_offsets<true>), dim3((wmb * hmb + 16 * kAqSpan - 1) / (16 * kAqSpan), B),
                     dim3(256), 0, static_cast<hipStream_t>(stream), g, sy, su, sv, 0.0f,
                     static_cast<const float*>(nullptr), 0LL, static_cast<int8_t*>(nullptr),
                     static_cast<const SlotRoute*>(nullptr), terms);
}

// mode: 2 (auto-variance) or 3 (with the dark-scene bias); terms: [B, nmb] of a term launch
extern "C" void mivc_launch_aq_auto_finish(int B, int nmb, const float* terms, int mode, float strength,
                                           const float* extra, long long extra_stride, int8_t* out, void* stream,
                                           const void* route) {
  hipLaunchKernelGGL(h264_aq_auto_finish, dim3(B), dim3(kAqFinishThreads), 0, static_cast<hipStream_t>(stream), nmb,
                     terms, mode, strength, extra, extra_stride, out, static_cast<const SlotRoute*>(route));
}

// the shapes and pointers prep_aq_rows takes
static bool prep_aq_fast(const uint8_t* in_y, const uint8_t* in_u, const uint8_t* in_v, int w, int h,
                         int64_t in_stride_y, int64_t in_stride_c, const uint8_t* out_y, const uint8_t* out_u,
                         const uint8_t* out_v, int W, int H) {
  auto al = [](const void* p, uintptr_t n) { return reinterpret_cast<uintptr_t>(p) % n == 0; };
  const int64_t fstep_y = static_cast<int64_t>(w) * h, fstep_c = static_cast<int64_t>(w / 2) * (h / 2);
  return w == W && W % 16 == 0 && H % 16 == 0 && h % 2 == 0 && h >= 2 && h <= H && in_stride_y % 16 == 0 &&
         in_stride_c % 8 == 0 && fstep_y % 16 == 0 && fstep_c % 8 == 0 && al(in_y, 16) && al(in_u, 8) && al(in_v, 8) &&
         al(out_y, 16) && al(out_u, 8) && al(out_v, 8);
}

// Pad frame fsel[slot] (nullable: frame 0) of every slot's clip to the coded size and write its
// AQ offsets in one launch.  Returns 0 and launches nothing unless the display width is the
// coded width and every row chunk is aligned (16 bytes luma, 8 bytes chroma): the caller then
// runs mivc_launch_prep and mivc_launch_aq_offsets.
extern "C" int mivc_launch_prep_aq(const uint8_t* in_y, const uint8_t* in_u, const uint8_t* in_v, int w, int h,
                                   int64_t in_stride_y, int64_t in_stride_c, int B, uint8_t* out_y, uint8_t* out_u,
                                   uint8_t* out_v, int W, int H, const int* fsel, float strength, const float* extra,
                                   long long extra_stride, int8_t* out, void* stream, const void* route) {
  const int64_t fstep_y = static_cast<int64_t>(w) * h, fstep_c = static_cast<int64_t>(w / 2) * (h / 2);
  const bool fast = strength > 0.f && prep_aq_fast(in_y, in_u, in_v, w, h, in_stride_y, in_stride_c, out_y, out_u, out_v, W, H);
  if (!fast) return 0;
  const Geom g{B, W / 16, H / 16, W, H};
  const int units = g.hmb * ((g.wmb + 63) / 64);
  hipLaunchKernelGGL(HIP_KERNEL_NAME(prep_aq_rows<false>), dim3((units + kPrepAqWaves - 1) / kPrepAqWaves, B),
                     dim3(64 * kPrepAqWaves), 0, static_cast<hipStream_t>(stream), in_y, in_u, in_v, h, in_stride_y,
                     in_stride_c, fsel, fstep_y, fstep_c, g, out_y, out_u, out_v, strength, extra, extra_stride, out,
                     static_cast<const SlotRoute*>(route), static_cast<float*>(nullptr));
  return 1;
}

// mivc_launch_prep_aq for auto-variance AQ: the planes as there, the terms ([B, nmb] float32)
// instead of the offsets.  The same fast path and return value; the caller's other route is
// mivc_launch_prep and mivc_launch_aq_terms.
extern "C" int mivc_launch_prep_aq_terms(const uint8_t* in_y, const uint8_t* in_u, const uint8_t* in_v, int w, int h,
                                         int64_t in_stride_y, int64_t in_stride_c, int B, uint8_t* out_y,
                                         uint8_t* out_u, uint8_t* out_v, int W, int H, const int* fsel, float* terms,
                                         void* stream) {
  if (!prep_aq_fast(in_y, in_u, in_v, w, h, in_stride_y, in_stride_c, out_y, out_u, out_v, W, H)) return 0;
  const int64_t fstep_y = static_cast<int64_t>(w) * h, fstep_c = static_cast<int64_t>(w / 2) * (h / 2);
  const Geom g{B, W / 16, H / 16, W, H};
  const int units = g.hmb * ((g.wmb + 63) / 64);
  hipLaunchKernelGGL(HIP_KERNEL_NAME(prep_aq_rows<true>), dim3((units + kPrepAqWaves - 1) / kPrepAqWaves, B),
                     dim3(64 * kPrepAqWaves), 0, static_cast<hipStream_t>(stream), in_y, in_u, in_v, h, in_stride_y,
                     in_stride_c, fsel, fstep_y, fstep_c, g, out_y, out_u, out_v, 0.0f, static_cast<const float*>(nullptr),
                     0LL, static_cast<int8_t*>(nullptr), static_cast<const SlotRoute*>(nullptr), terms);
  return 1;
}

extern "C" void mivc_launch_qp_fixup(int B, int wmb, int hmb, void* hdr, const int16_t* coef, const uint8_t* nz,
                                     uint8_t* flags, const int* slice_qp, void* stream, int slice_rows,
                                     const uint8_t* pre, const void* route) {
  const Geom g{B, wmb, hmb, wmb * 16, hmb * 16};
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int rows = (slice_rows > 0 && slice_rows < hmb) ? slice_rows : hmb;
  const int per_slot = (hmb + rows - 1) / rows;
  hipLaunchKernelGGL(h264_qp_flags, dim3((wmb * hmb + 15) / 16, B), dim3(256), 0, s, g,
                     static_cast<const mivc::h264::MbHeader*>(hdr), coef, nz, flags,
                     (pre && route) ? pre : nullptr, static_cast<const SlotRoute*>(route));
  hipLaunchKernelGGL(h264_qp_fixup, dim3(B * per_slot), dim3(1024), 0, s, g, static_cast<mivc::h264::MbHeader*>(hdr),
                     flags, slice_qp, rows * wmb, per_slot);
}
