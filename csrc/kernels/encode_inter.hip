// P-macroblock mode decision + transform/quant/reconstruction, fully parallel
// over macroblocks (inter prediction depends only on the previous frame's
// deblocked reconstruction, never on neighbours in the current frame):
//   * intra-vs-inter decision from the ME cost and the open-loop Intra16x16
//     estimate (MBs that go intra are flagged for the wavefront kernel);
//   * chroma motion compensation (eighth-sample bilinear, clause 8.4.2.2.2);
//   * 4x4 forward core transform, dead-zone quantisation, x264-style coefficient
//     decimation, dequantisation and the normative inverse transform, so the
//     reconstruction written here is exactly what a decoder produces.
// SURVEY.md K-C8.  Two launches, every lane of a wave64 at work in both: luma four macroblocks
// per wave (one 16-lane row per MB, a lane per 4x4 block: encode_inter_mb), then chroma eight
// per wave (eight lanes per MB: encode_inter_chroma).
//
// This file is compiled twice.  On its own it is the default kernels and the launcher.  With
// MIVC_INTER_MIXED_UNIT defined (encode_inter_mixed.hip includes it) it is the instances for P
// pictures with a reference per 8x8 quadrant (x264 --mixed-refs): encode_inter_mb_mixed and
// encode_inter_chroma_mixed take mref4 [B, nmb, 4], p_mixed_refs' choice (h264_p_mixed.hip) --
// the explicit weight applies to the quadrants on reference 0 only, chroma block cb predicts from
// its quadrant's picture, the record takes ref[0][q] = mref4[q], and quadrants pair into P_16x8 /
// P_8x16 / P_16x16 only when vector and reference agree.  Every difference sits behind that
// macro, so the default unit's kernels are compiled from the text they always were.
#include "h264_trellis.h"
#include "launch.h"
#include "mb_row.h"

namespace mivc {
namespace gpu {

using h264::MbHeader;

struct InterArgs {
  Geom g;
  const uint8_t *src_y, *src_u, *src_v;
  const uint8_t *ref_y, *ref_u, *ref_v;
  uint8_t *rec_y, *rec_u, *rec_v;
  const uint8_t* pred_y;   // [B, nmb, 256] from ME
  const int16_t* mv;       // [B, nmb, 2]
  const int16_t* mv8;      // [B, nmb, 4, 2] per-quadrant vectors of P partitions (nullable: 16x16)
  const int* me_cost;      // [B, nmb]
  const int* intra_cost;   // [B, nmb]
  const int* qp;           // [B]
  const int8_t* aq;        // [B, nmb] adaptive-quantisation QP offsets (nullable)
  int chroma_qp_offset;
  MbHeader* hdr;           // [B, nmb]
  int16_t* coef;           // [B, nmb, 408]
  uint8_t* nz;             // [B, nmb, 16] luma nonzero flags (raster 4x4)
  uint8_t* intra_flag;     // [B, nmb]
  int* intra_count;        // [B]
  // B pictures (bmode): the motion of every MB is already in hdr (kind / ref / mv per
  // quadrant, written by b_decide); chroma predicts from ref (list 0) and / or ref1
  // (list 1), averaged for bi-prediction; pred_y is b_decide's luma prediction
  const uint8_t *ref1_u, *ref1_v;
  int bmode;
  int w1[4];               // B pictures: implicit bi-prediction weight of list 1 per refIdxL0 (32: average)
  int t8;                  // High profile: choose the 8x8 transform per MB (sa8d < satd, as x264)
  // several list-0 pictures (x264 --ref): chroma of RefPicList0[r] (entry 0 = ref_u / ref_v);
  // P pictures take r from mref (the reference selection, nullable: 0), B pictures from the
  // records b_decide wrote
  const uint8_t* refs_u[4];
  const uint8_t* refs_v[4];
  const int8_t* mref;      // [B, nmb] (P pictures)
  // explicit weighted prediction of RefPicList0[0] in P pictures (nullable): [B, 8] = luma
  // weight, offset, log2 denominator, Cb weight, offset, Cr weight, offset, chroma denominator
  const int* wp;
  // x264 --trellis 1 (its default: on the final encode of each MB): levels by a rate-distortion
  // choice instead of the dead-zone rounding (trellis_lite below); 0 = off, 1 = 4x4 luma only
  // (round 3), 2 = also the 8x8 luma blocks and the chroma AC blocks
  int trellis;
  float trellis_lambda;    // multiplier of the SSD lambda 0.85 * 2^((QP - 12) / 3)
  // routed (route.h): ref_* / refs_* / ref1_* / rec_* are pools [B, nbuf, plane]; slots coding a
  // P (bmode 0) or B (bmode 1) picture take their roles and implicit weights from SlotRoute
  const SlotRoute* rt;
  int nbuf;
  // [B, nmb] (nullable): per MB 1 = it has a luma, chroma AC or chroma DC level (it carries
  // mb_qp_delta), 0 = none, 2 = handed to the intra kernels -- what h264_qp_flags would
  // otherwise read back from the levels (aq.hip)
  uint8_t* qp_flags;
  // [B, nmb] (nullable): the CABAC non-zero block mask of every MB coded here, in
  // cabac_block_mask's layout (h264_cabac.h) -- encode_inter_mb writes the luma bits (or
  // h264::kBlockMaskIntra for an MB it hands to the intra kernels), encode_inter_chroma, next on the
  // stream, ORs in the chroma bits; cabac_mask then takes the word instead of the levels
  uint32_t* mask_pre;
};

// trellis_lite4x4 / trellis_lite8_chunk: h264_trellis.h

// clause 8.4.2.3.2 for one sample: ((p * w + 2^(d-1)) >> d) + o, clipped
__device__ __forceinline__ int wp_sample(int p, int w, int o, int d) {
  return h264::clip1((d >= 1 ? ((p * w + (1 << (d - 1))) >> d) : p * w) + o);
}


// Chroma predictions travel as pairs of 16-bit samples: a 4x4 block is pp[4][2], pp[y][0] =
// samples (x0, x1) of row y, pp[y][1] = (x2, x3).  The bilinear sum and the bi-prediction blend
// fit 16 bits (the weights sum to 64, samples are <= 255: at most 64 * 255 + 32), so they run
// two samples per instruction (v_pk_mul_lo_u16 / v_pk_mad_u16 / v_pk_lshrrev_b16).
typedef unsigned short v2u16 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ v2u16 as_v2u16(uint32_t x) { return __builtin_bit_cast(v2u16, x); }
__device__ __forceinline__ uint32_t as_u32(v2u16 x) { return __builtin_bit_cast(uint32_t, x); }
__device__ __forceinline__ v2u16 splat_u16(int v) {
  return v2u16{static_cast<unsigned short>(v), static_cast<unsigned short>(v)};
}
__device__ __forceinline__ int pair_lo(uint32_t p) { return static_cast<int>(p & 0xFFFFu); }
__device__ __forceinline__ int pair_hi(uint32_t p) { return static_cast<int>(p >> 16); }
__device__ __forceinline__ uint32_t make_pair(int lo, int hi) {  // both in [0, 65535]
  return static_cast<uint32_t>(lo) | (static_cast<uint32_t>(hi) << 16);
}
// the four samples of a row of pairs (each <= 255) as one little-endian word
__device__ __forceinline__ uint32_t pairs_to_u8x4(const uint32_t (&p)[2]) {
  return __builtin_amdgcn_perm(p[1], p[0], 0x06040200u);
}

// Eighth-sample chroma prediction (clause 8.4.2.2.2) of a 4x4 block at (px0, py0) of a
// cw x ch plane with vector (mvx, mvy) (quarter-luma = eighth-chroma units), as pairs.
__device__ __forceinline__ void chroma_mc4x4(const uint8_t* refc, int cw, int CH, int px0, int py0, int mvx, int mvy,
                                             uint32_t (&pp)[4][2]) {
  const int xf = mvx & 7, yf = mvy & 7;
  const int xi = px0 + (mvx >> 3), yi = py0 + (mvy >> 3);
  // reference samples (rows yi..yi+4, cols xi..xi+4), edge-clamped, as the pairs the sum takes:
  // ra[r] = (c0, c1), (c2, c3) and rb[r] = (c1, c2), (c3, c4)
  uint32_t ra[5][2], rb[5][2];
  if (xi >= 0 && xi + 8 <= cw && yi >= 0 && yi + 5 <= CH) {
    // bytes s .. s + 4 of an aligned dword pair (s = xi & 3), widened by v_perm (0x0c: zero)
    const uint32_t s = static_cast<uint32_t>(xi & 3) * 0x00010001u;
    const uint32_t sa0 = 0x0c010c00u + s, sa1 = 0x0c030c02u + s, sb0 = 0x0c020c01u + s, sb1 = 0x0c040c03u + s;
#pragma unroll
    for (int r = 0; r < 5; ++r) {
      const uint8_t* row = refc + static_cast<size_t>(yi + r) * cw;
      const int a = xi & ~3;
      const uint32_t w0 = *reinterpret_cast<const uint32_t*>(row + a), w1 = *reinterpret_cast<const uint32_t*>(row + a + 4);
      ra[r][0] = __builtin_amdgcn_perm(w1, w0, sa0);
      ra[r][1] = __builtin_amdgcn_perm(w1, w0, sa1);
      rb[r][0] = __builtin_amdgcn_perm(w1, w0, sb0);
      rb[r][1] = __builtin_amdgcn_perm(w1, w0, sb1);
    }
  } else {
#pragma unroll
    for (int r = 0; r < 5; ++r) {
      const uint8_t* row = refc + static_cast<size_t>(clampi(yi + r, 0, CH - 1)) * cw;
      int c[5];
#pragma unroll
      for (int i = 0; i < 5; ++i) c[i] = row[clampi(xi + i, 0, cw - 1)];
      ra[r][0] = make_pair(c[0], c[1]);
      ra[r][1] = make_pair(c[2], c[3]);
      rb[r][0] = make_pair(c[1], c[2]);
      rb[r][1] = make_pair(c[3], c[4]);
    }
  }
  const v2u16 wA = splat_u16((8 - xf) * (8 - yf)), wB = splat_u16(xf * (8 - yf)), wC = splat_u16((8 - xf) * yf),
              wD = splat_u16(xf * yf), half = splat_u16(32);
#pragma unroll
  for (int y = 0; y < 4; ++y)
#pragma unroll
    for (int h = 0; h < 2; ++h)
      pp[y][h] = as_u32((half + wA * as_v2u16(ra[y][h]) + wB * as_v2u16(rb[y][h]) + wC * as_v2u16(ra[y + 1][h]) +
                         wD * as_v2u16(rb[y + 1][h])) >> 6);
}

// 16 levels to a 16-byte aligned row of the coefficient buffer
__device__ __forceinline__ void store_levels(int16_t* dst, const int* v) {
  uint32_t w[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) w[i] = (static_cast<uint32_t>(v[2 * i]) & 0xFFFFu) | (static_cast<uint32_t>(v[2 * i + 1]) << 16);
  reinterpret_cast<uint4*>(dst)[0] = make_uint4(w[0], w[1], w[2], w[3]);
  reinterpret_cast<uint4*>(dst)[1] = make_uint4(w[4], w[5], w[6], w[7]);
}

// x264 decimate_score of a 4x4 block in scan order (start..15), branch-free: 9 if any
// |level| > 1, else the sum over non-zero levels of kTab[zeros between it and the
// previous non-zero level (or `start`)], kTab = {3, 2, 2, 1, 1, 1, 0, ...}.
__device__ __forceinline__ int decimate_score(const int* scan, int start) {
  int score = 0, last = start - 1;
  bool big = false;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    if (i < start) continue;
    const int v = scan[i];
    const bool nzv = v != 0;
    big |= v > 1 || v < -1;
    const int run = i - last - 1;
    const int t = run == 0 ? 3 : (run <= 2 ? 2 : (run <= 5 ? 1 : 0));
    score += nzv ? t : 0;
    last = nzv ? i : last;
  }
  return big ? 9 : score;
}

// 4 bytes of a reference row starting at byte x (any alignment), from an aligned dword pair
__device__ __forceinline__ uint32_t ld4(const uint8_t* row, int x) {
  const int a = x & ~3;
  const uint32_t w0 = *reinterpret_cast<const uint32_t*>(row + a), w1 = *reinterpret_cast<const uint32_t*>(row + a + 4);
  return __builtin_amdgcn_alignbyte(w1, w0, x & 3);
}

// Luma: four macroblocks per wave64, one 16-lane row each (MB 4i + q on lanes 16q .. 16q + 15,
// lane l of a row = luma4x4BlkIdx l), from the 4x4 transform to the reconstruction store:
// quantisation / trellis, decimation, the 8x8 trial (sa8d of the 16 8x8 blocks of the wave on
// the int8 matrix cores, one MFMA column each) and its decision, final levels, inverse
// transform.  Lane 0 of each row writes the MB record.  Chroma is encode_inter_chroma's: luma
// decisions never depend on it, and eight MBs' chroma fill a wave where four MBs' fill half.
// Block sums, masks and minima stay in registers: a 4x4 block's 8x8 block is its lane quad,
// its MB its DPP row, so the decimation scores, the 8x8 statistics and the keep masks are
// quad / row DPP reductions.  LDS holds only what crosses lanes irregularly:
// the packed samples of the sa8d operands (2 KiB) and the 8x8 transform buffers (4 KiB).
// With 6 KiB of LDS per wave and at most 128 VGPRs, 16 single-wave blocks still fit a CU
// (160 KiB LDS, 512 VGPRs per SIMD lane): four waves per SIMD as before
// (profiles/r5_occupancy_ab.md, profiles/inter_four_mb_per_wave.md).
// Rows move as dwords (prediction, source, reconstruction), levels as 16-byte
// stores, and the decimation score is branch-free.  Every wave_sync() sits in wave-uniform
// control flow; MBs of a wave that are dead (tail), intra-flagged or not on the 8x8 path are
// masked by per-lane predicates, never by an early exit.
#ifdef MIVC_INTER_MIXED_UNIT
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4, 8))) void encode_inter_mb_mixed(InterArgs a,
                                                                                                        const int8_t* mref4) {
#else
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4, 8))) void encode_inter_mb(InterArgs a) {
#endif
  const Geom& g = a.g;
  const int lane = threadIdx.x, q = lane >> 4, l = lane & 15;
  const int nmb = g.nmb();
  int ux, slot;
  xcd_unit_slot(ux, slot);
  if (!route_active(a.rt, slot, a.bmode ? SK_B : SK_P)) return;  // wave-uniform
  const size_t rcur = route_index(a.rt, a.nbuf, slot, RO_CUR);
  const int W = g.W;
  // the wave's first MB (always inside the picture); MB q follows it in raster order
  const int mb0 = ux * kMbsPerWave;

  // 8x8 transform path (a.t8): the luma source / prediction samples (sa8d operands) and the
  // 8x8 transform buffers (residual -> coefficients, later dequantised levels -> residual)
  __shared__ uint32_t s_px[kMbsPerWave][2][16][4];  // [MB][source / prediction][row][dword]
  __shared__ int s_d8[kMbsPerWave][4][64];          // [MB][8x8 block][raster]

  int lv[16];       // levels of this lane's block (raster; scan order of its chunk on the 8x8 path)
  int res[16];      // residual / reconstruction scratch
  uint32_t prw[4];  // prediction rows (4 bytes each)

  {
    // this row's MB (the tail's dead rows are clamped to the last MB): position, record index,
    // inter-coded here (work), QP.  With adaptive quantisation the four MBs have four QPs:
    // every lane fetches its own MB's table rows (one address, 3-dword loads) -- fewer
    // registers and instructions than four scalar rows and three-deep selects per value.
    const bool live = mb0 + q < nmb;
    const int d = live ? q : nmb - 1 - mb0;  // 0..3
    int mx = mb0 % g.wmb + d, my = mb0 / g.wmb;
#pragma unroll
    for (int i = 0; i < 3; ++i) {  // at most 3 row wraps (wmb = 1)
      const bool wrap = mx >= g.wmb;
      mx -= wrap ? g.wmb : 0;
      my += wrap ? 1 : 0;
    }
    const size_t o = static_cast<size_t>(slot) * nmb + mb0 + d;
    const bool work = live && !(a.intra_cost[o] < a.me_cost[o]);
    const int qp = clampi(a.qp[slot] + (a.aq ? a.aq[o] : 0), 0, 51);
    MbHeader* h = a.hdr + o;
    int16_t* coef = a.coef + o * h264::kCoefPerMb;
    if (live && !work && l == 0) {
      // the wavefront kernel encodes this MB closed-loop; leave a consistent placeholder
      a.intra_flag[o] = 1;
      atomicAdd(a.intra_count + slot, 1);
      h->kind = h264::MBK_I16x16;
    }
    const int X0 = mx * 16, Y0 = my * 16;
    const int lbx = (((l >> 2) & 1) * 2 + (l & 1)) * 4, lby = (((l >> 3) & 1) * 2 + ((l >> 1) & 1)) * 4;
    // this block's 8x8 block is its lane quad (b8 = l >> 2); inside it: chunk / row pair k,
    // sample offset (ox, oy)
    const int k = l & 3, ox = lbx & 4, oy = lby & 4;
    int* dd = s_d8[q][l >> 2];

    int score = 0;
    if (work) {
      // ---- residual against the ME prediction, forward transform, quantisation
      const uint8_t* srcy = a.src_y + slot * g.ysize() + static_cast<size_t>(Y0 + lby) * W + X0 + lbx;
      const uint8_t* pred = a.pred_y + o * 256 + lby * 16 + lbx;
      uint32_t sw[4];
#pragma unroll
      for (int y = 0; y < 4; ++y) {
        prw[y] = *reinterpret_cast<const uint32_t*>(pred + y * 16);
        sw[y] = *reinterpret_cast<const uint32_t*>(srcy + static_cast<size_t>(y) * W);
      }
#ifdef MIVC_INTER_MIXED_UNIT
      if (a.wp && !a.bmode && !mref4[o * 4 + (l >> 2)]) {  // weighted RefPicList0[0] prediction, this block's quadrant
#else
      if (a.wp && !a.bmode && !(a.mref && a.mref[o])) {  // weighted RefPicList0[0] prediction
#endif
        const int* wt = a.wp + slot * 8;
        const int w = wt[0], wo = wt[1], d = wt[2];
        if (w != (1 << d) || wo != 0) {
#pragma unroll
          for (int y = 0; y < 4; ++y) {
            int v4[4];
#pragma unroll
            for (int x = 0; x < 4; ++x) v4[x] = wp_sample(static_cast<int>(__builtin_amdgcn_ubfe(prw[y], 8 * x, 8)), w, wo, d);
            prw[y] = pack4_u8(v4);
          }
        }
      }
#pragma unroll
      for (int y = 0; y < 4; ++y)
#pragma unroll
        for (int x = 0; x < 4; ++x)
          res[y * 4 + x] = static_cast<int>(__builtin_amdgcn_ubfe(sw[y], 8 * x, 8)) -
                           static_cast<int>(__builtin_amdgcn_ubfe(prw[y], 8 * x, 8));
      // 4x4 transform, quantisation and decimation score (always: most MBs end here)
      h264::forward_core4x4(res);
      int mf[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) mf[c] = h264::kQuantMF[qp % 6][c];
      const int qbits = 15 + qp / 6;
      if (a.trellis) {
        trellis_lite4x4(res, lv, mf, qbits, trellis_lambda4(a.trellis_lambda, qp));
      } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) lv[r] = h264::quant_coef(res[r], mf[h264::kPosClass[r]], qbits, 11);
      }
      int scan[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) scan[i] = lv[h264::kZigzag4x4[i]];
      score = decimate_score(scan, 0);
      if (a.t8) {
        // stage this block's source and prediction rows for the 8x8 trial
#pragma unroll
        for (int y = 0; y < 4; ++y) {
          s_px[q][0][lby + y][lbx >> 2] = sw[y];
          s_px[q][1][lby + y][lbx >> 2] = prw[y];
        }
      }
    }
    // x264 decimation: an 8x8 block (the quad) scoring under 4 is dropped, an MB (the row)
    // scoring under 6 altogether; scores of dead / intra lanes are 0.  (Every cross-lane sum
    // is formed by all lanes before it is tested: inside a short-circuit && or ?: it would run
    // under a divergent mask and miss the masked lanes' terms.)
    const int score8 = sum4(score), score16 = sum16(score);
    const bool keep4 = score8 >= 4 && score16 >= 6;

    bool use8 = false, keep8 = false;  // per MB: the 8x8 transform is used; per quad: its levels stay
    uint64_t use8_wave = 0;
    if (a.t8) {
      // High profile: an MB whose 4x4 luma levels survive decimation also tries the 8x8
      // transform -- sa8d of the residual < its satd picks it (x264 analyse), and only then is it
      // transformed and quantised; MBs without luma residual keep the 4x4 flag-free coding
      // (transform_size_8x8_flag is not even coded for them).  The trial runs when any of the
      // wave's four MBs wants it (the sa8d runs on the matrix cores for all of them at once).
      wave_sync();
      const uint64_t try_wave = __ballot(keep4);
      if (try_wave) {  // wave-uniform
        const bool mine = ((try_wave >> (16 * q)) & 0xFFFFu) != 0;
        int satd = 0;
        if (mine) {
          // this 4x4 block's residual: the 8x8 transform input (s_d8) and its 4x4 satd
          int r2[16];
#pragma unroll
          for (int y = 0; y < 4; ++y) {
            const uint32_t sv = s_px[q][0][lby + y][lbx >> 2], pv = s_px[q][1][lby + y][lbx >> 2];
#pragma unroll
            for (int x = 0; x < 4; ++x) {
              r2[y * 4 + x] = static_cast<int>(__builtin_amdgcn_ubfe(sv, 8 * x, 8)) -
                              static_cast<int>(__builtin_amdgcn_ubfe(pv, 8 * x, 8));
              dd[(oy + y) * 8 + ox + x] = r2[y * 4 + x];
            }
          }
          satd = h264::satd4x4(r2);
        }
        // sa8d of the wave's 16 8x8 blocks (MFMA column 4 * MB + b8) on the int8 matrix cores:
        // vec(H8 X H8^T) = H64 vec(X) with H64 = H8 (x) H8 (Sylvester: (-1)^popcount(i & k)),
        // X = S - P split as (S - 128) - (P - 128) so both operands fit int8 (exact).  Columns
        // of MBs that are not trying hold stale samples; their sums are never read.
        const int col = l, grp = q;
        mfma_i32x4 sop, pop;
        {
          const int cm = col >> 2, b8 = col & 3, r0 = (b8 >> 1) * 8 + 2 * grp, c0 = (b8 & 1) * 2;
#pragma unroll
          for (int sp = 0; sp < 2; ++sp) {
            mfma_i32x4& op = sp ? pop : sop;
            op[0] = static_cast<int>(s_px[cm][sp][r0][c0] ^ 0x80808080u);
            op[1] = static_cast<int>(s_px[cm][sp][r0][c0 + 1] ^ 0x80808080u);
            op[2] = static_cast<int>(s_px[cm][sp][r0 + 1][c0] ^ 0x80808080u);
            op[3] = static_cast<int>(s_px[cm][sp][r0 + 1][c0 + 1] ^ 0x80808080u);
          }
        }
        // this lane's A rows: H64[16 t + col][16 grp + j] = (-1)^popcount(t & grp) H16[col][j]
        mfma_i32x4 hp, hn;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          uint32_t w = 0;
#pragma unroll
          for (int b = 0; b < 4; ++b) w |= ((__builtin_popcount(col & (4 * j + b)) & 1) ? 0xFFu : 0x01u) << (8 * b);
          hp[j] = static_cast<int>(w);
          hn[j] = static_cast<int>(w ^ 0xFEFEFEFEu);  // 0x01 <-> 0xFF: the negation
        }
        int sa = 0;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const bool neg = __builtin_popcount(t & grp) & 1;
          mfma_i32x4 d = __builtin_amdgcn_mfma_i32_16x16x64_i8(neg ? hn : hp, sop, mfma_i32x4{0, 0, 0, 0}, 0, 0, 0);
          d = __builtin_amdgcn_mfma_i32_16x16x64_i8(neg ? hp : hn, pop, d, 0, 0, 0);
          sa += abs(d[0]) + abs(d[1]) + abs(d[2]) + abs(d[3]);
        }
        sa = sum_row_groups(sa);  // |coefficients| of column col, summed over its 4 lane groups
        // the MB's sa8d: its four columns are one quad; row q takes MB q's from lane 4 q
        const int sa8d = __shfl(sum4((sa + 2) >> 2), 4 * q, 64);
        const int satd16 = sum16(satd);
        use8 = mine && sa8d < satd16;
        use8_wave = __ballot(use8);
        wave_sync();  // the residuals in s_d8 are complete
        if (use8_wave) {  // wave-uniform
          // ---- 8x8 transform: forward passes (lane k on rows / columns 2k, 2k + 1 of its
          // quad's block), quantisation of scan positions 16k .. 16k + 15 with this chunk's share
          // of x264's decimate_score64 (zero runs priced 3 / 2 / 1 / 0; 9 once any |level| > 1):
          // runs inside the chunk here, the run into its first non-zero level from the previous
          // chunks' last.  The levels replace the 4x4 ones in lv.
          if (use8) {
            dct8_pass(dd + (2 * k) * 8, 1);
            dct8_pass(dd + (2 * k + 1) * 8, 1);
          }
          wave_sync();
          if (use8) {
            dct8_pass(dd + 2 * k, 8);
            dct8_pass(dd + 2 * k + 1, 8);
          }
          wave_sync();
          const int qbits8 = 16 + qp / 6;
          const int m = qp % 6;
          if (a.trellis >= 2) {
            // x264 --trellis on the 8x8 blocks too: the dead-zone levels say which later chunks
            // keep a non-zero level, then each chunk runs the greedy choice back to front
            float z[16];
            int nzc = 0;
            if (use8) {
              const float inv = exp2f(-static_cast<float>(qbits8));
#pragma unroll
              for (int i = 0; i < 16; ++i) {
                const int pos = kZz8[k * 16 + i];
                const int mf8 = kQuant8MF[m][pos8(pos & 7, pos >> 3)];
                z[i] = static_cast<float>(dd[pos]) * static_cast<float>(mf8) * inv;
                nzc |= h264::quant_coef(dd[pos], mf8, qbits8, 11) != 0;
              }
            }
            const int nz1 = quad_bcast<1>(nzc), nz2 = quad_bcast<2>(nzc), nz3 = quad_bcast<3>(nzc);
            const bool later = (k < 1 && nz1) || (k < 2 && nz2) || (k < 3 && nz3);
            if (use8) trellis_lite8_chunk(z, lv, a.trellis_lambda * 0.136f, later);
          } else if (use8) {
#pragma unroll
            for (int i = 0; i < 16; ++i) {
              const int pos = kZz8[k * 16 + i];
              lv[i] = h264::quant_coef(dd[pos], kQuant8MF[m][pos8(pos & 7, pos >> 3)], qbits8, 11);
            }
          }
          int lastnz = -1, firstnz = -1, inner = 0, big = 0;
          if (use8) {
#pragma unroll
            for (int i = 0; i < 16; ++i) {
              const int idx = k * 16 + i;
              const int v = lv[i];
              const bool nzv = v != 0;
              big |= v > 1 || v < -1;
              const int run = idx - lastnz - 1;
              inner += (nzv && firstnz >= 0) ? (run <= 3 ? 3 : (run <= 11 ? 2 : (run <= 23 ? 1 : 0))) : 0;
              firstnz = (nzv && firstnz < 0) ? idx : firstnz;
              lastnz = nzv ? idx : lastnz;
            }
          }
          const int l0 = quad_bcast<0>(lastnz), l1 = quad_bcast<1>(lastnz), l2 = quad_bcast<2>(lastnz);
          const int prev = max(k > 0 ? l0 : -1, max(k > 1 ? l1 : -1, k > 2 ? l2 : -1));
          const int run0 = firstnz - prev - 1;
          const int sc = inner + (firstnz >= 0 ? (run0 <= 3 ? 3 : (run0 <= 11 ? 2 : (run0 <= 23 ? 1 : 0))) : 0);
          const int big8 = sum4(big), sc8 = sum4(sc);
          const int scb = big8 ? 9 : sc8;  // the 8x8 block's score, on its four lanes
          const int total8 = sum16(k == 0 ? scb : 0);
          keep8 = use8 && scb >= 4 && total8 >= 6;
        }
      }
    }

    // ---- final levels, dequantisation, inverse transform: res = this block's residual
    bool any = false;  // this block's residual is added to the prediction
    bool lnz = false;  // the 16 levels this lane stores (4x4 block / chunk of an 8x8 block) have a non-zero one
    if (use8_wave) {  // wave-uniform
      // 8x8: levels in 8x8 scan order (chunk k of the quad's block), dequantised into the
      // transform buffer, inverse 8x8 (lanes on rows / columns 2k, 2k + 1), then every lane
      // takes its 4x4 part of the residual
      if (use8) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          lv[i] = keep8 ? lv[i] : 0;
          lnz |= lv[i] != 0;
        }
        store_levels(coef + h264::COEF_LUMA + l * 16, lv);
        const int m = qp % 6, q6 = qp / 6;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int pos = kZz8[k * 16 + i];
          const int ls = 16 * kNorm8[m][pos8(pos & 7, pos >> 3)];
          const int c = lv[i];
          dd[pos] = q6 >= 6 ? (c * ls) << (q6 - 6) : (c * ls + (1 << (5 - q6))) >> (6 - q6);
        }
      }
      wave_sync();
      if (use8) {
        idct8_pass(dd + (2 * k) * 8, 1);
        idct8_pass(dd + (2 * k + 1) * 8, 1);
      }
      wave_sync();
      if (use8) {
        idct8_pass(dd + 2 * k, 8);
        idct8_pass(dd + 2 * k + 1, 8);
      }
      wave_sync();
      if (use8) {
        any = keep8;
#pragma unroll
        for (int y = 0; y < 4; ++y)
#pragma unroll
          for (int x = 0; x < 4; ++x) res[y * 4 + x] = (dd[(oy + y) * 8 + ox + x] + 32) >> 6;
      }
    }
    if (work && !use8) {
      int sv[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        sv[i] = keep4 ? lv[h264::kZigzag4x4[i]] : 0;
        any |= sv[i] != 0;
      }
      lnz = any;
      store_levels(coef + h264::COEF_LUMA + l * 16, sv);
      int dv[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) dv[c] = h264::kDequantV[qp % 6][c];
#pragma unroll
      for (int r = 0; r < 16; ++r) res[r] = keep4 ? (lv[r] * dv[h264::kPosClass[r]]) << (qp / 6) : 0;
      if (any) h264::inverse_core4x4(res);
    }
    const bool t8_coded = ((__ballot(keep8) >> (16 * q)) & 0xFFFFu) != 0;  // the MB has 8x8 levels
    if (a.qp_flags) {
      // the MB's byte from luma alone (`any` is false outside `work`); encode_inter_chroma,
      // next on the stream, raises it to 1 for an MB that has chroma levels only
      const uint64_t luma_any = __ballot(any);
      if (live && l == 0) a.qp_flags[o] = !work ? 2 : (((luma_any >> (16 * q)) & 0xFFFFu) != 0 ? 1 : 0);
    }
    if (a.mask_pre) {
      // bit l = this lane's 16 stored levels (`lnz` is false outside `work`); the ballot is
      // formed by every lane before the row's lane 0 is picked
      const uint64_t luma_nz = __ballot(lnz);
      if (live && l == 0) a.mask_pre[o] = work ? static_cast<uint32_t>((luma_nz >> (16 * q)) & 0xFFFFu) : h264::kBlockMaskIntra;
    }
    if (work) {
      uint8_t* recy = a.rec_y + rcur * g.ysize() + static_cast<size_t>(Y0 + lby) * W + X0 + lbx;
#pragma unroll
      for (int y = 0; y < 4; ++y) {
        int v4[4];
#pragma unroll
        for (int x = 0; x < 4; ++x)
          v4[x] = h264::clip1(static_cast<int>(__builtin_amdgcn_ubfe(prw[y], 8 * x, 8)) + (any ? res[y * 4 + x] : 0));
        *reinterpret_cast<uint32_t*>(recy + static_cast<size_t>(y) * W) = pack4_u8(v4);
      }
      a.nz[o * 16 + (lbx >> 2) + lby] = any;
      // luma DC (unused for inter MBs): zero
      if (l < 2) reinterpret_cast<uint4*>(coef + h264::COEF_LUMA_DC)[l] = make_uint4(0, 0, 0, 0);
      if (l == 0) {
        // ---- the MB record
        h->qp = static_cast<int8_t>(qp);
        h->i16_mode = 0;
        h->chroma_mode = 0;
        // transform_size_8x8_flag is only coded (and only matters) when luma levels exist
        h->flags = t8_coded ? h264::MBF_T8x8 : 0;
        a.intra_flag[o] = 0;
        if (!a.bmode) {  // B pictures: kind / ref / mv are b_decide's
          const int mvx = a.mv[o * 2], mvy = a.mv[o * 2 + 1];
          const uint32_t mvw = (static_cast<uint32_t>(mvx) & 0xFFFFu) | (static_cast<uint32_t>(mvy) << 16);
          uint4 q4 = make_uint4(mvw, mvw, mvw, mvw);
          if (a.mv8) q4 = *reinterpret_cast<const uint4*>(a.mv8 + o * 8);
          // quadrant vectors -> the cheapest partition shape that carries them
#ifdef MIVC_INTER_MIXED_UNIT
          const uint32_t r = *reinterpret_cast<const uint32_t*>(mref4 + o * 4);  // the four quadrants' references
          const uint32_t r0 = r & 255u, r1 = (r >> 8) & 255u, r2 = (r >> 16) & 255u, r3 = r >> 24;
          const bool top = q4.x == q4.y && r0 == r1, bottom = q4.z == q4.w && r2 == r3;
          const bool left = q4.x == q4.z && r0 == r2, right = q4.y == q4.w && r1 == r3;
          h->kind = (top && bottom) ? (left ? h264::MBK_P16x16 : h264::MBK_P16x8)
                                    : ((left && right) ? h264::MBK_P8x16 : h264::MBK_P8x8);
          uint4* mvp = reinterpret_cast<uint4*>(&h->mv[0][0][0]);  // 16-byte aligned
          mvp[0] = q4;
#else
          h->kind = (q4.x == q4.y && q4.z == q4.w) ? (q4.x == q4.z ? h264::MBK_P16x16 : h264::MBK_P16x8)
                                                   : ((q4.x == q4.z && q4.y == q4.w) ? h264::MBK_P8x16 : h264::MBK_P8x8);
          uint4* mvp = reinterpret_cast<uint4*>(&h->mv[0][0][0]);  // 16-byte aligned
          mvp[0] = q4;
          const uint32_t r = a.mref ? static_cast<uint32_t>(a.mref[o]) * 0x01010101u : 0u;
#endif
          *reinterpret_cast<uint2*>(&h->ref[0][0]) = make_uint2(r, 0xFFFFFFFFu);  // L0 ref r, L1 unused
        }
      }
    }
  }

}

// Chroma of the same MBs: eight per wave64 (MB 8i + m on lanes 8m .. 8m + 7: component
// comp = (lane >> 2) & 1, 4x4 block cb = lane & 3, so a quad is one component of one MB): motion
// compensation, transform, the 2x2 DC Hadamard, levels, reconstruction.  It takes nothing from
// encode_inter_mb but the stream order: which MBs are coded here, their vectors, references and
// QP come from the same inputs (P pictures: mv / mv8 / mref; B pictures: b_decide's records).
// The component's four DC terms and its AC decimation score are quad DPP reductions, formed
// by every lane before they are tested; dead MBs of the last wave are clamped to the last MB
// and masked, never left early.  No LDS.
#ifdef MIVC_INTER_MIXED_UNIT
__global__ __launch_bounds__(64) void encode_inter_chroma_mixed(InterArgs a, const int8_t* mref4) {
#else
__global__ __launch_bounds__(64) void encode_inter_chroma(InterArgs a) {
#endif
  const Geom& g = a.g;
  const int lane = threadIdx.x, m = lane >> 3, comp = (lane >> 2) & 1, cb = lane & 3;
  const int nmb = g.nmb();
  int ux, slot;
  xcd_unit_slot(ux, slot);
  if (!route_active(a.rt, slot, a.bmode ? SK_B : SK_P)) return;  // wave-uniform
  const size_t rcur = route_index(a.rt, a.nbuf, slot, RO_CUR);
  const int cw = g.cw(), CH = g.ch();
  const int mb0 = ux * kMbsPerChromaWave;  // always inside the picture
  const bool live = mb0 + m < nmb;
  const int dm = live ? m : nmb - 1 - mb0;  // 0..7
  int mx = mb0 % g.wmb + dm, my = mb0 / g.wmb;
  while (__ballot(mx >= g.wmb)) {  // row wraps: one at most unless the picture is under 8 MBs wide
    const bool wrap = mx >= g.wmb;
    mx -= wrap ? g.wmb : 0;
    my += wrap ? 1 : 0;
  }
  const size_t o = static_cast<size_t>(slot) * nmb + mb0 + dm;
  const bool work = live && !(a.intra_cost[o] < a.me_cost[o]);
  const int qpc = h264::chroma_qp(clampi(a.qp[slot] + (a.aq ? a.aq[o] : 0), 0, 51), a.chroma_qp_offset);
  const MbHeader* h = a.hdr + o;
  int16_t* coef = a.coef + o * h264::kCoefPerMb;
  const int cbx = (cb & 1) * 4, cby = (cb >> 1) * 4;

  int lv[16];       // AC levels of this lane's block (raster)
  int res[16];      // residual / reconstruction scratch
  uint32_t prw[4];  // prediction rows (4 bytes each)
  int mfc[3], dvc[3];
  int dc = 0, score = 0;
  if (work) {
    // ---- eighth-sample MC (clause 8.4.2.2.2) + residual + forward + AC quantisation
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      mfc[c] = h264::kQuantMF[qpc % 6][c];
      dvc[c] = h264::kDequantV[qpc % 6][c];
    }
    const uint8_t* srcc = (comp == 0 ? a.src_u : a.src_v) + slot * g.csize();
    const int px0 = mx * 8 + cbx, py0 = my * 8 + cby;
    uint32_t pp[4][2];
    if (!a.bmode) {
      // the 4x4 chroma block cb covers luma quadrant cb (its partition's vector)
      const int cmx = a.mv8 ? a.mv8[o * 8 + cb * 2] : a.mv[o * 2], cmy = a.mv8 ? a.mv8[o * 8 + cb * 2 + 1] : a.mv[o * 2 + 1];
#ifdef MIVC_INTER_MIXED_UNIT
      const int r = mref4[o * 4 + cb] & 3;
#else
      const int r = a.mref ? a.mref[o] : 0;
#endif
      chroma_mc4x4((comp == 0 ? a.refs_u[r] : a.refs_v[r]) + route_index(a.rt, a.nbuf, slot, RO_L0 + r) * g.csize(), cw,
                   CH, px0, py0, cmx, cmy, pp);
      if (a.wp && r == 0) {
        const int* wt = a.wp + slot * 8;
        const int w = wt[3 + 2 * comp], wo = wt[4 + 2 * comp], d = wt[7];
        if (w != (1 << d) || wo != 0) {
#pragma unroll
          for (int y = 0; y < 4; ++y)
#pragma unroll
            for (int hh = 0; hh < 2; ++hh)
              pp[y][hh] = make_pair(wp_sample(pair_lo(pp[y][hh]), w, wo, d), wp_sample(pair_hi(pp[y][hh]), w, wo, d));
        }
      }
    } else {
      // the 4x4 chroma block cb covers luma quadrant cb: its lists and vectors
      const int r0 = h->ref[0][cb];
      const bool u0 = r0 >= 0, u1 = h->ref[1][cb] >= 0;
      const int w1 = a.rt ? a.rt[slot].w1[r0 & 3] : a.w1[r0 & 3];
      uint32_t p1[4][2];
      if (u0) chroma_mc4x4((comp == 0 ? a.refs_u[r0 & 3] : a.refs_v[r0 & 3]) +
                               route_index(a.rt, a.nbuf, slot, RO_L0 + (r0 & 3)) * g.csize(), cw, CH, px0, py0,
                           h->mv[0][cb][0], h->mv[0][cb][1], pp);
      if (u1) chroma_mc4x4((comp == 0 ? a.ref1_u : a.ref1_v) + route_index(a.rt, a.nbuf, slot, RO_L1) * g.csize(), cw,
                           CH, px0, py0,
                           h->mv[1][cb][0], h->mv[1][cb][1], p1);
      // implicit weights (w1 = 32: the plain average).  With both weights in [0, 64] the sum
      // fits 16 bits and needs no clip, so it runs on pairs; a weight outside (the lists on one
      // side of the picture) takes the 32-bit form.  Wave-uniform: one form per wave.
      const bool bi = u0 && u1;
      if (__ballot(bi && (w1 < 0 || w1 > 64)) == 0) {
        const v2u16 k0 = splat_u16(64 - w1), k1 = splat_u16(w1), half = splat_u16(32);
#pragma unroll
        for (int y = 0; y < 4; ++y)
#pragma unroll
          for (int hh = 0; hh < 2; ++hh) {
            const uint32_t b2 = as_u32((half + as_v2u16(pp[y][hh]) * k0 + as_v2u16(p1[y][hh]) * k1) >> 6);
            pp[y][hh] = u0 ? (u1 ? b2 : pp[y][hh]) : p1[y][hh];
          }
      } else {
#pragma unroll
        for (int y = 0; y < 4; ++y)
#pragma unroll
          for (int hh = 0; hh < 2; ++hh) {
            const int lo = h264::clip1((pair_lo(pp[y][hh]) * (64 - w1) + pair_lo(p1[y][hh]) * w1 + 32) >> 6);
            const int hi = h264::clip1((pair_hi(pp[y][hh]) * (64 - w1) + pair_hi(p1[y][hh]) * w1 + 32) >> 6);
            pp[y][hh] = u0 ? (u1 ? make_pair(lo, hi) : pp[y][hh]) : p1[y][hh];
          }
      }
    }
    uint32_t sw[4];
#pragma unroll
    for (int y = 0; y < 4; ++y) sw[y] = *reinterpret_cast<const uint32_t*>(srcc + static_cast<size_t>(py0 + y) * cw + px0);
#pragma unroll
    for (int y = 0; y < 4; ++y) {
#pragma unroll
      for (int x = 0; x < 4; ++x)
        res[y * 4 + x] = static_cast<int>(__builtin_amdgcn_ubfe(sw[y], 8 * x, 8)) -
                         ((x & 1) ? pair_hi(pp[y][x >> 1]) : pair_lo(pp[y][x >> 1]));
      prw[y] = pairs_to_u8x4(pp[y]);
    }
    h264::forward_core4x4(res);
    dc = res[0];
    const int qbits = 15 + qpc / 6;
    if (a.trellis >= 2) {  // chroma AC by the same rate-distortion choice, at the chroma QP's lambda
      trellis_lite4x4(res, lv, mfc, qbits, trellis_lambda4(a.trellis_lambda, qpc), 1);
    } else {
#pragma unroll
      for (int r = 0; r < 16; ++r)
        lv[r] = r == 0 ? 0 : h264::quant_coef(res[r], mfc[h264::kPosClass[r]], qbits, 11);
    }
    int scan[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) scan[i] = lv[h264::kZigzag4x4[i]];
    score = decimate_score(scan, 1);
  }
  // the component's four DC terms and its AC decimation score live in the quad
  const int d0 = quad_bcast<0>(dc), d1 = quad_bcast<1>(dc), d2 = quad_bcast<2>(dc), d3 = quad_bcast<3>(dc);
  const int score_c = sum4(score);
  const bool keep_ac = score_c >= 7;
  bool any_c = false;  // this block has an AC level or its component a DC level
  bool any_ac = false, any_dc = false;  // ... each on its own (any_dc: the same on the quad's four lanes)
  if (work) {
    // chroma DC: 2x2 Hadamard + quantisation with qbits+1 (every lane of the quad: no hand-off)
    const int f[4] = {d0 + d1 + d2 + d3, d0 - d1 + d2 - d3, d0 + d1 - d2 - d3, d0 - d1 - d2 + d3};
    int cl[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) cl[i] = h264::quant_coef(f[i], mfc[0], 15 + qpc / 6 + 1, 11);
    int sv[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      sv[i] = (keep_ac && i > 0) ? lv[h264::kZigzag4x4[i]] : 0;
      any_ac |= sv[i] != 0;
    }
    any_dc = (cl[0] | cl[1] | cl[2] | cl[3]) != 0;
    store_levels(coef + h264::COEF_CHROMA_AC + (comp * 4 + cb) * 16, sv);
    if (cb == 0) {
      // chroma DC levels (Cb then Cr, 4 x int16 each at COEF_CHROMA_DC)
      auto p2 = [](int lo, int hi) { return (static_cast<uint32_t>(lo) & 0xFFFFu) | (static_cast<uint32_t>(hi) << 16); };
      *reinterpret_cast<uint2*>(coef + h264::COEF_CHROMA_DC + comp * 4) = make_uint2(p2(cl[0], cl[1]), p2(cl[2], cl[3]));
    }
    // this block's row of the 2x2 Hadamard (signs by cb: no dynamically indexed array)
    const int c0 = cl[0], c1 = cl[1], c2 = cl[2], c3 = cl[3];
    const int fcb = cb == 0 ? c0 + c1 + c2 + c3 : (cb == 1 ? c0 - c1 + c2 - c3 : (cb == 2 ? c0 + c1 - c2 - c3 : c0 - c1 - c2 + c3));
    const int ls = 16 * dvc[0];
#pragma unroll
    for (int r = 0; r < 16; ++r) res[r] = (keep_ac && r > 0) ? (lv[r] * dvc[h264::kPosClass[r]]) << (qpc / 6) : 0;
    res[0] = ((fcb * ls) << (qpc / 6)) >> 5;
    const bool any = any_ac || any_dc;
    any_c = any;
    if (any) h264::inverse_core4x4(res);
    uint8_t* recc = (comp == 0 ? a.rec_u : a.rec_v) + rcur * g.csize() + static_cast<size_t>(my * 8 + cby) * cw + mx * 8 + cbx;
#pragma unroll
    for (int y = 0; y < 4; ++y) {
      int v4[4];
#pragma unroll
      for (int x = 0; x < 4; ++x)
        v4[x] = h264::clip1(static_cast<int>(__builtin_amdgcn_ubfe(prw[y], 8 * x, 8)) + (any ? res[y * 4 + x] : 0));
      *reinterpret_cast<uint32_t*>(recc + static_cast<size_t>(y) * cw) = pack4_u8(v4);
    }
  }
  if (a.qp_flags) {
    // encode_inter_mb wrote the MB's byte from luma; an MB coded here with a chroma level has 1
    const uint64_t chroma_any = __ballot(any_c);
    if (work && (lane & 7) == 0 && ((chroma_any >> (8 * m)) & 0xFFu) != 0) a.qp_flags[o] = 1;
  }
  if (a.mask_pre) {
    // lane & 7 = comp * 4 + cb is the AC bit's index; the DC bits come from the components' first
    // lanes.  Both ballots by every lane; an MB handed to the intra kernels keeps its h264::kBlockMaskIntra.
    const uint64_t ac_nz = __ballot(any_ac), dc_nz = __ballot(any_dc);
    const uint32_t ac = static_cast<uint32_t>((ac_nz >> (8 * m)) & 0xFFu), dcb = static_cast<uint32_t>((dc_nz >> (8 * m)) & 0xFFu);
    const uint32_t bits = (ac << 19) | ((dcb & 1u) << 17) | (((dcb >> 4) & 1u) << 18);
    if (work && (lane & 7) == 0 && bits) a.mask_pre[o] |= bits;
  }
}

#ifdef MIVC_INTER_MIXED_UNIT
void launch_encode_inter_mixed(const InterArgs& a, const int8_t* mref4, dim3 grid_luma, dim3 grid_chroma, hipStream_t s) {
  hipLaunchKernelGGL(encode_inter_mb_mixed, grid_luma, dim3(64), 0, s, a, mref4);
  hipLaunchKernelGGL(encode_inter_chroma_mixed, grid_chroma, dim3(64), 0, s, a, mref4);
}
#else
// the instances with a reference per quadrant (encode_inter_mixed.hip)
void launch_encode_inter_mixed(const InterArgs& a, const int8_t* mref4, dim3 grid_luma, dim3 grid_chroma, hipStream_t s);
#endif

}  // namespace gpu
}  // namespace mivc

#ifndef MIVC_INTER_MIXED_UNIT
using namespace mivc::gpu;

extern "C" void mivc_launch_encode_inter(int B, int wmb, int hmb, const uint8_t* src_y, const uint8_t* src_u,
                                         const uint8_t* src_v, const uint8_t* ref_y, const uint8_t* ref_u,
                                         const uint8_t* ref_v, uint8_t* rec_y, uint8_t* rec_u, uint8_t* rec_v,
                                         const uint8_t* pred_y, const int16_t* mv, const int* me_cost,
                                         const int* intra_cost, const int* qp, int chroma_qp_offset, void* hdr,
                                         int16_t* coef, uint8_t* nz, uint8_t* intra_flag, int* intra_count,
                                         const int8_t* aq, const uint8_t* ref1_u, const uint8_t* ref1_v, int bmode,
                                         int t8, const int16_t* mv8, void* stream, const int* w1, int nref,
                                         const uint8_t* const* xref_u, const uint8_t* const* xref_v,
                                         const int8_t* mref, const int* wp, int trellis, float trellis_lambda,
                                         const void* route, int nbuf, uint8_t* qp_flags, uint32_t* mask_pre,
                                         const int8_t* mref4) {
  InterArgs a;
  a.qp_flags = qp_flags;
  a.mask_pre = mask_pre;
  a.rt = static_cast<const SlotRoute*>(route);
  a.nbuf = nbuf;
  a.trellis = trellis;
  a.trellis_lambda = trellis_lambda;
  a.wp = bmode ? nullptr : wp;
  for (int r = 0; r < 4; ++r) {
    const int rr = r < nref ? r : 0;
    a.refs_u[r] = rr == 0 ? ref_u : xref_u[rr];
    a.refs_v[r] = rr == 0 ? ref_v : xref_v[rr];
  }
  a.mref = mref;
  for (int r = 0; r < 4; ++r) a.w1[r] = w1[r < nref ? r : 0];
  a.g = Geom{B, wmb, hmb, wmb * 16, hmb * 16};
  a.src_y = src_y;
  a.src_u = src_u;
  a.src_v = src_v;
  a.ref_y = ref_y;
  a.ref_u = ref_u;
  a.ref_v = ref_v;
  a.rec_y = rec_y;
  a.rec_u = rec_u;
  a.rec_v = rec_v;
  a.pred_y = pred_y;
  a.mv = mv;
  a.mv8 = bmode ? nullptr : mv8;
  a.me_cost = me_cost;
  a.intra_cost = intra_cost;
  a.qp = qp;
  a.chroma_qp_offset = chroma_qp_offset;
  a.hdr = static_cast<MbHeader*>(hdr);
  a.coef = coef;
  a.nz = nz;
  a.intra_flag = intra_flag;
  a.intra_count = intra_count;
  a.aq = aq;
  a.ref1_u = ref1_u;
  a.ref1_v = ref1_v;
  a.bmode = bmode;
  a.t8 = t8;
  if (mref4 && !bmode) {  // a reference per quadrant
    launch_encode_inter_mixed(a, mref4, dim3(mb_row_grid(wmb * hmb), B), dim3(chroma_wave_grid(wmb * hmb), B),
                              static_cast<hipStream_t>(stream));
    return;
  }
  hipLaunchKernelGGL(encode_inter_mb, dim3(mb_row_grid(wmb * hmb), B), dim3(64), 0, static_cast<hipStream_t>(stream), a);
  hipLaunchKernelGGL(encode_inter_chroma, dim3(chroma_wave_grid(wmb * hmb), B), dim3(64), 0, static_cast<hipStream_t>(stream), a);
}
#endif
