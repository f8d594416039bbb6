// In-loop deblocking filter (clause 8.7) of decoded High 10 pictures: planes of 16-bit
// samples (BitDepthY == BitDepthC in {9, 10}) in the decoder's DPB layout, boundary strengths
// from the parser.  Decoder only: no derivation from the records and no encoder routing
// (deblock.hip is the byte-packed 8-bit kernel of the encoder and of 8-bit decoding).
//
// Dependency order as stated at the top of deblock.hip: MB (x, y) runs after (x - 1, y) and
// (x + 1, y - 1).  One workgroup per slot, wave w owns MB rows w, w + kDeblock16Waves, ...;
// row progress counters in LDS, samples handed over through global memory (row_wait /
// row_publish, as decode_intra_wavefront).  Per MB the wave
//   1. fetches its own samples, waits for MB (x + 1, y - 1),
//   2. loads the 4-sample left / top halo; both go into an LDS tile (two samples a dword),
//   3. filters the vertical edges left to right, then the horizontal ones top to bottom, a
//      line per lane (lanes 0-15 luma, 16-23 Cb, 24-31 Cr), in place in the tile,
//   4. stores what it may have changed: its own samples, the three halo columns of MB
//      (x - 1, y) and the three halo rows of MB (x, y - 1) -- both final by then but for this
//      MB's filter, and touched by no other MB until this one is published.
// An MB whose boundary strengths are all zero touches no sample and is skipped.
//
// What differs from 8 bits (8.7.2.2, as h264_decoder.cc deblock_picture): qPp / qPq are the
// MBs' QPY (chroma: their QPC) without the bit-depth offset -- QPY may be negative, I_PCM
// counts as 0 (the parser's records carry that) --, the average indexes the tables clipped
// to 0..51, alpha' / beta' / tC0' are scaled by 1 << (bd - 8), clips go to (1 << bd) - 1.
#include "kcommon.h"
#include "launch.h"

namespace mivc {
namespace gpu {

using h264::MbHeader;

struct Deblock16Args {
  Geom g;
  uint16_t *rec_y, *rec_u, *rec_v;  // [B][dpb_n] pictures; picture cur_idx[slot] is filtered
  const MbHeader* hdr;              // [B, nmb]
  const uint8_t* bs;                // [B, nmb, 16] 4 bits per segment (h264_decoder.h DecodedPicture::bs)
  int chroma_qp_offset;
  int alpha_off, beta_off;          // slice_alpha_c0_offset_div2 * 2, slice_beta_offset_div2 * 2
  int bd;
  int dpb_n;
  const int16_t* cur_idx;
  int* err;
};

constexpr int kDeblock16Waves = 16;  // MB rows in flight (row y trails row y - 1 by two MBs)
constexpr int LT16 = 20;  // luma tile stride: 4 halo + 16 (rows -4..15, cols -4..15)
constexpr int CT16 = 12;  // chroma tile stride: 4 halo + 8

struct Deblock16Shared {
  alignas(8) uint16_t ty[LT16 * LT16];
  alignas(8) uint16_t tc[2][CT16 * CT16];
  int bs[2][4][4];       // [dir][edge][segment]
  int par[2][2][2][5];   // [dir][mb edge / inner][luma / chroma]: alpha, beta, tc0 for bS 1..3
};

// filter one line across an edge (8.7.2.3 / 8.7.2.4); q0 points at q0, step = distance p0 -> q0
__device__ __forceinline__ void dbk16_line(uint16_t* q0p, int step, int bs, int alpha, int beta, int tc0, bool chroma,
                                           int maxv) {
  const int p0 = q0p[-step], p1 = q0p[-2 * step], q0 = q0p[0], q1 = q0p[step];
  if (!(abs(p0 - q0) < alpha && abs(p1 - p0) < beta && abs(q1 - q0) < beta)) return;
  const int p2 = chroma ? 0 : q0p[-3 * step], q2 = chroma ? 0 : q0p[2 * step];
  const bool apb = !chroma && abs(p2 - p0) < beta, aqb = !chroma && abs(q2 - q0) < beta;
  if (bs < 4) {
    const int tc = chroma ? tc0 + 1 : tc0 + apb + aqb;
    const int delta = clampi((((q0 - p0) << 2) + (p1 - q1) + 4) >> 3, -tc, tc);
    q0p[-step] = static_cast<uint16_t>(h264::clip1(p0 + delta, maxv));
    q0p[0] = static_cast<uint16_t>(h264::clip1(q0 - delta, maxv));
    const int avg = (p0 + q0 + 1) >> 1;
    if (apb) q0p[-2 * step] = static_cast<uint16_t>(p1 + clampi((p2 + avg - (p1 << 1)) >> 1, -tc0, tc0));
    if (aqb) q0p[step] = static_cast<uint16_t>(q1 + clampi((q2 + avg - (q1 << 1)) >> 1, -tc0, tc0));
  } else {
    const bool strong = abs(p0 - q0) < ((alpha >> 2) + 2);
    if (apb && strong) {
      const int p3 = q0p[-4 * step];
      q0p[-step] = static_cast<uint16_t>((p2 + 2 * p1 + 2 * p0 + 2 * q0 + q1 + 4) >> 3);
      q0p[-2 * step] = static_cast<uint16_t>((p2 + p1 + p0 + q0 + 2) >> 2);
      q0p[-3 * step] = static_cast<uint16_t>((2 * p3 + 3 * p2 + p1 + p0 + q0 + 4) >> 3);
    } else {
      q0p[-step] = static_cast<uint16_t>((2 * p1 + p0 + q1 + 2) >> 2);
    }
    if (aqb && strong) {
      const int q3 = q0p[3 * step];
      q0p[0] = static_cast<uint16_t>((p1 + 2 * p0 + 2 * q0 + 2 * q1 + q2 + 4) >> 3);
      q0p[step] = static_cast<uint16_t>((p0 + q0 + q1 + q2 + 2) >> 2);
      q0p[2 * step] = static_cast<uint16_t>((2 * q3 + 3 * q2 + q1 + q0 + p0 + 4) >> 3);
    } else {
      q0p[0] = static_cast<uint16_t>((2 * q1 + q0 + p1 + 2) >> 2);
    }
  }
}

// the (up to) four edges of one direction on this lane's line
__device__ __forceinline__ void dbk16_edges(Deblock16Shared& S, int dir, int lane, bool has_nb, int maxv) {
  if (lane >= 32) return;
  const bool chroma = lane >= 16;
  const int comp = (lane - 16) >> 3, line = chroma ? (lane & 7) : lane;
  const int seg = chroma ? line >> 1 : line >> 2;
  const int pitch = chroma ? CT16 : LT16;
  uint16_t* t = chroma ? S.tc[comp] : S.ty;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    if (chroma && (e & 1)) continue;  // chroma edges 0 and 4 take the strengths of luma edges 0 and 2
    const int bs = (e == 0 && !has_nb) ? 0 : S.bs[dir][e][seg];
    if (bs == 0) continue;
    const int* P = S.par[dir][e == 0 ? 0 : 1][chroma ? 1 : 0];
    const int tc0 = bs < 4 ? P[2 + bs - 1] : 0;
    const int pos = 4 + (chroma ? e * 2 : e * 4);  // the edge's q0 along the line
    uint16_t* q0 = dir == 0 ? t + (4 + line) * pitch + pos : t + pos * pitch + 4 + line;
    dbk16_line(q0, dir == 0 ? 1 : pitch, bs, P[0], P[1], tc0, chroma, maxv);
  }
}

__global__ __launch_bounds__(64 * kDeblock16Waves) void deblock16_wavefront(Deblock16Args a) {
  __shared__ Deblock16Shared SS[kDeblock16Waves];
  __shared__ int prog[kMaxRows];
  const Geom& g = a.g;
  const int slot = blockIdx.x;
  for (int i = threadIdx.x; i < g.hmb; i += blockDim.x) prog[i] = 0;
  __syncthreads();
  const int w = wave_id(), lane = lane_id();
  Deblock16Shared& S = SS[w];
  const int W = g.W, cw = g.cw(), wmb = g.wmb, hmb = g.hmb;
  const int maxv = (1 << a.bd) - 1, qpbd = 6 * (a.bd - 8), scale = a.bd - 8;
  const size_t pic = static_cast<size_t>(slot) * a.dpb_n + a.cur_idx[slot];
  uint16_t* const recy = a.rec_y + pic * g.ysize();
  uint16_t* const rcu = a.rec_u + pic * g.csize();
  uint16_t* const rcv = a.rec_v + pic * g.csize();
  const MbHeader* hdr = a.hdr + static_cast<size_t>(slot) * g.nmb();
  const uint8_t* bsp = a.bs + static_cast<size_t>(slot) * g.nmb() * 16;

  for (int y = w; y < hmb; y += kDeblock16Waves) {
    const bool has_top = y > 0;
    for (int x = 0; x < wmb; ++x) {
      const bool has_left = x > 0;
      const int mb = y * wmb + x;
      // ---- boundary strengths: lane = dir * 16 + edge * 4 + segment
      int bs = 0;
      if (lane < 32) {
        bs = (bsp[static_cast<size_t>(mb) * 16 + (lane >> 1)] >> ((lane & 1) * 4)) & 15;
        if (((lane >> 2) & 3) == 0 && !((lane >> 4) ? has_top : has_left)) bs = 0;
        if (bs > 4) bs = 4;
      }
      if (__ballot(bs != 0) == 0ull) {
        // nothing to filter (uniform): this MB reads and writes no sample, so it has nothing to
        // wait for; every MB that filters waits for its own neighbours
        row_publish(prog, y, x + 1);
        continue;
      }
      if (lane < 32) S.bs[lane >> 4][(lane >> 2) & 3][lane & 3] = bs;
      // ---- filter parameters: lane - 32 = dir * 4 + inner * 2 + chroma
      if (lane >= 32 && lane < 40) {
        const int i = lane - 32, dir = i >> 2, inner = (i >> 1) & 1, ch = i & 1;
        const int nb = dir == 0 ? (has_left ? mb - 1 : mb) : (has_top ? mb - wmb : mb);
        int qq = hdr[mb].qp, qn = inner ? qq : static_cast<int>(hdr[nb].qp);
        if (ch) {  // QPC of the two MBs (8.7.2.2 with 8.5.8): no bit-depth offset added
          qq = h264::chroma_qp_bd(qq, a.chroma_qp_offset, qpbd);
          qn = h264::chroma_qp_bd(qn, a.chroma_qp_offset, qpbd);
        }
        const int qpav = (qq + qn + 1) >> 1;
        const int ia = clampi(qpav + a.alpha_off, 0, 51), ib = clampi(qpav + a.beta_off, 0, 51);
        int* P = S.par[dir][inner][ch];
        P[0] = static_cast<int>(h264::kAlpha[ia]) << scale;
        P[1] = static_cast<int>(h264::kBeta[ib]) << scale;
        P[2] = static_cast<int>(h264::kTc0[ia][0]) << scale;
        P[3] = static_cast<int>(h264::kTc0[ia][1]) << scale;
        P[4] = static_cast<int>(h264::kTc0[ia][2]) << scale;
      }
      // ---- the MB and its halo -> tile (dword = two samples; halo outside the picture is
      // neither read nor used: its edges have strength 0).  No other MB writes this MB's own
      // samples before it runs, so they are fetched ahead of the wait for MB (x + 1, y - 1);
      // the halo, which the neighbours' filters changed, after it.
      constexpr int kYD = LT16 * (LT16 / 2), kCD = 2 * CT16 * (CT16 / 2);  // tile dwords
      constexpr int kYI = (kYD + 63) / 64, kCI = (kCD + 63) / 64;          // per lane
      auto y_at = [&](int i, int& r, int& c2) { r = i / (LT16 / 2); c2 = i - r * (LT16 / 2); };
      auto c_at = [&](int i, int& c, int& r, int& c2) {
        c = i / (CT16 * (CT16 / 2));
        const int j = i - c * (CT16 * (CT16 / 2));
        r = j / (CT16 / 2);
        c2 = j - r * (CT16 / 2);
      };
      auto y_src = [&](int r, int c2) {
        return reinterpret_cast<const uint32_t*>(recy + static_cast<size_t>(y * 16 + r - 4) * W + x * 16 + c2 * 2 - 4);
      };
      auto c_src = [&](int c, int r, int c2) {
        return reinterpret_cast<const uint32_t*>((c ? rcv : rcu) + static_cast<size_t>(y * 8 + r - 4) * cw + x * 8 + c2 * 2 - 4);
      };
      uint32_t own_y[kYI], own_c[kCI];
#pragma unroll
      for (int k = 0; k < kYI; ++k) {
        int r, c2;
        y_at(lane + 64 * k, r, c2);
        own_y[k] = (lane + 64 * k < kYD && r >= 4 && c2 >= 2) ? *y_src(r, c2) : 0u;
      }
#pragma unroll
      for (int k = 0; k < kCI; ++k) {
        int c, r, c2;
        c_at(lane + 64 * k, c, r, c2);
        own_c[k] = (lane + 64 * k < kCD && r >= 4 && c2 >= 2) ? *c_src(c, r, c2) : 0u;
      }
      if (has_top) row_wait(prog, y - 1, min(x + 2, wmb), a.err);
#pragma unroll
      for (int k = 0; k < kYI; ++k) {
        int r, c2;
        y_at(lane + 64 * k, r, c2);
        if (lane + 64 * k >= kYD) continue;
        uint32_t* dst = reinterpret_cast<uint32_t*>(&S.ty[r * LT16 + c2 * 2]);
        if (r >= 4 && c2 >= 2) *dst = own_y[k];
        else if ((r >= 4 || has_top) && (c2 >= 2 || has_left)) *dst = *y_src(r, c2);
      }
#pragma unroll
      for (int k = 0; k < kCI; ++k) {
        int c, r, c2;
        c_at(lane + 64 * k, c, r, c2);
        if (lane + 64 * k >= kCD) continue;
        uint32_t* dst = reinterpret_cast<uint32_t*>(&S.tc[c][r * CT16 + c2 * 2]);
        if (r >= 4 && c2 >= 2) *dst = own_c[k];
        else if ((r >= 4 || has_top) && (c2 >= 2 || has_left)) *dst = *c_src(c, r, c2);
      }
      wave_sync();
      dbk16_edges(S, 0, lane, has_left, maxv);
      wave_sync();
      dbk16_edges(S, 1, lane, has_top, maxv);
      wave_sync();
      // ---- store rows -3..15 x cols -4..15, without the corner that belongs to MB (x - 1, y - 1)
      for (int i = lane; i < LT16 * (LT16 / 2); i += 64) {
        const int r = i / (LT16 / 2), c2 = i - r * (LT16 / 2);
        if (r >= 4 ? (c2 >= 2 || has_left) : (r >= 1 && c2 >= 2 && has_top))
          *reinterpret_cast<uint32_t*>(recy + static_cast<size_t>(y * 16 + r - 4) * W + x * 16 + c2 * 2 - 4) =
              *reinterpret_cast<const uint32_t*>(&S.ty[r * LT16 + c2 * 2]);
      }
      for (int i = lane; i < 2 * CT16 * (CT16 / 2); i += 64) {
        const int c = i / (CT16 * (CT16 / 2)), j = i - c * (CT16 * (CT16 / 2));
        const int r = j / (CT16 / 2), c2 = j - r * (CT16 / 2);
        if (r >= 4 ? (c2 >= 1 && (c2 >= 2 || has_left)) : (r >= 2 && c2 >= 2 && has_top))
          *reinterpret_cast<uint32_t*>((c ? rcv : rcu) + static_cast<size_t>(y * 8 + r - 4) * cw + x * 8 + c2 * 2 - 4) =
              *reinterpret_cast<const uint32_t*>(&S.tc[c][r * CT16 + c2 * 2]);
      }
      row_publish(prog, y, x + 1);
    }
  }
}

}  // namespace gpu
}  // namespace mivc

using namespace mivc::gpu;

// decoder: filter picture cur_idx[slot] of each slot's DPB of bd-bit samples (bd 9 or 10) with
// the parser's boundary strengths
extern "C" void mivc_launch_deblock_dpb16(int B, int wmb, int hmb, int dpb_n, uint16_t* dpb_y, uint16_t* dpb_u,
                                          uint16_t* dpb_v, const int16_t* cur_idx, const void* hdr, const uint8_t* bs,
                                          int chroma_qp_offset, int alpha_off, int beta_off, int bd, int* err,
                                          void* stream) {
  Deblock16Args a;
  a.g = Geom{B, wmb, hmb, wmb * 16, hmb * 16};
  a.rec_y = dpb_y;
  a.rec_u = dpb_u;
  a.rec_v = dpb_v;
  a.hdr = static_cast<const mivc::h264::MbHeader*>(hdr);
  a.bs = bs;
  a.chroma_qp_offset = chroma_qp_offset;
  a.alpha_off = alpha_off;
  a.beta_off = beta_off;
  a.bd = bd;
  a.dpb_n = dpb_n;
  a.cur_idx = cur_idx;
  a.err = err;
  hipLaunchKernelGGL(deblock16_wavefront, dim3(B), dim3(64 * kDeblock16Waves), 0, static_cast<hipStream_t>(stream), a);
}
