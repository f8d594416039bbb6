// HEVC inter prediction of one block by one wave (8.5.3.3): fractional sample interpolation
// through LDS and the weighted sample prediction, shared by hevc_inter_cu (hevc_inter.hip) and
// the stand-alone probe launch (hevc_mc_probe.hip).
#pragma once
#include "hevc_common.h"

namespace mivc {
namespace gpu {

constexpr int kWpLog2 = 6;

constexpr int kLumaTapsD[4][8] = {{0, 0, 0, 64, 0, 0, 0, 0},
                                  {-1, 4, -10, 58, 17, -5, 1, 0},
                                  {-1, 4, -11, 40, 40, -11, 4, -1},
                                  {0, 1, -5, 17, 58, -10, 4, -1}};
constexpr int kChromaTapsD[8][4] = {{0, 64, 0, 0},    {-2, 58, 10, -2}, {-4, 54, 16, -2}, {-6, 46, 28, -4},
                                    {-4, 36, 36, -4}, {-4, 28, 46, -6}, {-2, 16, 54, -4}, {-2, 10, 58, -2}};


struct InterShared {
  uint16_t win[39 * 39];  // reference window (n + 7)^2
  int tmp[39 * 32];       // horizontal pass
  int R[32 * 32], S[32 * 32];
  int R2[32 * 32];        // luma residual / reconstruction of the quarter-TU alternative
  int16_t lev2[32 * 32];  // its levels
  uint16_t pred[32 * 32];
};

// The default instance's LDS (15.8 KB with the DCT matrix instead of 26.5 KB: 10 workgroups
// per CU instead of 6): the motion-compensation window and horizontal pass live only until
// the residual is formed, the transform scratch S only after, so they share storage; the
// 16-bit intermediates (horizontal pass, the list-0 prediction of bi-prediction) are what
// the standard bounds them to (8.5.3.3.3: 14-bit predSamples, 16-bit first stage)
struct InterSharedLean {
  union {
    struct {
      uint16_t win[39 * 39];
      int16_t tmp[39 * 32];
    };
    int S[32 * 32];
  };
  int R[32 * 32];
  int16_t R2[32 * 32];  // list-0 prediction samples of a bi-predicted block
  uint16_t pred[32 * 32];
};

// motion-compensated prediction samples predSamplesLX (14-bit intermediate, 8.5.3.3.3
// fractional interpolation) of one n x n block of a component into dst[y * n + x]
template <int NT, typename SH, typename DT>
__device__ __forceinline__ void mc_inter(SH& S, const uint16_t* ref, int pw, int ph, int bx, int by, int n,
                                         int mvx, int mvy, int bd, DT* dst) {
  const int lane = lane_id();
  const int fb = NT == 8 ? 2 : 3;  // fraction bits
  const int half = NT / 2 - 1;     // taps before the sample
  const int fx = mvx & ((1 << fb) - 1), fy = mvy & ((1 << fb) - 1);
  const int ix = bx + (mvx >> fb) - half, iy = by + (mvy >> fb) - half;
  const int wn = n + NT - 1;
  for (int i = lane; i < wn * wn; i += 64) {
    const int r = i / wn, c = i - r * wn;
    const int x = clampi(ix + c, 0, pw - 1), y = clampi(iy + r, 0, ph - 1);
    S.win[r * wn + c] = ref[static_cast<size_t>(y) * pw + x];
  }
  wave_sync();
  const int sh1 = bd - 8 < 4 ? bd - 8 : 4;
  const int wsh = 14 - bd;
  auto tap = [&](int f, int k) { return NT == 8 ? kLumaTapsD[f][k] : kChromaTapsD[f][k]; };
  if (fx != 0 && fy != 0) {  // separable: horizontal pass over n + NT - 1 rows
    for (int i = lane; i < wn * n; i += 64) {
      const int r = i / n, x = i - r * n;
      int s = 0;
#pragma unroll
      for (int k = 0; k < NT; ++k) s += tap(fx, k) * S.win[r * wn + x + k];
      S.tmp[r * 32 + x] = static_cast<std::remove_reference_t<decltype(S.tmp[0])>>(s >> sh1);
    }
    wave_sync();
  }
  for (int i = lane; i < n * n; i += 64) {
    const int y = i / n, x = i - y * n;
    int v;
    if (fx == 0 && fy == 0) {
      v = static_cast<int>(S.win[(y + half) * wn + x + half]) << wsh;
    } else if (fy == 0) {
      int s = 0;
#pragma unroll
      for (int k = 0; k < NT; ++k) s += tap(fx, k) * S.win[(y + half) * wn + x + k];
      v = s >> sh1;
    } else if (fx == 0) {
      int s = 0;
#pragma unroll
      for (int k = 0; k < NT; ++k) s += tap(fy, k) * S.win[(y + k) * wn + x + half];
      v = s >> sh1;
    } else {
      int s = 0;
#pragma unroll
      for (int k = 0; k < NT; ++k) s += tap(fy, k) * S.tmp[(y + k) * 32 + x];
      v = s >> 6;
    }
    dst[i] = static_cast<DT>(v);
  }
  wave_sync();
}

// prediction of one n x n block of a component into S.pred: default weighted sample
// prediction (8.5.3.3.4.2) of one list, or the average of both (bi-prediction); with a weight
// (ww != 0), the explicit prediction (8.5.3.3.4.3) of a uni-directional block.
// WB (B pictures of a weighted slot, x265 --weightb): (ww, wo) weights list 0 and (ww1, wo1)
// list 1 -- a uni-directional block takes its own list's pair, a bi-predicted block the explicit
// bi formula when either weight is set (the caller passes (64, 0) for a list the slice does not
// weight: with (64, 0) on both lists the explicit formulas equal the default ones).  Offsets in
// 8-bit units; every intermediate fits int32 (|predSamples| < 2^15, weights <= 127, two terms,
// the offset term below 2^21).
template <int NT, bool WB = false, typename SH>
__device__ __forceinline__ void mc_block(SH& S, const uint16_t* ref0, const uint16_t* ref1, int pw, int ph,
                                         int bx, int by, int n, int dir, int mvx, int mvy, int mv1x, int mv1y, int bd,
                                         int ww = 0, int wo = 0, int ww1 = 0, int wo1 = 0) {
  const int lane = lane_id();
  const int maxv = (1 << bd) - 1;
  if (dir == hevc::DIR_BI) {
    mc_inter<NT>(S, ref0, pw, ph, bx, by, n, mvx, mvy, bd, S.R2);
    mc_inter<NT>(S, ref1, pw, ph, bx, by, n, mv1x, mv1y, bd, S.R);
    if (WB && (ww | ww1)) {  // explicit weighted sample prediction, bi-directional
      const int lwd = kWpLog2 + 14 - bd, ob = ((wo + wo1) * (1 << (bd - 8)) + 1) << lwd;
      for (int i = lane; i < n * n; i += 64) {
        const int v = (S.R2[i] * ww + S.R[i] * ww1 + ob) >> (lwd + 1);
        S.pred[i] = static_cast<uint16_t>(v < 0 ? 0 : (v > maxv ? maxv : v));
      }
    } else {
      const int sh2 = 15 - bd, off2 = 1 << (sh2 - 1);
      for (int i = lane; i < n * n; i += 64) {
        const int v = (S.R2[i] + S.R[i] + off2) >> sh2;
        S.pred[i] = static_cast<uint16_t>(v < 0 ? 0 : (v > maxv ? maxv : v));
      }
    }
  } else {
    const bool l1 = dir == hevc::DIR_L1;
    mc_inter<NT>(S, l1 ? ref1 : ref0, pw, ph, bx, by, n, l1 ? mv1x : mvx, l1 ? mv1y : mvy, bd, S.R);
    if (WB && l1) {
      ww = ww1;
      wo = wo1;
    }
    if (ww) {  // explicit weighted sample prediction, uni-directional (8.5.3.3.4.3)
      const int lwd = kWpLog2 + 14 - bd, rnd = 1 << (lwd - 1), o = wo * (1 << (bd - 8));
      for (int i = lane; i < n * n; i += 64) {
        const int v = ((S.R[i] * ww + rnd) >> lwd) + o;
        S.pred[i] = static_cast<uint16_t>(v < 0 ? 0 : (v > maxv ? maxv : v));
      }
    } else {
      const int wsh = 14 - bd, woff = 1 << (wsh - 1);
      for (int i = lane; i < n * n; i += 64) {
        const int v = (S.R[i] + woff) >> wsh;
        S.pred[i] = static_cast<uint16_t>(v < 0 ? 0 : (v > maxv ? maxv : v));
      }
    }
  }
  wave_sync();
}

}  // namespace gpu
}  // namespace mivc
