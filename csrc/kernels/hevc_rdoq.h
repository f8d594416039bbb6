// Rate-distortion optimised quantisation of an HEVC transform block (x265 --rdoq-level 1 / 2),
// the second user of transform_quant_block's packed-word path (hevc_common.h).
//
// Integer arithmetic only; tests/ref_models_hevc_rdoq.py is the normative text and the numpy
// model the probe launch (hevc_tq_probe.hip) is compared with exactly.  Per coefficient c at
// coder scan position p = 16 * group + q (the TU's scanIdx; DC at p = 0):
//   z = |c| * qscale, lr = min(32767, (z + (1 << (qbits - 1))) >> qbits)  (nearest, no dead zone)
//   candidates lr, lr - 1 (>= 1), 0 (lr <= 2)
//   e(l) = min(16383, (z - (l << qbits)) >> (qbits - 8)), D = e^2     ((1 / 256 step)^2; the
//          bound is reached only behind the 32767 clip and keeps e in the packed word's field)
//   J = D + lam * R(l, seen, p), R in 1 / 16 bit from the static bin costs below, ties to the
//          smaller level; lam = round(rdoq_lambda * 368): the SSD lambda of the inter TU split
//          0.57 * 2^((QP - 12) / 3) over Qstep^2 = 2^((QP - 4) / 3) is 0.0898 step^2 per bit at
//          every QP and bit depth, times 65536 / 16
// greedy in reverse scan order; a choice depends on the earlier ones only through `seen` (a
// later position kept a non-zero level), so, as in h264_trellis.h, every coefficient evaluates
// both its choices and one wave max-reduction finds the largest p whose seen = false choice is
// non-zero: positions above it take 0, it takes that choice, positions below their seen = true
// choice.  Level 2 then clears whole 4x4 groups (not group 0; only groups whose every lr <= 2)
// when sum D(0) + lam * CSBF0 < sum (D(l) + lam * R(l, true, p)) + lam * CSBF1, every group
// deciding from the step-1 levels (one lane per group).
// Costs stay in int32: D <= 16383^2 < 2^28, lam * R < 2^21 (lam <= 1472, R < 1024), and a
// group sum is 16 terms with D <= 640^2.
#pragma once
#include "kcommon.h"

namespace mivc {
namespace gpu {
namespace hv {

// typical bin costs of the residual coder in 1 / 16 bit (static: no context state)
constexpr int kRdoqSig0 = 9, kRdoqSig1 = 22;      // sig_coeff_flag 0 / 1
constexpr int kRdoqSign = 16;                     // coeff_sign_flag (bypass)
constexpr int kRdoqGt1No = 10, kRdoqGt1Yes = 24;  // coeff_abs_level_greater1_flag
constexpr int kRdoqGt2No = 11, kRdoqGt2Yes = 22;  // coeff_abs_level_greater2_flag
constexpr int kRdoqLastBase = 24, kRdoqLastStep = 20;  // last_sig_coeff prefix / suffix: base + step * floor(log2(p + 1))
constexpr int kRdoqCsbf0 = 8, kRdoqCsbf1 = 18;    // coded_sub_block_flag 0 / 1
constexpr int kRdoqLamScale = 368;                // lam of rdoq_lambda 1.0
constexpr int kRdoqLamMax = 4 * kRdoqLamScale;
constexpr int kRdoqErrMax = 16383;

// greater1 / greater2 / coeff_abs_level_remaining (Golomb-Rice, cRiceParam 0) of a level l >= 1
__device__ __forceinline__ int rdoq_g(int l) {
  if (l == 1) return kRdoqGt1No;
  if (l == 2) return kRdoqGt1Yes + kRdoqGt2No;
  const int r = l - 3;
  const int bins = r < 4 ? r + 1 : 5 + 2 * (31 - __builtin_clz(r - 3));
  return kRdoqGt1Yes + kRdoqGt2Yes + 16 * bins;
}

__device__ __forceinline__ int rdoq_rate(int l, bool seen, int p) {
  if (l == 0) return seen ? kRdoqSig0 : 0;
  return kRdoqSig1 + kRdoqSign + rdoq_g(l) + (seen ? 0 : kRdoqLastBase + kRdoqLastStep * (31 - __builtin_clz(p + 1)));
}

// index of (x, y) in the scan `scan` (0 diagonal up-right, 1 horizontal, 2 vertical) of a
// (1 << log2size)^2 grid: the inverse of hevc::scan_pos in closed form
__device__ __forceinline__ int rdoq_scan_index(int scan, int log2size, int x, int y) {
  const int n = 1 << log2size;
  if (scan == 1) return y * n + x;
  if (scan == 2) return x * n + y;
  const int d = x + y, m = 2 * n - 1 - d;
  const int before = d <= n ? d * (d + 1) / 2 : n * n - m * (m + 1) / 2;  // diagonals 0 .. d - 1
  return before + (d < n ? d : n - 1) - y;
}
// coder scan position of coefficient (x, y) of a (1 << lg)^2 TU
__device__ __forceinline__ int rdoq_pos(int scan, int lg, int x, int y) {
  return 16 * rdoq_scan_index(scan, lg - 2, x >> 2, y >> 2) + rdoq_scan_index(scan, 2, x & 3, y & 3);
}

// lr and e(lr) of |c| = a
__device__ __forceinline__ void rdoq_round(int a, int qscale, int qbits, int& lr, int& e0) {
  const int64_t z = static_cast<int64_t>(a) * qscale;
  const int64_t l = (z + (1ll << (qbits - 1))) >> qbits;
  lr = l > 32767 ? 32767 : static_cast<int>(l);
  const int64_t e = (z - (static_cast<int64_t>(lr) << qbits)) >> (qbits - 8);
  e0 = e > kRdoqErrMax ? kRdoqErrMax : static_cast<int>(e);
}
// e(l) from e(lr): l << qbits is a multiple of 1 << (qbits - 8)
__device__ __forceinline__ int rdoq_err(int e0, int lr, int l) {
  const int e = e0 + (lr - l) * 256;
  return e > kRdoqErrMax ? kRdoqErrMax : e;
}

__device__ __forceinline__ int rdoq_choose(int lr, int e0, int lam, int p, bool seen) {
  int best = lr;
  int jb = e0 * e0 + lam * rdoq_rate(lr, seen, p);
  if (lr >= 1) {
    const int e = rdoq_err(e0, lr, lr - 1);
    const int j = e * e + lam * rdoq_rate(lr - 1, seen, p);
    if (j <= jb) {
      jb = j;
      best = lr - 1;
    }
  }
  if (lr == 2) {
    const int e = rdoq_err(e0, lr, 0);
    const int j = e * e + lam * rdoq_rate(0, seen, p);
    if (j <= jb) best = 0;
  }
  return best;
}

// R [n][n] (row stride 32) holds the coefficients; on return the packed words of the parity
// pass / level write of transform_quant_block: level with the coefficient's sign (bits 0-15),
// e(level) (bits 16-30), coefficient sign (bit 31).  S: scratch.  Every lane calls.
__device__ __forceinline__ void rdoq_block(int* R, int* S, int lg, int scan, int level, int lam, int qscale, int qbits) {
  const int n = 1 << lg, lane = lane_id();
  // coefficient pass: both choices, then the last position
  int pmax = -1;
  for (int i = lane; i < n * n; i += 64) {
    const int y = i >> lg, x = i & (n - 1);
    const int c = R[y * 32 + x];
    int lr, e0;
    rdoq_round(c < 0 ? -c : c, qscale, qbits, lr, e0);
    int lf = 0, lt = 0;
    if (lr) {
      const int p = rdoq_pos(scan, lg, x, y);
      lf = rdoq_choose(lr, e0, lam, p, false);
      lt = rdoq_choose(lr, e0, lam, p, true);
      if (lf && p > pmax) pmax = p;
    }
    S[y * 32 + x] = lf | (lt << 16);
  }
  pmax = -min64(-pmax);
  for (int i = lane; i < n * n; i += 64) {
    const int y = i >> lg, x = i & (n - 1);
    const int w = S[y * 32 + x];
    int l = 0;
    if (w) {
      const int p = rdoq_pos(scan, lg, x, y);
      l = p > pmax ? 0 : (p == pmax ? w & 0xFFFF : w >> 16);
    }
    S[y * 32 + x] = l;
  }
  wave_sync();
  if (level >= 2 && lg >= 3) {  // group pass: one lane per 4x4 group
    const int nsb = n >> 2;
    if (lane < nsb * nsb) {
      const int gx = lane % nsb, gy = lane / nsb;
      const int gi = rdoq_scan_index(scan, lg - 2, gx, gy);
      int nzl = 0, big = gi == 0, d0 = 0, d1 = 0;
      for (int q = 0; q < 16; ++q) {
        const int o = (gy * 4 + (q >> 2)) * 32 + gx * 4 + (q & 3);
        const int c = R[o], l = S[o];
        int lr, e0;
        rdoq_round(c < 0 ? -c : c, qscale, qbits, lr, e0);
        nzl |= l;
        if (lr > 2) big = 1;
        if (!big) {
          const int ez = rdoq_err(e0, lr, 0), el = rdoq_err(e0, lr, l);
          d0 += ez * ez;
          d1 += el * el + lam * rdoq_rate(l, true, 16 * gi + rdoq_scan_index(scan, 2, q & 3, q >> 2));
        }
      }
      if (nzl && !big && d0 + lam * kRdoqCsbf0 < d1 + lam * kRdoqCsbf1)
        for (int q = 0; q < 16; ++q) S[(gy * 4 + (q >> 2)) * 32 + gx * 4 + (q & 3)] = 0;
    }
    wave_sync();
  }
  for (int i = lane; i < n * n; i += 64) {
    const int y = i >> lg, x = i & (n - 1);
    const int c = R[y * 32 + x], l = S[y * 32 + x];
    int lr, e0;
    rdoq_round(c < 0 ? -c : c, qscale, qbits, lr, e0);
    const int dl = rdoq_err(e0, lr, l);
    const int sl = c < 0 ? -l : l;
    R[y * 32 + x] = static_cast<int>((static_cast<uint32_t>(sl) & 0xFFFFu) | ((static_cast<uint32_t>(dl) & 0x7FFFu) << 16) |
                                     (c < 0 ? 0x80000000u : 0u));
  }
  wave_sync();
}

}  // namespace hv
}  // namespace gpu
}  // namespace mivc
