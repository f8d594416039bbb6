// Auto-variance adaptive quantisation (x264 --aq-mode 2 / 3), the part both codecs share.
//
// Per slot and coded picture, over its N 16x16 blocks with AC energy e_i (aq.hip aq_energy /
// hevc_filters.hip, at bit depth bd):
//   a_i  = (e_i / 4^(bd - 8) + 1) ^ 0.125                 (the "term" of a block, >= 1)
//   m    = mean a_i,  m2 = mean a_i^2,  avg = m - 0.5 (m2 - 14) / m
//   adj_i = strength * m * (a_i - avg)                    mode 2
//         + strength * (1 - 14 / a_i^2)                   mode 3 (dark-scene bias)
// A block's offset needs the sums over its whole picture, so the rule runs as two launches: a
// term pass stores a_i as float32 ([B, nblocks]; the source is read once, as for mode 1), and a
// finish pass -- one workgroup per slot -- sums a_i and a_i^2 in double in a fixed order
// (strided per-thread partials, then an LDS tree; no atomics: the sums, and with them the coded
// bytes, are the same from run to run), derives m and avg and writes the offsets.
#pragma once
#include "kcommon.h"

namespace mivc {
namespace gpu {

constexpr int kAqFinishThreads = 1024;

// x = e / 4^(bd - 8) (exact in float for 8-bit energies, below 2^24) -> (x + 1)^(1/8) by three
// correctly rounded square roots: about one ulp, the same value wherever it is computed
__device__ __forceinline__ float aq_term(float x) { return sqrtf(sqrtf(sqrtf(x + 1.0f))); }

struct AqAutoStats {
  float sm;    // strength * m
  float avg;
  float bias;  // strength in mode 3, 0 in mode 2
};

// every thread of the kAqFinishThreads-wide workgroup calls this; t: the slot's n terms,
// red: 2 * kAqFinishThreads doubles of LDS
__device__ __forceinline__ AqAutoStats aq_auto_stats(const float* __restrict__ t, int n, int mode, float strength,
                                                     double* red) {
  const int tid = threadIdx.x;
  double s1 = 0.0, s2 = 0.0;
  for (int i = tid; i < n; i += kAqFinishThreads) {
    const double a = static_cast<double>(t[i]);
    s1 += a;
    s2 += a * a;
  }
  red[tid] = s1;
  red[kAqFinishThreads + tid] = s2;
  __syncthreads();
  for (int off = kAqFinishThreads / 2; off > 0; off >>= 1) {
    if (tid < off) {
      red[tid] += red[tid + off];
      red[kAqFinishThreads + tid] += red[kAqFinishThreads + tid + off];
    }
    __syncthreads();
  }
  const double m = red[0] / n, m2 = red[kAqFinishThreads] / n;  // m >= 1
  AqAutoStats st;
  st.sm = static_cast<float>(strength * m);
  st.avg = static_cast<float>(m - 0.5 * (m2 - 14.0) / m);
  st.bias = mode == 3 ? strength : 0.0f;
  return st;
}

__device__ __forceinline__ float aq_auto_adj(const AqAutoStats& st, float a) {
  float adj = st.sm * (a - st.avg);
  if (st.bias != 0.0f) adj += st.bias * (1.0f - 14.0f / (a * a));  // (uniform)
  return adj;
}

}  // namespace gpu
}  // namespace mivc
