// H.264 motion-vector prediction from the neighbouring partitions A (left), B (above) and C
// (above-right, else D above-left), clause 8.4.1.3: shared by the decision passes (h264_b.hip,
// h264_p_refine.hip) and the CAVLC writer (cavlc.hip).
#pragma once
#include "kcommon.h"

namespace mivc {
namespace gpu {

__device__ __forceinline__ int med3(int a, int b, int c) { return max(min(a, b), min(max(a, b), c)); }

struct NbMv16 {
  bool avail;
  int ref;
  int mv[2];
};

// Spatial direct of one list (8.4.1.2.2): refIdx = MinPositive over the neighbours A, B, C
// (C replaced by D by the caller), the vector = the 16x16 motion-vector predictor of that
// reference (8.4.1.3: a single neighbour on it gives its vector, else the median, with A
// standing in for B and C when only A is available)
__device__ __forceinline__ void spatial_pmv(NbMv16 A, NbMv16 B, NbMv16 C, int& ref, int& px, int& py) {
  auto minpos = [](int p, int qv) { return (p >= 0 && qv >= 0) ? min(p, qv) : max(p, qv); };
  ref = minpos(A.ref, minpos(B.ref, C.ref));
  px = py = 0;
  if (ref < 0) return;
  if (!B.avail && !C.avail && A.avail) {
    B = A;
    C = A;
  }
  const int match = (A.ref == ref) + (B.ref == ref) + (C.ref == ref);
  if (match == 1) {
    const NbMv16& m = A.ref == ref ? A : (B.ref == ref ? B : C);
    px = m.mv[0];
    py = m.mv[1];
  } else {
    px = med3(A.mv[0], B.mv[0], C.mv[0]);
    py = med3(A.mv[1], B.mv[1], C.mv[1]);
  }
}

// clause 8.4.1.3.1 with every neighbour at ref 0 (P partitions)
__device__ __forceinline__ void med_pred(int ax, int ay, bool ha, int bx, int by, bool hb, int cx, int cy, bool hc,
                                         int* px, int* py) {
  if (ha && !hb && !hc) {  // B and C unavailable, A available -> A
    *px = ax;
    *py = ay;
    return;
  }
  if (!ha) ax = ay = 0;
  if (!hb) bx = by = 0;
  if (!hc) cx = cy = 0;
  *px = med3(ax, bx, cx);
  *py = med3(ay, by, cy);
}

}  // namespace gpu
}  // namespace mivc
