// Stand-alone launch of mc_block (hevc_mc.h), the motion compensation and weighted sample
// prediction of hevc_inter_cu: one wave per case predicts an n x n block of planted reference
// planes and stores the prediction.  Kernel and numpy model (tests/ref_models_hevc_wp.py) meet
// here on planted planes, vectors and weights instead of only through whole encodes.
#include "hevc_mc.h"
#include "launch.h"

namespace mivc {
namespace gpu {

struct McProbeArgs {
  const uint16_t *ref0, *ref1;  // [ph, pw] planes of RefPicList0[0] / RefPicList1[0]
  int pw, ph;
  const int16_t* cases;  // [ncase, 6]: block x, y, list-0 vector x, y, list-1 vector x, y
  uint16_t* out;         // [ncase, n * n] prediction samples
  int n, dir, bd;
  int ww, wo, ww1, wo1;  // mc_block's weights (0 = none)
};

// NT: 8-tap luma / 4-tap chroma filter; WB: mc_block's weightb instance; LEAN: the default
// kernel instance's LDS layout (16-bit intermediates) or the TU-split instances'
template <int NT, bool WB, bool LEAN>
__global__ __launch_bounds__(64) void hevc_mc_probe(McProbeArgs a) {
  __shared__ typename std::conditional<LEAN, InterSharedLean, InterShared>::type S;
  const int16_t* c = a.cases + static_cast<size_t>(blockIdx.x) * 6;
  mc_block<NT, WB>(S, a.ref0, a.ref1, a.pw, a.ph, c[0], c[1], a.n, a.dir, c[2], c[3], c[4], c[5], a.bd, a.ww, a.wo, a.ww1,
                   a.wo1);
  uint16_t* o = a.out + static_cast<size_t>(blockIdx.x) * a.n * a.n;
  for (int i = lane_id(); i < a.n * a.n; i += 64) o[i] = S.pred[i];
}

template <int NT, bool WB>
void launch_mc_probe(int ncase, bool lean, hipStream_t s, const McProbeArgs& a) {
  if (lean) hipLaunchKernelGGL((hevc_mc_probe<NT, WB, true>), dim3(ncase), dim3(64), 0, s, a);
  else hipLaunchKernelGGL((hevc_mc_probe<NT, WB, false>), dim3(ncase), dim3(64), 0, s, a);
}

}  // namespace gpu
}  // namespace mivc

using namespace mivc::gpu;

// returns non-zero for sizes or weights mc_block is not defined for (vectors and block positions
// are free: reference coordinates are clamped to the plane)
extern "C" int mivc_launch_hevc_mc_probe(int ncase, const uint16_t* ref0, const uint16_t* ref1, int pw, int ph,
                                         const int16_t* cases, uint16_t* out, int nt, int n, int dir, int bd, int ww, int wo,
                                         int ww1, int wo1, int wb, int lean, void* stream) {
  if (ncase < 1 || pw < 1 || ph < 1 || !ref0 || !ref1 || !cases || !out) return 1;
  if (!((nt == 8 && (n == 8 || n == 16 || n == 32)) || (nt == 4 && (n == 4 || n == 8 || n == 16)))) return 1;
  if (dir < 1 || dir > 3 || (bd != 8 && bd != 10)) return 1;
  if (ww < 0 || ww > 127 || ww1 < 0 || ww1 > 127 || wo < -128 || wo > 127 || wo1 < -128 || wo1 > 127) return 1;
  if (!wb && (ww1 || wo1)) return 1;
  McProbeArgs a{ref0, ref1, pw, ph, cases, out, n, dir, bd, ww, wo, ww1, wo1};
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (nt == 8) {
    if (wb) launch_mc_probe<8, true>(ncase, lean != 0, s, a);
    else launch_mc_probe<8, false>(ncase, lean != 0, s, a);
  } else {
    if (wb) launch_mc_probe<4, true>(ncase, lean != 0, s, a);
    else launch_mc_probe<4, false>(ncase, lean != 0, s, a);
  }
  return 0;
}
