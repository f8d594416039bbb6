// Stand-alone launch of the transform skip decision of a 4x4 TU (hv::tskip_tu, hevc_tskip.h) as
// hevc_intra_recon and hevc_inter_cu run it: one wave per block forms the residual of a source
// block against a prediction block, runs hv::transform_quant_block as configured (candidate A),
// then the decision, and stores the levels, the reconstructed samples, the chosen
// transform_skip_flag, the cbf and the terms of the comparison.  Kernel and numpy model
// (tests/ref_models_hevc_tskip.py) meet here on planted blocks.
#include "hevc_tskip.h"
#include "launch.h"

namespace mivc {
namespace gpu {

struct TskipProbeArgs {
  const uint16_t *src, *pred;  // [nblk, 4, 4]
  int16_t* lev;                // [nblk, 4, 4] the winner's levels
  uint16_t* rec;               // [nblk, 4, 4] reconstructed samples
  int* flag;                   // [nblk, 2] transform_skip_flag, cbf
  long long* terms;            // [nblk, 4] D_A, D_B, R_A, R_B
  hv::TqParams tp;
  int scan, lamq;
};

// RDOQ: the block function's instance, as the encoding kernels choose it
template <bool RDOQ>
__global__ __launch_bounds__(64) void hevc_tskip_probe(TskipProbeArgs a) {
  __shared__ int R[32 * 32], S[32 * 32];
  __shared__ uint16_t P[16];
  __shared__ hv::DctLds D;
  hv::dct_lds_init(D);
  __syncthreads();
  const int lane = lane_id(), maxv = (1 << a.tp.bd) - 1;
  const size_t base = static_cast<size_t>(blockIdx.x) * 16;
  const uint16_t* src = a.src + base;
  if (lane < 16) {
    const int p = a.pred[base + lane];
    P[lane] = static_cast<uint16_t>(p);
    R[(lane >> 2) * 32 + (lane & 3)] = static_cast<int>(src[lane]) - p;
  }
  wave_sync();
  bool ts;
  hv::TskipTerms t;
  const bool nza = hv::transform_quant_block<RDOQ>(D, R, S, a.lev + base, 4, a.tp);
  const bool nz = hv::tskip_tu<RDOQ>(D, nza, P, 4, R, S, src, 4, a.lev + base, 4, a.tp, a.scan, maxv, a.lamq, ts, t);
  if (lane < 16) {
    const int v = P[lane] + (nz ? R[(lane >> 2) * 32 + (lane & 3)] : 0);
    a.rec[base + lane] = static_cast<uint16_t>(v < 0 ? 0 : (v > maxv ? maxv : v));
  }
  if (lane == 0) {
    a.flag[blockIdx.x * 2] = ts ? 1 : 0;
    a.flag[blockIdx.x * 2 + 1] = nz ? 1 : 0;
    a.terms[blockIdx.x * 4] = t.d_a;
    a.terms[blockIdx.x * 4 + 1] = t.d_b;
    a.terms[blockIdx.x * 4 + 2] = t.r_a;
    a.terms[blockIdx.x * 4 + 3] = t.r_b;
  }
}

}  // namespace gpu
}  // namespace mivc

using namespace mivc::gpu;

// returns non-zero for parameters the decision is not defined for (samples above the bit depth's
// range are the caller's to avoid)
extern "C" int mivc_launch_hevc_tskip_probe(int nblk, const uint16_t* src, const uint16_t* pred, int16_t* lev, uint16_t* rec,
                                            int* flag, long long* terms, int bd, int qp, int intra, int dst, int scan, int sdh,
                                            int rdoq, int rdoq_lam, int lamq, void* stream) {
  if (nblk < 1 || (bd != 8 && bd != 10) || qp < 0 || qp > 51 + 6 * (bd - 8) || scan < 0 || scan > 2) return 1;
  if (rdoq < 0 || rdoq > 2 || rdoq_lam < 0 || rdoq_lam > hv::kRdoqLamMax || lamq < 0 || lamq > hv::kRdCbfLamMax) return 1;
  if (dst && !intra) return 1;
  TskipProbeArgs a;
  a.src = src;
  a.pred = pred;
  a.lev = lev;
  a.rec = rec;
  a.flag = flag;
  a.terms = terms;
  a.tp = hv::TqParams{2, bd, qp, intra != 0, dst != 0, sdh ? scan : -1};
  a.tp.mfma = false;
  a.tp.scan = scan;
  a.tp.rdoq = rdoq;
  a.tp.rdoq_lam = rdoq_lam;
  a.scan = scan;
  a.lamq = lamq;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (rdoq) hipLaunchKernelGGL(hevc_tskip_probe<true>, dim3(nblk), dim3(64), 0, s, a);
  else hipLaunchKernelGGL(hevc_tskip_probe<false>, dim3(nblk), dim3(64), 0, s, a);
  return 0;
}
