// Stand-alone launch of the rate-distortion check of an inter TU's levels against no levels
// (hv::rd_cbf_tu, hevc_rdcbf.h) as hevc_inter_cu runs it: one wave per block forms the residual
// of a source block against a prediction block (summing D0 on the way), runs
// hv::transform_quant_block with the inter dead zone and the diagonal scan, then the check, and
// stores the levels, the reconstructed samples, the flag and the terms of the comparison.
// Kernel and numpy model (tests/ref_models_hevc_rdcbf.py) meet here on planted blocks.
#include "hevc_common.h"
#include "hevc_rdcbf.h"
#include "launch.h"

namespace mivc {
namespace gpu {

struct RdCbfProbeArgs {
  const uint16_t *src, *pred;  // [nblk, n, n]
  int16_t* lev;                // [nblk, n, n] levels after the check
  uint16_t* rec;               // [nblk, n, n] reconstructed samples
  int* flag;                   // [nblk] cbf after the check
  long long* terms;            // [nblk, 3] D0, D1, Rb (D1 = D0, Rb = 0 for a block without levels)
  hv::TqParams tp;
  int lamq;
};

// RDOQ: the block function's instance, as the encoding kernels choose it
template <bool RDOQ>
__global__ __launch_bounds__(64) void hevc_rd_cbf_probe(RdCbfProbeArgs a) {
  __shared__ int R[32 * 32], S[32 * 32];
  __shared__ uint16_t P[32 * 32];
  __shared__ hv::DctLds D;
  hv::dct_lds_init(D);
  __syncthreads();
  const int lane = lane_id(), lg = a.tp.log2n, n = 1 << lg, maxv = (1 << a.tp.bd) - 1;
  const size_t base = static_cast<size_t>(blockIdx.x) * n * n;
  const uint16_t* src = a.src + base;
  int d0 = 0;
  for (int i = lane; i < n * n; i += 64) {
    const int p = a.pred[base + i];
    const int r = static_cast<int>(src[i]) - p;
    P[i] = static_cast<uint16_t>(p);
    R[(i >> lg) * 32 + (i & (n - 1))] = r;
    d0 += r * r;
  }
  d0 = sum64(d0);
  wave_sync();
  int d1, rb;
  const bool nz = hv::rd_cbf_tu(hv::transform_quant_block<RDOQ>(D, R, S, a.lev + base, n, a.tp), P, n, R, src, n, a.lev + base,
                                n, lg, maxv, a.lamq, d0, d1, rb);
  for (int i = lane; i < n * n; i += 64) {
    const int v = P[i] + R[(i >> lg) * 32 + (i & (n - 1))];
    a.rec[base + i] = static_cast<uint16_t>(v < 0 ? 0 : (v > maxv ? maxv : v));
  }
  if (lane == 0) {
    a.flag[blockIdx.x] = nz ? 1 : 0;
    a.terms[blockIdx.x * 3] = d0;
    a.terms[blockIdx.x * 3 + 1] = d1;
    a.terms[blockIdx.x * 3 + 2] = rb;
  }
}

}  // namespace gpu
}  // namespace mivc

using namespace mivc::gpu;

// returns non-zero for parameters the check is not defined for (samples above the bit depth's
// range are the caller's to avoid)
extern "C" int mivc_launch_hevc_rd_cbf_probe(int nblk, const uint16_t* src, const uint16_t* pred, int16_t* lev, uint16_t* rec,
                                             int* flag, long long* terms, int log2n, int bd, int qp, int sdh, int rdoq,
                                             int rdoq_lam, int lamq, void* stream) {
  if (nblk < 1 || log2n < 2 || log2n > 5 || (bd != 8 && bd != 10) || qp < 0 || qp > 51 + 6 * (bd - 8)) return 1;
  if (rdoq < 0 || rdoq > 2 || rdoq_lam < 0 || rdoq_lam > hv::kRdoqLamMax || lamq < 0 || lamq > hv::kRdCbfLamMax) return 1;
  RdCbfProbeArgs a;
  a.src = src;
  a.pred = pred;
  a.lev = lev;
  a.rec = rec;
  a.flag = flag;
  a.terms = terms;
  a.tp = hv::TqParams{log2n, bd, qp, false, false, sdh ? 0 : -1};  // as hevc_inter_cu: inter, diagonal scan
  a.tp.rdoq = rdoq;
  a.tp.rdoq_lam = rdoq_lam;
  a.lamq = lamq;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (rdoq) hipLaunchKernelGGL(hevc_rd_cbf_probe<true>, dim3(nblk), dim3(64), 0, s, a);
  else hipLaunchKernelGGL(hevc_rd_cbf_probe<false>, dim3(nblk), dim3(64), 0, s, a);
  return 0;
}
