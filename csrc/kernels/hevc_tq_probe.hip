// Stand-alone launch of hv::transform_quant_block (hevc_common.h), the transform / quantiser /
// reconstruction of every HEVC encoding kernel: one wave per block loads an n x n residual,
// runs the block function with the given parameters and stores the levels, the reconstructed
// residual and the returned flag.  Kernel and numpy model (tests/ref_models_hevc_rdoq.py) meet
// here on planted blocks instead of only through whole encodes.
#include "hevc_common.h"
#include "launch.h"

namespace mivc {
namespace gpu {

struct TqProbeArgs {
  const int* res;  // [nblk, n, n] residual
  int16_t* lev;    // [nblk, n, n] levels
  int* rec;        // [nblk, n, n] reconstructed residual (zero where the flag is 0)
  int* flag;       // [nblk] transform_quant_block's return value
  hv::TqParams tp;
};

// RDOQ: the block function's instance, as the encoding kernels choose it
template <bool RDOQ>
__global__ __launch_bounds__(64) void hevc_tq_probe(TqProbeArgs a) {
  __shared__ int R[32 * 32], S[32 * 32];
  __shared__ hv::DctLds D;
  hv::dct_lds_init(D);
  __syncthreads();
  const int lane = lane_id(), lg = a.tp.log2n, n = 1 << lg;
  const size_t base = static_cast<size_t>(blockIdx.x) * n * n;
  for (int i = lane; i < n * n; i += 64) R[(i >> lg) * 32 + (i & (n - 1))] = a.res[base + i];
  wave_sync();
  const bool nz = hv::transform_quant_block<RDOQ>(D, R, S, a.lev + base, n, a.tp);
  for (int i = lane; i < n * n; i += 64) a.rec[base + i] = nz ? R[(i >> lg) * 32 + (i & (n - 1))] : 0;
  if (lane == 0) a.flag[blockIdx.x] = nz ? 1 : 0;
}

}  // namespace gpu
}  // namespace mivc

using namespace mivc::gpu;

// returns non-zero for parameters the block function is not defined for
extern "C" int mivc_launch_hevc_tq_probe(int nblk, const int* res, int16_t* lev, int* rec, int* flag, int log2n, int bd,
                                         int qp, int intra, int dst, int scan, int sdh, int rdoq, int rdoq_lam, int mfma,
                                         void* stream) {
  if (nblk < 1 || log2n < 2 || log2n > 5 || (bd != 8 && bd != 10) || qp < 0 || qp > 51 + 6 * (bd - 8)) return 1;
  if ((dst && log2n != 2) || scan < 0 || scan > 2 || rdoq < 0 || rdoq > 2 || rdoq_lam < 0 || rdoq_lam > hv::kRdoqLamMax) return 1;
  TqProbeArgs a;
  a.res = res;
  a.lev = lev;
  a.rec = rec;
  a.flag = flag;
  a.tp = hv::TqParams{log2n, bd, qp, intra != 0, dst != 0, sdh ? scan : -1};
  a.tp.mfma = mfma != 0;
  a.tp.scan = scan;
  a.tp.rdoq = rdoq;
  a.tp.rdoq_lam = rdoq_lam;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (rdoq) hipLaunchKernelGGL(hevc_tq_probe<true>, dim3(nblk), dim3(64), 0, s, a);
  else hipLaunchKernelGGL(hevc_tq_probe<false>, dim3(nblk), dim3(64), 0, s, a);
  return 0;
}
