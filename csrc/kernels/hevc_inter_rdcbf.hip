// The instances of hevc_inter_cu (hevc_inter_cu.h) with the rate-distortion check of every TU's
// levels against no levels (hevc_rdcbf.h; HevcParams.rd_cbf), in a translation unit of their own.
#include "hevc_inter_cu.h"

namespace mivc {
namespace gpu {

template <bool TSPLIT, bool RDOQ>
static void launch_rdc(const HevcInterArgs& a, dim3 grid, hipStream_t s, bool wb) {
  if (wb) hipLaunchKernelGGL((hevc_inter_cu<TSPLIT, RDOQ, true, true>), grid, dim3(64), 0, s, a);
  else hipLaunchKernelGGL((hevc_inter_cu<TSPLIT, RDOQ, false, true>), grid, dim3(64), 0, s, a);
}

void launch_hevc_inter_cu_rdc(const HevcInterArgs& a, dim3 grid, hipStream_t s, bool tu_split, bool rdoq, bool wb) {
  if (rdoq) {
    if (tu_split) launch_rdc<true, true>(a, grid, s, wb);
    else launch_rdc<false, true>(a, grid, s, wb);
  } else {
    if (tu_split) launch_rdc<true, false>(a, grid, s, wb);
    else launch_rdc<false, false>(a, grid, s, wb);
  }
}

}  // namespace gpu
}  // namespace mivc
