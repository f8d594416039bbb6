// The instances of hevc_inter_cu (hevc_inter_cu.h) with the transform skip decision on the chroma
// 4x4 TUs of 8x8 CUs (hevc_tskip.h; HevcParams.tskip) without the rate-distortion check of
// hevc_rdcbf.h, in a translation unit of their own.
#include "hevc_inter_cu.h"

namespace mivc {
namespace gpu {

template <bool TSPLIT, bool RDOQ>
static void launch_tsk(const HevcInterArgs& a, dim3 grid, hipStream_t s, bool wb) {
  if (wb) hipLaunchKernelGGL((hevc_inter_cu<TSPLIT, RDOQ, true, false, true>), grid, dim3(64), 0, s, a);
  else hipLaunchKernelGGL((hevc_inter_cu<TSPLIT, RDOQ, false, false, true>), grid, dim3(64), 0, s, a);
}

void launch_hevc_inter_cu_tsk(const HevcInterArgs& a, dim3 grid, hipStream_t s, bool tu_split, bool rdoq, bool wb) {
  if (rdoq) {
    if (tu_split) launch_tsk<true, true>(a, grid, s, wb);
    else launch_tsk<false, true>(a, grid, s, wb);
  } else {
    if (tu_split) launch_tsk<true, false>(a, grid, s, wb);
    else launch_tsk<false, false>(a, grid, s, wb);
  }
}

}  // namespace gpu
}  // namespace mivc
