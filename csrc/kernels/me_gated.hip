// The gated instances of the motion search (me_search.h): one wave per run of kGateSpan MBs.
#define MIVC_ME_GATED_UNIT
#include "me_search.h"

namespace mivc {
namespace gpu {

void launch_me_gated(const MeArgs& a, hipStream_t s) {
  const dim3 grid((a.g.nmb() + kGateSpan - 1) / kGateSpan, a.g.B);
  if (a.range <= 8) hipLaunchKernelGGL((me_p16x16<8, kGateSpan>), grid, dim3(64), 0, s, a);
  else hipLaunchKernelGGL((me_p16x16<kMaxR, kGateSpan>), grid, dim3(64), 0, s, a);
}

}  // namespace gpu
}  // namespace mivc
