// Picture sizes the kernels' fixed LDS arrays are built for.  Plain C++: the kernels size
// their arrays with these (kcommon.h), the bindings refuse a larger geometry before they
// launch (launch.h, bindings_hip.cc), and Python reads them from the module
// (_hip.max_mb_rows / max_mb_cols, ops/native.py kernel_limits).
#pragma once

namespace mivc {
namespace gpu {

// row-progress counters of the wavefront kernels (prog[kMaxRows]): H.264 MB rows, HEVC CTB rows
constexpr int kMaxRows = 272;  // 8K: 4320 / 16 = 270 MB rows
// per-column hand-over between MB rows (deblock's ringB, the spatial direct kernels' nbq)
constexpr int kMaxCols = 480;  // 8K: 7680 / 16 MB columns

// b_spatial_exact runs one lane per MB row in one workgroup of kExactWaves waves
constexpr int kExactWaves = 5;
constexpr int kExactMaxRows = 64 * kExactWaves;  // 320 >= kMaxRows
static_assert(kExactMaxRows >= kMaxRows, "b_spatial_exact must cover every picture the row limit admits");

}  // namespace gpu
}  // namespace mivc
