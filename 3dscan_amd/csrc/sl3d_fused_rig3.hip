// the 3-step timed kernels of rig class 3 (sl3d_fused.h: plain projector K, purely radial distortion, the table in LDS), dense and
// segmented clouds
#include "sl3d_fused.h"
namespace sl3d {
template FusedTable fused_table<fused_family_id(false, false, 3, 0)>();
template FusedTable fused_table<fused_family_id(false, false, 3, 2)>();
}  // namespace sl3d
