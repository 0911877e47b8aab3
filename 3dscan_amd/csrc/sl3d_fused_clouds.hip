// the 3-step timed kernels that write segmented ordered clouds (CMODE 2, sl3d_run_clouds), rig classes 0 and 1 (sl3d_fused.h; rig class 2:
// sl3d_fused_clouds_rig2.hip, rig class 3: sl3d_fused_rig3.hip)
#include "sl3d_fused.h"
namespace sl3d {
template FusedTable fused_table<fused_family_id(false, false, 0, 2)>();
template FusedTable fused_table<fused_family_id(false, false, 1, 2)>();
}  // namespace sl3d
