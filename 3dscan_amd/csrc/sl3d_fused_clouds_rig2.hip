// the 3-step timed kernels of rig class 2 that write segmented ordered clouds (CMODE 2, sl3d_run_clouds; sl3d_fused.h)
#include "sl3d_fused.h"
namespace sl3d {
template FusedTable fused_table<fused_family_id(false, false, 2, 2)>();
}  // namespace sl3d
