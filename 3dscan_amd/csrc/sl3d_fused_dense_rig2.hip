// the 3-step timed dense kernels of rig class 2 (sl3d_fused.h): N = 6..12 exact, NMAX = 6..12 padded (unequal axes) + the unroll bound 16, each with and
// without the LDS reciprocal table
#include "sl3d_fused.h"
namespace sl3d {
template FusedTable fused_table<fused_family_id(false, false, 2, 0)>();
}  // namespace sl3d
