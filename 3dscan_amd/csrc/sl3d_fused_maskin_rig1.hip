// the MASKIN launches of rig class 1 (sl3d_fused.h: the fused kernel evaluates the views' raw selection itself -- new mask + one view
// in ONE launch): the pipelined small-launch instantiation of every N = 6..12, exact and padded, dense and segmented clouds, and the
// gated large-launch one for views known to be sparsely selected
#include "sl3d_fused.h"
namespace sl3d {
template FusedTable fused_table<fused_family_id(false, false, 1, 4)>();
template FusedTable fused_table<fused_family_id(false, false, 1, 6)>();
}  // namespace sl3d
