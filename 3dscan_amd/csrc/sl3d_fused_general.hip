// the instantiations off the benchmarked path (sl3d_fused.h): the parity mode (KEEP: every stage-boundary plane of the reference,
// rig class 0) and the 4-step / all-invalid 5-step fringes (FGEN: 3/wrapped_phase.cpp:188-229), dense and segmented
#include "sl3d_fused.h"
namespace sl3d {
template FusedTable fused_table<fused_family_id(true, false, 0, 0)>();
template FusedTable fused_table<fused_family_id(true, true, 0, 0)>();
template FusedTable fused_table<fused_family_id(false, true, 0, 0)>();
template FusedTable fused_table<fused_family_id(false, true, 1, 0)>();
template FusedTable fused_table<fused_family_id(false, true, 2, 0)>();
template FusedTable fused_table<fused_family_id(false, true, 0, 2)>();
template FusedTable fused_table<fused_family_id(false, true, 1, 2)>();
template FusedTable fused_table<fused_family_id(false, true, 2, 2)>();
}  // namespace sl3d
