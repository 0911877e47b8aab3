// sl3d_capi_period.cpp -- sl3d_repair_periods: the repair of 2*Pi period jumps between stage 4 and stage 5.  The argument checks
// are period_check_args (sl3d_period.h, which tests/native/period_check.cpp compiles without HIP); the kernels are sl3d_period.hip.
#include "sl3d_capi_internal.h"
#include "sl3d_period.h"

static_assert(SL3D_E_INVALID_ARG == -1 && SL3D_E_STATE == -4 && SL3D_E_UNSUPPORTED == -5, "period_check_args returns these values");

// (arguments checked by the caller: a KEEP_STAGES context, an axis with Gray planes)
int period_repair_enqueue(sl3d_ctx *x, int view, int axis, int radius)
{
    const bool wide = (axis == 0 ? x->P.Nv : x->P.Nh) >= 8;
    int rc = ensure_plane(x, &x->d_period_jump, x->P.px_view_stride);
    if (!rc && wide) rc = ensure_plane(x, &x->d_period_wide, x->P.px_view_stride);
    if (!rc) rc = ensure_plane(x, &x->d_period_counts, (size_t)x->cfg.max_views * 4);
    if (rc) return rc;
    const PeriodPlanes b = {x->d_period_jump, wide ? x->d_period_wide : nullptr, x->d_period_counts + 4 * (size_t)view + 2 * (size_t)axis};
    return launched(x, launch_period_repair(x->P, view, axis, radius, b, x->stream));
}

extern "C" int sl3d_repair_periods(sl3d_ctx *x, int view, int axis, int radius, uint32_t counts[2])
try {
    if (!x) return SL3D_E_INVALID_ARG;
    const int status = period_check_args(view, x->cfg.max_views, x->keep, axis, radius, x->P.Nv, x->P.Nh);
    if (status) {  // (nothing has been touched; the first two refusals in the words of every stage entry point)
        int rc = check_view(x, view);
        if (rc || (rc = need_keep(x))) return rc;
        if (status == SL3D_E_UNSUPPORTED) return fail(x, status, "repair_periods: the axis has no Gray planes (n_gray == 0), there is no period to repair");
        return fail(x, status, axis != 0 && axis != 1 ? "axis must be 0 or 1" : "repair_periods: radius must be 1..8");
    }
    if (x->anchor)  // (nothing has been touched)
        return fail(x, SL3D_E_UNSUPPORTED,
                    "repair_periods: not on a SL3D_FLAG_ANCHOR_PERIODS context: the repair turns code from the Gray cell into a fringe index, which leaves "
                    "nothing to anchor to (create the context without SL3D_FLAG_ANCHOR_PERIODS to repair instead)");
    int rc = one_axis_serves(x, axis, "repair_periods");  // (nothing has been touched)
    if (rc) return rc;
    ON_DEVICE(x);
    if ((rc = ensure_plane(x, &x->d_period_counts, (size_t)x->cfg.max_views * 4))) return rc;
    unsigned *cnt = x->d_period_counts + 4 * (size_t)view + 2 * (size_t)axis;
    HIPCHK(x, hipMemsetAsync(cnt, 0, 2 * sizeof(unsigned), x->stream));
    if ((rc = period_repair_enqueue(x, view, axis, radius))) return rc;
    if (counts) {
        HIPCHK(x, hipMemcpyAsync(counts, cnt, 2 * sizeof(unsigned), hipMemcpyDeviceToHost, x->stream));
        SYNC_FOR_CALLER(x);
    }
    return SL3D_OK;
}
SL3D_CATCH(x)
