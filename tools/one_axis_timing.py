"""The one-axis scan of a timed context (SL3D_FLAG_SUBPIXEL | SL3D_FLAG_ANCHOR_PERIODS | SL3D_FLAG_ONLY_VERTICAL) at 1920x1080, over 1 and
over 16 views, against the two-axis anchored sub-pixel scan of the same build, alternating in one process, each timed with its context's HIP
events (sl3d_timer_start / sl3d_timer_stop around the asynchronous call):
  (a) one_axis  sl3d_run on a SL3D_FLAG_SUBPIXEL | SL3D_FLAG_ANCHOR_PERIODS | SL3D_FLAG_ONLY_VERTICAL context: one launch of k_one_axis<0, true>
  (b) two_axes  sl3d_run on a SL3D_FLAG_SUBPIXEL | SL3D_FLAG_ANCHOR_PERIODS context: one launch of k_subpixel_fused<true>
Before anything is timed the points and valid planes of (a) over all 16 views are compared bit for bit with the staged route on a
SL3D_FLAG_KEEP_STAGES context with the same flags (per view sl3d_compute_wrapped_phase and sl3d_unwrap_phase of the vertical axis and
sl3d_compute_c_p_map, then one sl3d_triangulate_subpixel(+inf, NULL) over all views); a difference ends the tool with an error.  Every shape
is warmed up; the medians over the repetitions are reported with p10 / p90 and the ratio (a) / (b).  Required: (a) below (b) at both view
counts -- (a) does strictly less; the estimate from the bytes alone is 35 / 52 = 0.67.  The tool ends with an error if (a) is not below (b).
The capture: synthetic 1080p views (fringe width 16, 7 Gray planes per axis, camera noise +-2, synth_rig: an undistorted projector with a
horizontal baseline), the plane tilted differently per view, generated on the device with the same arguments on every context.
Not measured: other sizes, 10 Gray planes, the horizontal form, hardware counters, the host pipeline's rate.
Written to --out (default profiles/one_axis_timing.json) and printed.  usage: one_axis_timing.py [--reps N] [--out PATH]"""
import argparse
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

try:
    import torch  # noqa: F401  (its ROCm stack first, as tests/conftest.py)
except Exception:
    pass

W, H, N, FW, F = 1920, 1080, 7, 16, 3
VIEWS = (1, 16)
WARMUP = 10


def _bits(a):
    return a.view(np.uint32 if a.dtype == np.float32 else a.dtype)


def staged(sc, n_views):
    for v in range(n_views):
        sc.compute_wrapped_phase(0, v)
        sc.unwrap_phase(0, v)
        sc.compute_c_p_map(v)
    sc.triangulate_subpixel(0, n_views, want_counts=False)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "one_axis_timing.json"))
    a = ap.parse_args()
    syn = importlib.import_module("3dscan_amd.synth")
    scm = importlib.import_module("3dscan_amd.scanner")
    V = max(VIEWS)
    out = {"tool": "one_axis_timing", "size": [W, H], "n_gray": N, "fringe_width": FW, "noise": 2, "reps": a.reps,
           "timer": "HIP events around the asynchronous call, median over the repetitions, the two routes alternating",
           "estimate_from_bytes_one_axis_over_two_axes": round(35 / 52, 3),
           "not_measured": ["other sizes", "n_gray = 10", "the horizontal form", "hardware counters", "the host pipeline's rate"], "runs": []}
    common = dict(max_views=V, subpixel=True, anchored=True)

    def prepare(sc):
        sc.set_calibration(*syn.cal_tuple(syn.synth_rig(W, H, W, H)))
        for v in range(V):
            sc.synth_view(v, plane=(0.0, 0.05 - 0.005 * v, 0.05 + 0.003 * v), noise=2)
            sc.set_mask(syn.default_mask(W, H), view=v)

    with scm.Scanner(W, H, W, H, N, N, FW, FW, only_axis=0, **common) as one, scm.Scanner(W, H, W, H, N, N, FW, FW, **common) as two:
        for sc in (one, two):
            prepare(sc)
        out["kernels"] = {"one_axis": one.fused_kernel_name(1), "two_axes": two.fused_kernel_name(1)}
        # the planes of (a) against the staged route, bit for bit, before anything is timed
        one.run(0, V)
        two.run(0, V)
        n_valid = n_both = 0
        with scm.Scanner(W, H, W, H, N, N, FW, FW, keep_stages=True, only_axis=0, **common) as keep:
            prepare(keep)
            staged(keep, V)
            for v in range(V):
                (xa, va), (xb, vb), (_, vc) = one.points(v), keep.points(v), two.points(v)
                if not (np.array_equal(va, vb) and np.array_equal(_bits(xa), _bits(xb))):
                    sys.exit(f"view {v}: the one-axis launch and the staged route differ (valid {int((va != vb).sum())}, points {int((_bits(xa) != _bits(xb)).sum())} elements)")
                if ((vc == 1) & (va != 1)).any():
                    sys.exit(f"view {v}: the one-axis scan lost {int(((vc == 1) & (va != 1)).sum())} pixels the two-axis scan keeps")
                n_valid += int((va == 1).sum())
                n_both += int((vc == 1).sum())
        out["planes_equal_bit_for_bit"] = True
        out["valid_pixels"] = {"one_axis": n_valid, "two_axes": n_both}
        ok = True
        for n_views in VIEWS:
            t = {"one_axis": [], "two_axes": []}
            for rep in range(a.reps + WARMUP):
                one.timer_start()
                one.run(0, n_views)
                ta = one.timer_stop()
                two.timer_start()
                two.run(0, n_views)
                tb = two.timer_stop()
                if rep >= WARMUP:
                    t["one_axis"].append(ta)
                    t["two_axes"].append(tb)
            med = {k: float(np.median(v)) * 1e3 for k, v in t.items()}
            run = {"views": n_views}
            for k, v in t.items():
                run[k + "_us"] = round(med[k], 2)
                run[k + "_us_p10_p90"] = [round(float(np.percentile(v, q)) * 1e3, 2) for q in (10, 90)]
            run.update({"one_axis_over_two_axes": round(med["one_axis"] / med["two_axes"], 3), "one_axis_is_faster": med["one_axis"] < med["two_axes"]})
            ok = ok and run["one_axis_is_faster"]
            out["runs"].append(run)
    with open(a.out, "w") as f:
        f.write(json.dumps(out) + "\n")
    print(json.dumps(out))
    if not ok:
        sys.exit("the one-axis launch is not faster than the two-axis launch")


if __name__ == "__main__":
    main()
