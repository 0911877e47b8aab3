"""The anchored sub-pixel scan of a timed context (SL3D_FLAG_SUBPIXEL | SL3D_FLAG_ANCHOR_PERIODS) at 1920x1080, over 1 and over 16
views, against the unflagged sub-pixel scan of the same build, alternating in one process, each timed with its context's HIP events
(sl3d_timer_start / sl3d_timer_stop around the asynchronous call):
  (a) anchored  sl3d_run on a SL3D_FLAG_SUBPIXEL | SL3D_FLAG_ANCHOR_PERIODS context: one launch of k_subpixel_fused<true>
  (b) plain     sl3d_run on a SL3D_FLAG_SUBPIXEL context: one launch of k_subpixel_fused<false>
Before anything is timed the points, valid and residual planes of (a) over all 16 views are compared bit for bit with the staged route on a
SL3D_FLAG_KEEP_STAGES | SL3D_FLAG_SUBPIXEL | SL3D_FLAG_ANCHOR_PERIODS context (per view two sl3d_compute_wrapped_phase, two sl3d_unwrap_phase
and one sl3d_compute_c_p_map, then one sl3d_triangulate_subpixel(+inf, NULL) over all views); a difference ends the tool with an error.
The valid planes of (a) and (b) must be equal too: the flag does not change validity.  Every shape is warmed up; the medians over the
repetitions are reported with p10 / p90 and the ratio (a) / (b); the expectation is at most 1.10.
The capture: synthetic 1080p views (fringe width 16, 7 Gray planes per axis, camera noise +-2, synth_rig: an undistorted projector), the
plane tilted differently per view, generated on the device with the same arguments on every context.
Written to --out (default profiles/anchor_timing.json) and printed.  usage: anchor_timing.py [--reps N] [--out PATH]"""
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
        for axis in (0, 1):
            sc.compute_wrapped_phase(axis, v)
        for axis in (0, 1):
            sc.unwrap_phase(axis, v)
        sc.compute_c_p_map(v)
    sc.triangulate_subpixel(0, n_views, want_counts=False)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "anchor_timing.json"))
    a = ap.parse_args()
    syn = importlib.import_module("3dscan_amd.synth")
    scm = importlib.import_module("3dscan_amd.scanner")
    V = max(VIEWS)
    out = {"tool": "anchor_timing", "size": [W, H], "n_gray": N, "fringe_width": FW, "noise": 2, "reps": a.reps,
           "timer": "HIP events around the asynchronous call, median over the repetitions, the two routes alternating",
           "parent_plain_us": {"1": 48.7, "16": 586.0}, "expectation_anchored_over_plain": 1.10, "runs": []}
    common = dict(max_views=V, subpixel=True)

    def prepare(sc):
        sc.set_calibration(*syn.cal_tuple(syn.synth_rig(W, H, W, H)))
        for v in range(V):
            sc.synth_view(v, plane=(0.0, 0.05 - 0.005 * v, 0.05 + 0.003 * v), noise=2)
            sc.set_mask(syn.default_mask(W, H), view=v)

    with scm.Scanner(W, H, W, H, N, N, FW, FW, anchored=True, **common) as anchored, scm.Scanner(W, H, W, H, N, N, FW, FW, **common) as plain:
        for sc in (anchored, plain):
            prepare(sc)
        out["kernels"] = {"anchored": anchored.fused_kernel_name(1), "plain": plain.fused_kernel_name(1)}
        # the planes of (a) against the staged route, bit for bit, before anything is timed
        anchored.run(0, V)
        plain.run(0, V)
        n_valid = n_moved = 0
        with scm.Scanner(W, H, W, H, N, N, FW, FW, keep_stages=True, anchored=True, **common) as keep:
            prepare(keep)
            staged(keep, V)
            for v in range(V):
                (xa, va), (xb, vb), (xc, vc) = anchored.points(v), keep.points(v), plain.points(v)
                ra, rb = anchored.residuals(v), keep.residuals(v)
                if not (np.array_equal(va, vb) and np.array_equal(_bits(xa), _bits(xb)) and np.array_equal(_bits(ra), _bits(rb))):
                    sys.exit(f"view {v}: the anchored launch and the staged route differ "
                             f"(valid {int((va != vb).sum())}, points {int((_bits(xa) != _bits(xb)).sum())}, residuals {int((_bits(ra) != _bits(rb)).sum())} elements)")
                if not np.array_equal(va, vc):
                    sys.exit(f"view {v}: the flag changed the valid map ({int((va != vc).sum())} pixels)")
                n_valid += int((va == 1).sum())
                n_moved += int(((_bits(xa) != _bits(xc)).any(-1) & (va == 1)).sum())
        out["planes_equal_bit_for_bit"] = True
        out["valid_pixels"] = n_valid
        out["valid_pixels_whose_point_differs_from_the_plain_scan"] = n_moved
        for n_views in VIEWS:
            t = {"anchored": [], "plain": []}
            for rep in range(a.reps + WARMUP):
                anchored.timer_start()
                anchored.run(0, n_views)
                ta = anchored.timer_stop()
                plain.timer_start()
                plain.run(0, n_views)
                tb = plain.timer_stop()
                if rep >= WARMUP:
                    t["anchored"].append(ta)
                    t["plain"].append(tb)
            med = {k: float(np.median(v)) * 1e3 for k, v in t.items()}
            run = {"views": n_views}
            for k, v in t.items():
                run[k + "_us"] = round(med[k], 2)
                run[k + "_us_p10_p90"] = [round(float(np.percentile(v, q)) * 1e3, 2) for q in (10, 90)]
            run.update({"anchored_over_plain": round(med["anchored"] / med["plain"], 3), "plain_over_parent": round(med["plain"] / out["parent_plain_us"][str(n_views)], 3),
                        "within_expectation": med["anchored"] <= 1.10 * med["plain"]})
            out["runs"].append(run)
    with open(a.out, "w") as f:
        f.write(json.dumps(out) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
