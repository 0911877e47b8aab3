"""The sub-pixel scan of a timed context (SL3D_FLAG_SUBPIXEL) at 1920x1080, over 1 and over 16 views, three routes alternating in
one process, each timed with its context's HIP events (sl3d_timer_start / sl3d_timer_stop around the asynchronous calls):
  (a) fused    sl3d_run on a SL3D_FLAG_SUBPIXEL context: one launch of k_subpixel_fused
  (b) staged   the only route to the same planes without the flag: on a SL3D_FLAG_KEEP_STAGES context, per view two
               sl3d_compute_wrapped_phase, two sl3d_unwrap_phase and one sl3d_compute_c_p_map, then ONE sl3d_triangulate_subpixel(+inf, NULL)
               over all views
  (c) integer  sl3d_run on a timed context without the flag (SL3D_FLAG_SERIAL_LAUNCHES: the time of a lone launch on the context's
               stream, as (a)'s is): the integer scan, for scale
Before anything is timed the points, valid and residual planes of (a) and (b) of all 16 views are compared bit for bit; a difference
ends the tool with an error.  Every shape is warmed up; the medians over the repetitions are reported, with (a) / (b), (a) / (c) and the
bytes the design moves per pixel and view in (a) -- 2 F + 2 (Nv + Nh) frame bytes and the valid byte read, 12 + 4 + 1 written -- over its time.
The capture: synthetic 1080p views (fringe width 16, 7 Gray planes per axis, camera noise +-2, synth_rig: an undistorted projector), the
plane tilted differently per view, generated on the device with the same arguments on every context.
Written to --out (default profiles/subpixel_fused_timing.json) and printed.  usage: subpixel_fused_timing.py [--reps N] [--out PATH]"""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "subpixel_fused_timing.json"))
    a = ap.parse_args()
    syn = importlib.import_module("3dscan_amd.synth")
    scm = importlib.import_module("3dscan_amd.scanner")
    V = max(VIEWS)
    bytes_px = (2 * F + 4 * N + 1, 12 + 4 + 1)
    out = {"tool": "subpixel_fused_timing", "size": [W, H], "n_gray": N, "fringe_width": FW, "noise": 2, "reps": a.reps,
           "timer": "HIP events around the asynchronous calls, median over the repetitions, the three routes alternating",
           "model_bytes_per_pixel_read_written": list(bytes_px), "runs": []}
    common = dict(max_views=V)
    with scm.Scanner(W, H, W, H, N, N, FW, FW, subpixel=True, **common) as fused, \
            scm.Scanner(W, H, W, H, N, N, FW, FW, keep_stages=True, **common) as keep, \
            scm.Scanner(W, H, W, H, N, N, FW, FW, serial_launches=True, **common) as integer:
        ctxs = (fused, keep, integer)
        for sc in ctxs:
            sc.set_calibration(*syn.cal_tuple(syn.synth_rig(W, H, W, H)))
            for v in range(V):
                sc.synth_view(v, plane=(0.0, 0.05 - 0.005 * v, 0.05 + 0.003 * v), noise=2)
                sc.set_mask(syn.default_mask(W, H), view=v)
        out["kernel"] = fused.fused_kernel_name(1)
        out["integer_kernels"] = {str(n): integer.fused_kernel_name(n) for n in VIEWS}
        # the planes of (a) and (b), bit for bit, before anything is timed
        fused.run(0, V)
        staged(keep, V)
        n_valid = 0
        for v in range(V):
            (xa, va), (xb, vb) = fused.points(v), keep.points(v)
            ra, rb = fused.residuals(v), keep.residuals(v)
            if not (np.array_equal(va, vb) and np.array_equal(_bits(xa), _bits(xb)) and np.array_equal(_bits(ra), _bits(rb))):
                sys.exit(f"view {v}: the fused launch and the staged route differ "
                         f"(valid {int((va != vb).sum())}, points {int((_bits(xa) != _bits(xb)).sum())}, residuals {int((_bits(ra) != _bits(rb)).sum())} elements)")
            n_valid += int((va == 1).sum())
        out["planes_equal_bit_for_bit"] = True
        out["valid_pixels"] = n_valid
        for n_views in VIEWS:
            t = {"fused": [], "staged": [], "integer": []}
            for rep in range(a.reps + WARMUP):
                fused.timer_start()
                fused.run(0, n_views)
                ta = fused.timer_stop()
                keep.timer_start()
                staged(keep, n_views)
                tb = keep.timer_stop()
                integer.timer_start()
                integer.run(0, n_views)
                tc = integer.timer_stop()
                if rep >= WARMUP:
                    t["fused"].append(ta)
                    t["staged"].append(tb)
                    t["integer"].append(tc)
            med = {k: float(np.median(v)) * 1e3 for k, v in t.items()}
            px = W * H * n_views
            run = {"views": n_views}
            for k, v in t.items():
                run[k + "_us"] = round(med[k], 2)
                run[k + "_us_p10_p90"] = [round(float(np.percentile(v, q)) * 1e3, 2) for q in (10, 90)]
            run.update({"fused_over_staged": round(med["fused"] / med["staged"], 3), "fused_over_integer": round(med["fused"] / med["integer"], 3),
                        "fused_us_per_view": round(med["fused"] / n_views, 2), "fused_model_bytes": sum(bytes_px) * px,
                        "fused_model_tbs": round(sum(bytes_px) * px / (med["fused"] * 1e-6) / 1e12, 3),
                        "fused_below_staged": med["fused"] < med["staged"]})
            out["runs"].append(run)
    with open(a.out, "w") as f:
        f.write(json.dumps(out) + "\n")
    print(json.dumps(out))
    if not all(r["fused_below_staged"] for r in out["runs"]):
        sys.exit("the fused launch is not below the staged route")


if __name__ == "__main__":
    main()
