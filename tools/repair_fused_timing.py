"""The period-repaired scan of a timed context (SL3D_FLAG_REPAIR_PERIODS) at 1920x1080 with 10 Gray planes per axis, over 1 and
over 16 views, in integer and in sub-pixel mode; per mode three routes alternating in one process, each timed with its context's HIP events
(sl3d_timer_start / sl3d_timer_stop around the asynchronous calls):
  (a) fused      sl3d_run on a SL3D_FLAG_REPAIR_PERIODS context (sub-pixel mode: | SL3D_FLAG_SUBPIXEL): one launch of k_repair_fused
  (b) staged     the only route to the same planes without the flag: on a SL3D_FLAG_KEEP_STAGES context, per view two
                 sl3d_compute_wrapped_phase, two sl3d_unwrap_phase, two sl3d_repair_periods(radius 4, no counts) and one
                 sl3d_compute_c_p_map, then sl3d_triangulate per view (sub-pixel mode: ONE sl3d_triangulate_subpixel(+inf, NULL) over all views)
  (c) unflagged  sl3d_run on a timed context without the flag: the unrepaired scan, for scale -- integer mode: a k_fused instantiation
                 (SL3D_FLAG_SERIAL_LAUNCHES: the time of a lone launch on the context's stream, as (a)'s is); sub-pixel mode: k_subpixel_fused
Before anything is timed the points and valid planes (sub-pixel mode: and the residual planes) of (a) and (b) of all 16 views are compared
bit for bit; a difference ends the tool with an error.  Every shape is warmed up; the medians over the repetitions are reported, with
(a) / (b), (a) / (c) and the bytes the design moves per pixel and view in (a) -- 1.31 x (2 F + 2 (Nv + Nh)) frame bytes (the tile's halo) and
the valid byte read, 12 (+ 4) + 1 written -- over its time.
The capture: synthetic 1080p views (fringe width 16, camera noise +-2, synth_rig: an undistorted projector), the plane tilted differently
per view, generated on the device with the same arguments on every context; the staged route's counts of one pass over them are reported
(what there was to repair).
Written to --out (default profiles/repair_fused_timing.json) and printed.  usage: repair_fused_timing.py [--reps N] [--out PATH]"""
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

W, H, N, FW, F = 1920, 1080, 10, 16, 3
VIEWS = (1, 16)
WARMUP = 5
RADIUS = 4
HALO = (72 * 16 + 64 * 24) / (2.0 * 64 * 16)   # decodes per axis and pixel of a 64 x 16 tile: 1.3125


def _bits(a):
    return a.view(np.uint32 if a.dtype == np.float32 else a.dtype)


def staged(sc, n_views, subpixel, counts=None):
    for v in range(n_views):
        for axis in (0, 1):
            sc.compute_wrapped_phase(axis, v)
        for axis in (0, 1):
            sc.unwrap_phase(axis, v)
        for axis in (0, 1):
            c = sc.repair_periods(axis, RADIUS, v, want_counts=counts is not None)
            if counts is not None:
                counts[0] += c[0]
                counts[1] += c[1]
        sc.compute_c_p_map(v)
        if not subpixel:
            sc.triangulate(v)
    if subpixel:
        sc.triangulate_subpixel(0, n_views, want_counts=False)


def measure(mode, reps, syn, scm):
    sub = mode == "subpixel"
    V = max(VIEWS)
    bytes_px = (HALO * (2 * F + 4 * N) + 1, 12 + (4 if sub else 0) + 1)
    out = {"mode": mode, "model_bytes_per_pixel_read_written": [round(b, 2) for b in bytes_px], "runs": []}
    common = dict(max_views=V)
    with scm.Scanner(W, H, W, H, N, N, FW, FW, repaired=True, subpixel=sub, **common) as fused, \
            scm.Scanner(W, H, W, H, N, N, FW, FW, keep_stages=True, **common) as keep, \
            scm.Scanner(W, H, W, H, N, N, FW, FW, subpixel=sub, serial_launches=not sub, **common) as plain:
        for sc in (fused, keep, plain):
            sc.set_calibration(*syn.cal_tuple(syn.synth_rig(W, H, W, H)))
            for v in range(V):
                sc.synth_view(v, plane=(0.0, 0.05 - 0.005 * v, 0.05 + 0.003 * v), noise=2)
                sc.set_mask(syn.default_mask(W, H), view=v)
        out["kernel"] = fused.fused_kernel_name(1)
        out["unflagged_kernels"] = {str(n): plain.fused_kernel_name(n) for n in VIEWS}
        # the planes of (a) and (b), bit for bit, before anything is timed
        fused.run(0, V)
        counts = [0, 0]
        staged(keep, V, sub, counts)
        n_valid = 0
        for v in range(V):
            (xa, va), (xb, vb) = fused.points(v), keep.points(v)
            same = np.array_equal(va, vb) and np.array_equal(_bits(xa), _bits(xb))
            if sub:
                same = same and np.array_equal(_bits(fused.residuals(v)), _bits(keep.residuals(v)))
            if not same:
                sys.exit(f"{mode}, view {v}: the fused launch and the staged route differ "
                         f"(valid {int((va != vb).sum())}, points {int((_bits(xa) != _bits(xb)).sum())} elements)")
            n_valid += int((va == 1).sum())
        out["planes_equal_bit_for_bit"] = True
        out["valid_pixels"] = n_valid
        out["staged_counts_repaired_unrepairable"] = counts
        for n_views in VIEWS:
            t = {"fused": [], "staged": [], "unflagged": []}
            for rep in range(reps + WARMUP):
                fused.timer_start()
                fused.run(0, n_views)
                ta = fused.timer_stop()
                keep.timer_start()
                staged(keep, n_views, sub)
                tb = keep.timer_stop()
                plain.timer_start()
                plain.run(0, n_views)
                tc = plain.timer_stop()
                if rep >= WARMUP:
                    t["fused"].append(ta)
                    t["staged"].append(tb)
                    t["unflagged"].append(tc)
            med = {k: float(np.median(v)) * 1e3 for k, v in t.items()}
            px = W * H * n_views
            run = {"views": n_views}
            for k, v in t.items():
                run[k + "_us"] = round(med[k], 2)
                run[k + "_us_p10_p90"] = [round(float(np.percentile(v, q)) * 1e3, 2) for q in (10, 90)]
            run.update({"fused_over_staged": round(med["fused"] / med["staged"], 3), "fused_over_unflagged": round(med["fused"] / med["unflagged"], 3),
                        "fused_us_per_view": round(med["fused"] / n_views, 2), "fused_model_bytes": int(sum(bytes_px) * px),
                        "fused_model_tbs": round(sum(bytes_px) * px / (med["fused"] * 1e-6) / 1e12, 3),
                        "fused_below_staged": med["fused"] < med["staged"]})
            out["runs"].append(run)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "repair_fused_timing.json"))
    a = ap.parse_args()
    syn = importlib.import_module("3dscan_amd.synth")
    scm = importlib.import_module("3dscan_amd.scanner")
    out = {"tool": "repair_fused_timing", "size": [W, H], "n_gray": N, "fringe_width": FW, "noise": 2, "radius": RADIUS, "reps": a.reps,
           "timer": "HIP events around the asynchronous calls, median over the repetitions, the three routes alternating",
           "not_measured": "hardware counters, other sizes, a distorted projector or camera, masks other than the default",
           "modes": [measure(mode, a.reps, syn, scm) for mode in ("integer", "subpixel")]}
    with open(a.out, "w") as f:
        f.write(json.dumps(out) + "\n")
    print(json.dumps(out))
    if not all(r["fused_below_staged"] for m in out["modes"] for r in m["runs"]):
        sys.exit("the fused launch is not below the staged route in every mode")


if __name__ == "__main__":
    main()
