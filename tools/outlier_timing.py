"""The radius outlier filter (sl3d_filter_outliers, k_outlier_support<RADIUS> then k_outlier_apply) at 1920x1080 over 1 and 16
synthetic views, radius 1, 2 and 4, timed with the context's HIP events (sl3d_timer_start / sl3d_timer_stop around the asynchronous call,
counts == NULL): the median of --reps calls after 10.  Every timed call is preceded, outside the timer, by sl3d_run over the same views, so
each call filters the unfiltered scan.  max_dist is 1.25 * radius median distances between row neighbours, min_neighbours 40 % of the
neighbourhood: a setting that rejects the window's border and the decode's stragglers; the share rejected is recorded.  min_neighbours = 0
(the support launch alone) is timed too.  Beside it, on the same context and the same views, timed the same way:
  run_us         sl3d_run
  mesh_views_us  sl3d_mesh_views at max_edge = +inf (the call ends in its own read-back of the counts: the events span it)
There is no bar to meet.  Before anything is timed the counts of one call are checked against the valid planes (samples on entry = valid
pixels before, rejected = valid pixels lost); a difference ends the tool with an error.
Not measured: hardware counters (LDS and fp64-VALU utilisation, bank conflicts), other sizes, other tile shapes, sparse selections, the
symmetric form that evaluates a pair once.
Written to --out (default profiles/outlier_timing.json) and printed.  usage: outlier_timing.py [--reps N] [--out PATH]"""
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

W, H, N, FW = 1920, 1080, 10, 2
VIEWS = (1, 16)
RADII = (1, 2, 4)
WARMUP = 10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "outlier_timing.json"))
    a = ap.parse_args()
    syn = importlib.import_module("3dscan_amd.synth")
    scm = importlib.import_module("3dscan_amd.scanner")
    out = {"tool": "outlier_timing", "size": [W, H], "n_gray": N, "reps": a.reps, "warmup": WARMUP,
           "timer": "HIP events around the asynchronous call, median over the repetitions; sl3d_run over the views before every timed call, outside the timer",
           "not_measured": ["hardware counters", "other sizes", "other tile shapes", "sparse selections", "the symmetric form"], "runs": []}

    def timed(sc, call, before=None):
        t = []
        for rep in range(a.reps + WARMUP):
            if before:
                before()
            sc.timer_start()
            call()
            ms = sc.timer_stop()
            if rep >= WARMUP:
                t.append(ms * 1e3)
        return round(float(np.median(t)), 2), [round(float(np.percentile(t, q)), 2) for q in (10, 90)]

    with scm.Scanner(W, H, W, H, N, N, FW, FW, max_views=max(VIEWS)) as sc:
        sc.set_calibration(*syn.cal_tuple(syn.synth_rig(W, H, W, H)))
        for v in range(max(VIEWS)):
            sc.synth_view(v, noise=1, view_id=v)
        sc.set_masks(syn.default_mask(W, H))
        sc.run(0, max(VIEWS))
        xyz, valid = sc.points(0)
        both = (valid[:, 1:] == 1) & (valid[:, :-1] == 1)
        spacing = float(np.median(np.linalg.norm(xyz[:, 1:].astype(np.float64) - xyz[:, :-1], axis=-1)[both]))
        out["pixel_spacing_mm"] = round(spacing, 5)
        for n in VIEWS:
            run_us, run_p = timed(sc, lambda: sc.run(0, n))
            mesh_us, mesh_p = timed(sc, lambda: sc.mesh_device(float("inf"), 0, n))
            for radius in RADII:
                max_dist = float(np.float32(1.25 * radius * spacing))
                min_n = int(0.4 * ((2 * radius + 1) ** 2 - 1))
                sc.run(0, n)
                before = sum(int((sc.points(v)[1] == 1).sum()) for v in range(n))
                counts = sc.filter_outliers(radius, max_dist, min_n, 0, n)
                after = sum(int((sc.points(v)[1] == 1).sum()) for v in range(n))
                if int(counts[:, 0].sum()) != before or int(counts[:, 1].sum()) != before - after:
                    sys.exit(f"radius {radius}, {n} views: the counts {counts.sum(axis=0).tolist()} and the valid planes ({before} -> {after}) disagree")
                us, p = timed(sc, lambda: sc.filter_outliers(radius, max_dist, min_n, 0, n, counts=False), before=lambda: sc.run(0, n))
                sup_us, sup_p = timed(sc, lambda: sc.filter_outliers(radius, max_dist, 0, 0, n, counts=False), before=lambda: sc.run(0, n))
                out["runs"].append({"views": n, "radius": radius, "max_dist": round(max_dist, 5), "min_neighbours": min_n,
                                    "filter_us": us, "filter_us_p10_p90": p, "support_only_us": sup_us, "support_only_us_p10_p90": sup_p,
                                    "run_us": run_us, "run_us_p10_p90": run_p, "mesh_views_us": mesh_us, "mesh_views_us_p10_p90": mesh_p,
                                    "filter_over_run": round(us / run_us, 3), "filter_over_mesh_views": round(us / mesh_us, 3),
                                    "ns_per_sample": round(us * 1e3 / max(before, 1), 4),
                                    "samples": before, "share_rejected": round((before - after) / max(before, 1), 5)})
    with open(a.out, "w") as f:
        f.write(json.dumps(out) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
