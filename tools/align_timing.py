"""One correspondence pass of the turntable refinement (sl3d_align_sums -- the memset of the pairs' records and k_align_pass<WINDOW>)
and a whole sl3d_refine_turntable of 10 iterations over synthetic 1920x1080 views: one pair (2 views) and 15 pairs (16 views), windows 1, 2
and 4.  The views are one noisy plane seen 16 times, the estimate a step of 0.5 degrees about the vertical through the centroid of view 0:
every source lands within a few pixels of its own pixel, as on a turntable whose step is known roughly.

Per case: the pass between the context's HIP events (sl3d_timer_start / sl3d_timer_stop around the asynchronous call, sums == NULL), the
median of --reps calls after 5; the refinement by the host's clock around the synchronous call (it downloads the words of every pass),
the median of 5 calls after 1.  Beside them, on the same context over the same views and timed by the same events: the support launch
of sl3d_filter_outliers at radius = window (min_neighbours 0, no counts: k_outlier_support alone, the library's other neighbourhood
gather) and sl3d_register_views.  On one pair the words are held against the NumPy restatement (tests/align_reference.py) at window 1
before anything is timed.
There is no bar to meet.  Not measured: hardware counters (cache hit rates of the gather, atomic requests), other sizes, real turntable
steps (20 degrees and more move the footprints of a wave apart), windows 0 and 3, scenes with large invalid regions.
Written to --out (default profiles/align_timing.json) and printed.  usage: align_timing.py [--reps N] [--out PATH]"""
import argparse
import ctypes as C
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
W, H, N, FW = 1920, 1080, 10, 2
VIEWS = (2, 16)
WINDOWS = (1, 2, 4)
WARMUP = 5
STEP_DEG, RANGE, ITERATIONS = 0.5, 256.0, 10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "align_timing.json"))
    a = ap.parse_args()
    import numpy as np
    try:
        import torch  # noqa: F401  (its ROCm stack first, as tests/conftest.py)
    except Exception:
        pass
    import align_reference as AR
    syn = importlib.import_module("3dscan_amd.synth")
    scm = importlib.import_module("3dscan_amd.scanner")

    def timed(sc, call):
        t = []
        for rep in range(a.reps + WARMUP):
            sc.timer_start()
            call()
            ms = sc.timer_stop()
            if rep >= WARMUP:
                t.append(ms * 1e3)
        return round(float(np.median(t)), 2), [round(float(np.percentile(t, q)), 2) for q in (10, 90)]

    runs = []
    with scm.Scanner(W, H, W, H, N, N, FW, FW, max_views=max(VIEWS)) as sc:
        L = sc.L
        sc.set_calibration(*syn.cal_tuple(syn.synth_rig(W, H, W, H)))
        for v in range(max(VIEWS)):
            sc.synth_view(v, noise=1, view_id=v)
        sc.set_masks(syn.default_mask(W, H))
        sc.run(0, max(VIEWS))
        views = [sc.points(v) for v in range(2)]
        xyz, valid = views[0]
        both = (valid[:, 1:] == 1) & (valid[:, :-1] == 1)
        spacing = float(np.median(np.linalg.norm(xyz[:, 1:].astype(np.float64) - xyz[:, :-1], axis=-1)[both]))
        axis = [float(v) for v in xyz[valid == 1].astype(np.float64).mean(axis=0)]
        max_dist = float(np.float32(4.0 * spacing))
        est = AR.estimate(STEP_DEG, axis[0], axis[2])
        rot = float(AR.degrees_22_7(STEP_DEG))
        got = sc.align_sums(0, 2, est, axis[0], axis[2], RANGE, max_dist, 1)
        want = AR.pass_sums(np.stack([p for p, _ in views]), np.stack([m for _, m in views]), sc.align_camera(), 0, 0, est, axis[0], axis[2], RANGE,
                            max_dist, 1)
        if not np.array_equal(got, want):
            sys.exit("align_timing: the words of a pass differ from the restatement")
        total = C.c_int64(0)
        e = np.ascontiguousarray(est)
        for n in VIEWS:
            def register():
                sc._chk(L.sl3d_register_views(sc._h, 0, n, axis[0], axis[1], axis[2], rot, None, 0, C.byref(total)), "sl3d_register_views")
            reg_us, reg_p = timed(sc, register)
            for w in WINDOWS:
                words = sc.align_sums(0, n, est, axis[0], axis[2], RANGE, max_dist, w)
                pass_us, pass_p = timed(sc, lambda: sc._chk(L.sl3d_align_sums(sc._h, 0, n, e.ctypes.data, axis[0], axis[2], RANGE, max_dist, w, None),
                                                            "sl3d_align_sums"))
                sup_us, sup_p = timed(sc, lambda: sc._chk(L.sl3d_filter_outliers(sc._h, 0, n, w, max_dist, 0, None), "sl3d_filter_outliers"))
                wall, done = [], 0
                for rep in range(6):
                    t0 = time.perf_counter()
                    out = sc.refine_turntable(0, n, axis[0], axis[1], axis[2], rot, RANGE, max_dist, w, ITERATIONS)
                    wall.append((time.perf_counter() - t0) * 1e6)
                    done = out["n_done"]
                pairs, px = n - 1, (n - 1) * W * H
                runs.append({"views": n, "pairs": pairs, "window": w, "accepted": int(words[:, 0].sum()), "sources": int(words[:, 11].sum()),
                             "pass_us": pass_us, "pass_us_p10_p90": pass_p, "pass_ns_per_source_pixel": round(pass_us * 1e3 / px, 4),
                             "outlier_support_us": sup_us, "outlier_support_us_p10_p90": sup_p, "outlier_support_views": n,
                             "pass_per_pair_over_support_per_view": round((pass_us / pairs) / (sup_us / n), 3),
                             "refine_iterations_asked": ITERATIONS, "refine_iterations_made": done, "refine_wall_us": round(float(np.median(wall[1:])), 1),
                             "refine_wall_us_per_iteration": round(float(np.median(wall[1:])) / max(done, 1), 1),
                             "register_views_us": reg_us, "register_views_us_p10_p90": reg_p})
    out = {"tool": "align_timing", "size": [W, H], "n_gray": N, "reps": a.reps, "warmup": WARMUP, "step_deg": STEP_DEG, "range": RANGE,
           "max_dist_mm": round(max_dist, 5), "pixel_spacing_mm": round(spacing, 5), "axis": [round(v, 3) for v in axis],
           "timer": "HIP events around the asynchronous call (sums == NULL; the outlier filter: min_neighbours 0, counts == NULL, its support launch "
                    "alone), medians over the repetitions; refine_wall_us: the host's clock around the synchronous call, median of 5 after 1; "
                    "register_views_us includes its compaction and its read-back of the counts",
           "not_measured": ["hardware counters", "other sizes", "steps of 20 degrees and more", "windows 0 and 3", "scenes with large invalid regions"],
           "runs": runs}
    with open(a.out, "w") as f:
        f.write(json.dumps(out) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
