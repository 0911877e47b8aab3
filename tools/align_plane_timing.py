"""The point-to-plane turntable refinement over synthetic 1920x1080 views: one pair (2 views) and 15 pairs (16 views), windows 1,
2 and 4.  The views are one noisy plane seen 16 times with a smooth bump of 3 mm laid over it through tests/dense_planes.put_dense (a
single plane would leave the solve degenerate and end the loop after one pass); the estimate is a step of 0.5 degrees about the vertical
through the centroid of view 0, as in tools/align_timing.py.

Per case, between the context's HIP events (sl3d_timer_start / sl3d_timer_stop around the asynchronous call), alternating within one
loop so that drift hits all alike, the median of --reps rounds after 5:
  normals_us       sl3d_align_normals over the pairs' target views (k_align_normals alone)
  plane_sums_us    sl3d_align_plane_sums with sums == NULL: the normals launch, the memset of the records and k_align_plane_pass<WINDOW>
  plane_pass_us    plane_sums_us - normals_us: the pass alone (a difference of two medians, not a measurement of its own)
  parent_pass_us   sl3d_align_sums with sums == NULL: the memset and k_align_pass<WINDOW> of the point-to-point form, in the same session
and the ratios plane_pass_us / parent_pass_us and plane_pass_us / (parent_pass_us + normals_us).  A whole sl3d_refine_turntable_plane of 5
iterations by the host's clock around the synchronous call (normals once, then per iteration a pass, the download of its words and the
solve), the median of 5 calls after 1, with the iterations it made.  On one pair the words are held against the NumPy restatement
(tests/align_plane_reference.py) at window 1 before anything is timed.
There is no bar to meet.  Not measured: hardware counters (none were collected: cache hit rates of the gather and of the stencil, atomic
requests), other sizes, real turntable steps, windows 0 and 3, scenes with large invalid regions.
Written to --out (default profiles/align_plane_timing.json) and printed.  usage: align_plane_timing.py [--reps N] [--out PATH]"""
import argparse
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
STEP_DEG, RANGE, ITERATIONS, BUMP_MM = 0.5, 256.0, 5, 3.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "align_plane_timing.json"))
    a = ap.parse_args()
    import numpy as np
    try:
        import torch  # noqa: F401  (its ROCm stack first, as tests/conftest.py)
    except Exception:
        pass
    import align_plane_reference as PR
    import align_reference as AR
    from dense_planes import put_dense
    syn = importlib.import_module("3dscan_amd.synth")
    scm = importlib.import_module("3dscan_amd.scanner")

    def event_us(sc, call):
        sc.timer_start()
        call()
        return sc.timer_stop() * 1e3

    def stats(t):
        return round(float(np.median(t)), 2), [round(float(np.percentile(t, q)), 2) for q in (10, 90)]

    runs = []
    with scm.Scanner(W, H, W, H, N, N, FW, FW, max_views=max(VIEWS)) as sc:
        L = sc.L
        sc.set_calibration(*syn.cal_tuple(syn.synth_rig(W, H, W, H)))
        for v in range(max(VIEWS)):
            sc.synth_view(v, noise=1, view_id=v)
        sc.set_masks(syn.default_mask(W, H))
        sc.run(0, max(VIEWS))
        sc.synchronize()
        r, c = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        bump = (BUMP_MM * np.sin(2.0 * np.pi * c / 400.0) * np.cos(2.0 * np.pi * r / 300.0)).astype(np.float32)
        views = []
        for v in range(max(VIEWS)):
            xyz, valid = sc.points(v)
            xyz = xyz.copy()
            xyz[..., 2] += bump
            put_dense(sc, v, xyz, valid, pad_xyz=np.float32(0.0), pad_valid=0)
            if v < 2:
                views.append((xyz, valid))
        xyz, valid = views[0]
        both = (valid[:, 1:] == 1) & (valid[:, :-1] == 1)
        spacing = float(np.median(np.linalg.norm(xyz[:, 1:].astype(np.float64) - xyz[:, :-1], axis=-1)[both]))
        axis = [float(v) for v in xyz[valid == 1].astype(np.float64).mean(axis=0)]
        max_dist, edge = float(np.float32(4.0 * spacing)), float(np.float32(4.0 * spacing))
        est = AR.estimate(STEP_DEG, axis[0], axis[2])
        rot = float(AR.degrees_22_7(STEP_DEG))
        got = sc.align_plane_sums(0, 2, est, axis[0], axis[2], RANGE, max_dist, edge, 1)
        want = PR.pass_sums(np.stack([p for p, _ in views]), np.stack([m for _, m in views]), sc.align_camera(), 0, 0, est, axis[0], axis[2], RANGE,
                            max_dist, edge, 1)
        if not np.array_equal(got, want):
            sys.exit("align_plane_timing: the words of a pass differ from the restatement")
        e = np.ascontiguousarray(est)
        for n in VIEWS:
            for w in WINDOWS:
                words = sc.align_plane_sums(0, n, est, axis[0], axis[2], RANGE, max_dist, edge, w)
                calls = {
                    "normals": lambda: sc._chk(L.sl3d_align_normals(sc._h, 0, n - 1, edge), "sl3d_align_normals"),
                    "plane_sums": lambda: sc._chk(L.sl3d_align_plane_sums(sc._h, 0, n, e.ctypes.data, axis[0], axis[2], RANGE, max_dist, edge, w, None),
                                                  "sl3d_align_plane_sums"),
                    "parent_pass": lambda: sc._chk(L.sl3d_align_sums(sc._h, 0, n, e.ctypes.data, axis[0], axis[2], RANGE, max_dist, w, None), "sl3d_align_sums"),
                }
                t = {k: [] for k in calls}
                for rep in range(a.reps + WARMUP):                          # alternating: one round times each call once
                    for k, call in calls.items():
                        us = event_us(sc, call)
                        if rep >= WARMUP:
                            t[k].append(us)
                (nrm_us, nrm_p), (sums_us, sums_p), (par_us, par_p) = (stats(t[k]) for k in ("normals", "plane_sums", "parent_pass"))
                pass_us = round(sums_us - nrm_us, 2)
                wall, done, deg = [], 0, False
                for rep in range(6):
                    t0 = time.perf_counter()
                    out = sc.refine_turntable_plane(0, n, axis[0], axis[1], axis[2], rot, RANGE, max_dist, edge, w, ITERATIONS)
                    wall.append((time.perf_counter() - t0) * 1e6)
                    done, deg = out["n_done"], out["degenerate"]
                pairs = n - 1
                runs.append({"views": n, "pairs": pairs, "window": w, "accepted": int(words[:, 0].sum()), "sources": int(words[:, 16].sum()),
                             "lost_to_missing_normal": int(words[:, 17].sum()),
                             "normals_us": nrm_us, "normals_us_p10_p90": nrm_p, "normals_views": pairs,
                             "normals_ns_per_pixel": round(nrm_us * 1e3 / (pairs * W * H), 4),
                             "plane_sums_us": sums_us, "plane_sums_us_p10_p90": sums_p, "plane_pass_us": pass_us,
                             "parent_pass_us": par_us, "parent_pass_us_p10_p90": par_p,
                             "plane_pass_over_parent_pass": round(pass_us / par_us, 3),
                             "plane_pass_over_parent_pass_plus_normals": round(pass_us / (par_us + nrm_us), 3),
                             "refine_iterations_asked": ITERATIONS, "refine_iterations_made": done, "refine_degenerate": bool(deg),
                             "refine_wall_us": round(float(np.median(wall[1:])), 1),
                             "refine_wall_us_per_iteration": round(float(np.median(wall[1:])) / max(done, 1), 1)})
    out = {"tool": "align_plane_timing", "size": [W, H], "n_gray": N, "reps": a.reps, "warmup": WARMUP, "step_deg": STEP_DEG, "range": RANGE,
           "bump_mm": BUMP_MM, "max_dist_mm": round(max_dist, 5), "normal_edge_mm": round(edge, 5), "pixel_spacing_mm": round(spacing, 5),
           "axis": [round(v, 3) for v in axis],
           "timer": "HIP events around the asynchronous call (sums == NULL), the three calls alternating within one loop, medians over the "
                    "repetitions; plane_pass_us is plane_sums_us - normals_us; refine_wall_us: the host's clock around the synchronous call, "
                    "median of 5 after 1",
           "counters": "not collected",
           "not_measured": ["hardware counters", "other sizes", "steps of 20 degrees and more", "windows 0 and 3", "scenes with large invalid regions"],
           "runs": runs}
    with open(a.out, "w") as f:
        f.write(json.dumps(out) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
