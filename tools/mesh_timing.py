"""sl3d_mesh_views at the BASELINE frame sizes: 1 and 16 views of 1920x1080, 3 views of 4096x3000; the default mask and the 19 % lasso;
max_edge = +inf and a value at the median of the candidates' edge lengths.  After warm-up, the host clock around REPS back-to-back calls
(every call ends in its own synchronise), per view; beside it the bytes the design moves (from the shapes and the returned counts), bytes
over time against the 6.3 TB/s achievable and the 8 TB/s peak, and -- for scale -- sl3d_compact_views on the same views (same reads,
vertices only).  One JSON line.  Under `rocprofv3 --kernel-trace --stats` (a run of its own) the kernel table gives the per-kernel split.
--normals: the normals leg instead -- sl3d_mesh_normals over the same cases, sl3d_mesh_views timed in the same process in alternating
blocks of calls so that both see the same clocks, the ratio per case (profiles/mesh_normals_timing.json).
--components: the components leg -- sl3d_mesh_components and sl3d_mesh_views_filtered (min_vertices = MIN_VERTICES) over the same cases,
each against sl3d_mesh_views in alternating blocks in the same process, the ratios and the component counts per case; written to --out
(default profiles/mesh_components_timing.json) as well as printed.
--smooth: the smoothing leg -- sl3d_mesh_smooth (10 iterations, lambda 0.5, mu -0.53: 20 steps) with both flags off and with both on,
each against sl3d_mesh_views in alternating blocks in the same process; the time per step is the difference to a run of 1 iteration
(2 steps) over the 18 steps between them, so the cell, ring, scan and output launches and the read-back cancel; written to --out (default
profiles/mesh_smooth_timing.json) as well as printed.
--lod: the level-of-detail leg -- sl3d_mesh_views_lod at steps 2, 4 and 8 without and with SL3D_LOD_MEAN (min_vertices 1) and behind the
filter (min_vertices = MIN_VERTICES), each against sl3d_mesh_views in alternating blocks in the same process, the ratio per case; one
1080p view unless --only names another configuration; written to --out (default profiles/mesh_lod_timing.json) as well as
printed.
--fill: the hole-filling leg -- sl3d_mesh_fill_holes at max_hole 16 and 256, min_vertices 1 and MIN_VERTICES, on one and on 16 views of 1080p,
the default mask and the 19 % lasso each with a seeded 1 % of their pixels knocked out, max_edge 4 and fill_edge 2 median edge lengths, each
against sl3d_mesh_views in alternating blocks in the same process, the ratio per case; written to --out (default
profiles/mesh_fill_timing.json) as well as printed.
usage: mesh_timing.py [--reps N] [--only 1080p_1|1080p_16|12mp_3] [--normals | --components | --smooth | --lod | --fill [--out PATH]]"""
import argparse
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

try:
    import torch  # noqa: F401  (its ROCm stack first, as tests/conftest.py)
except Exception:
    pass
from mesh_reference import np_mesh  # the NumPy restatement of the definition: the source of the median edge length

ACHIEVABLE_TBS, PEAK_TBS = 6.3, 8.0
CONFIGS = {"1080p_1": (1920, 1080, 1920, 1080, 1), "1080p_16": (1920, 1080, 1920, 1080, 16), "12mp_3": (4096, 3000, 2048, 2048, 3)}
N, FW = 10, 2
MIN_VERTICES = 100
SMOOTH = (10, 0.5, -0.53)  # iterations, lambda, mu of the smoothing leg
LOD_STEPS = (2, 4, 8)      # of the level-of-detail leg
FILL_MAX_HOLES = (16, 256)  # of the hole-filling leg
FILL_KNOCKED_OUT = 0.01


def lasso(W, H, share=358580.0 / 1920000.0):
    mh, mw = int(round(H * share ** 0.5)), int(round(W * share ** 0.5))
    m = np.zeros((H, W), np.uint8)
    m[(H - mh) // 2:(H - mh) // 2 + mh, (W - mw) // 2:(W - mw) // 2 + mw] = 1
    return m


def clock(fn, reps):
    for _ in range(20):
        fn()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t0) / reps


def clock_alternating(fa, fb, reps, blocks=4):
    """reps back-to-back calls of each, in `blocks` alternating blocks after one warm-up of both: seconds per call of fa, of fb"""
    for _ in range(20):
        fa()
        fb()
    ta = tb = 0.0
    per = max(1, reps // blocks)
    for _ in range(blocks):
        t0 = time.perf_counter()
        for _ in range(per):
            fa()
        t1 = time.perf_counter()
        for _ in range(per):
            fb()
        ta, tb = ta + (t1 - t0), tb + (time.perf_counter() - t1)
    return ta / (per * blocks), tb / (per * blocks)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--only", default="")
    ap.add_argument("--normals", action="store_true")
    ap.add_argument("--components", action="store_true")
    ap.add_argument("--smooth", action="store_true")
    ap.add_argument("--lod", action="store_true")
    ap.add_argument("--fill", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    a.out = a.out or os.path.join(ROOT, "profiles", "mesh_fill_timing.json" if a.fill else "mesh_lod_timing.json" if a.lod else "mesh_smooth_timing.json" if a.smooth else "mesh_components_timing.json")
    if a.lod and not a.only:
        a.only = "1080p_1"
    syn = importlib.import_module("3dscan_amd.synth")
    scm = importlib.import_module("3dscan_amd.scanner")
    if a.fill:
        out = {"tool": "mesh_timing --fill", "reps": a.reps, "max_holes": list(FILL_MAX_HOLES), "min_vertices_of_the_filtered_case": MIN_VERTICES,
               "knocked_out_share": FILL_KNOCKED_OUT, "max_edge": "4 median edges", "fill_edge": "2 median edges",
               "bytes_note": "hole kernels = init 1 B/px read + 8 written, union 2 B/px, flatten 1 B/px + 8 per non-candidate, fill 13 B per "
                             "candidate read + 17 B/px written + 5 B per non-candidate: about 32 B/px; the call adds the cell pass (14 B/px) "
                             "and the mesh's design bytes over the filled grid", "runs": []}
    elif a.lod:
        out = {"tool": "mesh_timing --lod", "reps": a.reps, "steps": list(LOD_STEPS), "min_vertices_of_the_filtered_case": MIN_VERTICES,
               "achievable_tbs": ACHIEVABLE_TBS, "peak_tbs": PEAK_TBS,
               "bytes_note": "block pass = 13 B per fine pixel read once (candidate byte + point) + 17 B per coarse pixel written; call, "
                             "min_vertices 1 = cell pass 14 B/px (13 read, cell byte written) + block pass + the fine mesh's design bytes "
                             "over the coarse grid (4 B per coarse pixel + 48 B per vertex + 12 B per vertex and face written) + 8 B per "
                             "vertex (ids)", "runs": []}
    elif a.smooth:
        out = {"tool": "mesh_timing --smooth", "reps": a.reps, "iterations": SMOOTH[0], "lambda": SMOOTH[1], "mu": SMOOTH[2],
               "achievable_tbs": ACHIEVABLE_TBS, "peak_tbs": PEAK_TBS,
               "bytes_note": "design, one step = 2 B/px (valid, ring) + 24 B per vertex (points read once, rows r-1 / r+1 counted as L2 hits, "
                             "points written)", "runs": []}
    elif a.components:
        out = {"tool": "mesh_timing --components", "reps": a.reps, "min_vertices": MIN_VERTICES,
               "bytes_note": "design, atomics not counted: components = 17 B/px (valid 3x, cell plane written + read, labels, sizes and ids "
                             "initialised) + 32 B per vertex (points once, label read + written by the flatten, label + root id read, label "
                             "written); filtered = 21 B/px (valid 3x, cell plane written + read 3x, labels, sizes, ids, keep bytes written + read) "
                             "+ 28 B per vertex (points, flatten, label + size by the keep pass) + 32 B per kept vertex + 12 B per kept face", "runs": []}
    elif a.normals:
        out = {"tool": "mesh_timing --normals", "reps": a.reps, "achievable_tbs": ACHIEVABLE_TBS, "peak_tbs": PEAK_TBS,
               "bytes_note": "design = valid 2x (count; the gather's rows r-1 and r+1 counted as L2 hits) + points 12 B per vertex read once "
                             "(rows r-1 / r+1 likewise) + 12 B per vertex written", "runs": []}
    else:
        out = {"tool": "mesh_timing", "reps": a.reps, "achievable_tbs": ACHIEVABLE_TBS, "peak_tbs": PEAK_TBS,
               "bytes_note": "design = valid 4x (compaction count + scatter, mesh count + emit; the second row of a block counted as an L2 hit) + "
                             "points 12 B per vertex 3x (scatter, count, emit) + 12 B per vertex and per face written; algorithmic = 13 B/px read once "
                             "+ 12 B per vertex and per face written", "runs": []}
    for name, (W, H, PW, PH, V) in CONFIGS.items():
        if (a.only and a.only != name) or (a.fill and not a.only and name == "12mp_3"):
            continue
        with scm.Scanner(W, H, PW, PH, N, N, FW, FW, max_views=V) as sc:
            sc.set_calibration(*syn.cal_tuple(syn.synth_rig(W, H, PW, PH)))
            for sel, mask in (("default", syn.default_mask(W, H)), ("lasso_19pct", lasso(W, H))):
                if a.fill:
                    mask = mask & (np.random.default_rng(11).random((H, W)) >= FILL_KNOCKED_OUT).astype(np.uint8)
                for v in range(V):
                    sc.set_mask(mask, view=v)
                    sc.synth_view(v, plane=(0.75 * (v % 16), 0.05, 0.05 - 0.003 * (v % 16)), view_id=v, noise=2)
                sc.run(0, V)
                sc.synchronize()
                xyz, valid = sc.points(0)
                r0 = H // 2 - 100
                st = {}
                np_mesh(np.ascontiguousarray(xyz[r0:r0 + 200]), np.ascontiguousarray(valid[r0:r0 + 200]), float("inf"), st)
                med = float(np.float32(np.sqrt(np.median(st["len2"]))))
                if a.fill:
                    max_edge, fill_edge = 4.0 * med, 2.0 * med
                    _, nv, nf = sc.mesh_device(max_edge, 0, V)
                    for max_hole in FILL_MAX_HOLES:
                        for min_vertices in (1, MIN_VERTICES):
                            kw = dict(max_edge=max_edge, min_vertices=min_vertices)
                            _, fv, ff, nh, nfl = sc.mesh_fill_holes_device(max_hole, fill_edge, 0, V, **kw)
                            tf, tm = clock_alternating(lambda: sc.mesh_fill_holes_device(max_hole, fill_edge, 0, V, **kw),
                                                       lambda: sc.mesh_device(max_edge, 0, V), a.reps)
                            out["runs"].append({"config": name, "size": [W, H], "views": V, "selection": sel, "max_edge_mm": round(max_edge, 6),
                                                "fill_edge_mm": round(fill_edge, 6), "max_hole": max_hole, "min_vertices": min_vertices,
                                                "mesh_vertices_per_view": round(sum(nv) / V), "mesh_faces_per_view": round(sum(nf) / V),
                                                "vertices_per_view": round(sum(fv) / V), "faces_per_view": round(sum(ff) / V),
                                                "holes_per_view": round(sum(nh) / V), "filled_per_view": round(sum(nfl) / V),
                                                "us_per_call": round(tf * 1e6, 1), "mesh_us_per_call": round(tm * 1e6, 1),
                                                "over_mesh": round(tf / tm, 3)})
                    continue
                t_compact = 0.0 if a.normals or a.components or a.smooth or a.lod else clock(lambda: sc.compact_views(0, V), a.reps)
                for label, max_edge in (("inf", float("inf")), ("median", med)):
                    if a.lod:
                        _, nv, nf = sc.mesh_device(max_edge, 0, V)
                        for step in LOD_STEPS:
                            # the coarse grid's neighbours are `step` pixels apart: the fine bar scaled by the step (doubled: the diagonals)
                            lod_edge = max_edge if label == "inf" else 2.0 * step * med
                            m, cv, cf = sc.mesh_lod_device(step, lod_edge, 0, V)
                            coarse = m.grid_width * m.grid_height * V
                            block = 13 * W * H * V + 17 * coarse
                            call = 14 * W * H * V + block + 4 * coarse + 68 * sum(cv) + 12 * sum(cf)
                            run = {"config": name, "size": [W, H], "views": V, "selection": sel, "max_edge": label, "step": step,
                                   "lod_edge_mm": None if label == "inf" else round(lod_edge, 6), "grid": [m.grid_width, m.grid_height],
                                   "fine_vertices_per_view": round(sum(nv) / V), "fine_faces_per_view": round(sum(nf) / V),
                                   "vertices_per_view": round(sum(cv) / V), "faces_per_view": round(sum(cf) / V),
                                   "block_pass_model_bytes_per_view": block // V, "call_model_bytes_per_view": call // V}
                            for tag, kw in (("plain", {}), ("mean", dict(mean=True)), ("mean_normals", dict(mean=True, normals=True)),
                                            ("filtered", dict(max_edge=max_edge, min_vertices=MIN_VERTICES))):
                                tl, tm = clock_alternating(lambda: sc.mesh_lod_device(step, lod_edge, 0, V, **kw), lambda: sc.mesh_device(max_edge, 0, V), a.reps)
                                run.update({f"{tag}_us_per_call": round(tl * 1e6, 1), f"{tag}_mesh_us_per_call": round(tm * 1e6, 1),
                                            f"{tag}_over_mesh": round(tl / tm, 3)})
                            run["plain_call_model_tbs"] = round(call / (run["plain_us_per_call"] * 1e-6) / 1e12, 3)
                            out["runs"].append(run)
                        continue
                    if a.smooth:
                        it, lam, mu = SMOOTH
                        _, nv, nf = sc.mesh_device(max_edge, 0, V)
                        assert sc.mesh_smoothed_device(max_edge, 0, V, it, lam, mu)[1] == nv
                        run = {"config": name, "size": [W, H], "views": V, "selection": sel, "max_edge": label,
                               "max_edge_mm": None if label == "inf" else round(med, 6), "vertices_per_view": round(sum(nv) / V),
                               "faces_per_view": round(sum(nf) / V)}
                        step_bytes = 2 * W * H * V + 24 * sum(nv)
                        for tag, flag in (("plain", False), ("fixed_normals", True)):
                            ts, tm = clock_alternating(lambda: sc.mesh_smoothed_device(max_edge, 0, V, it, lam, mu, flag, flag),
                                                       lambda: sc.mesh_device(max_edge, 0, V), a.reps)
                            t1, _ = clock_alternating(lambda: sc.mesh_smoothed_device(max_edge, 0, V, 1, lam, mu, flag, flag),
                                                      lambda: sc.mesh_device(max_edge, 0, V), a.reps)
                            step = (ts - t1) / (2 * (it - 1))
                            run.update({f"{tag}_us_per_call": round(ts * 1e6, 1), f"{tag}_us_per_view": round(ts * 1e6 / V, 2),
                                        f"{tag}_one_iteration_us_per_call": round(t1 * 1e6, 1), f"{tag}_mesh_us_per_call": round(tm * 1e6, 1),
                                        f"{tag}_over_mesh": round(ts / tm, 2), f"{tag}_step_us_per_view": round(step * 1e6 / V, 2),
                                        f"{tag}_step_design_tbs": round(step_bytes / step / 1e12, 3)})
                        run["step_design_bytes_per_view"] = step_bytes // V
                        out["runs"].append(run)
                        continue
                    if a.components:
                        _, nv, nf = sc.mesh_device(max_edge, 0, V)
                        _, _, cv, nc = sc.mesh_components_device(max_edge, 0, V)
                        _, kv, kf = sc.mesh_filtered_device(max_edge, MIN_VERTICES, 0, V)
                        assert cv == nv
                        tc, tm = clock_alternating(lambda: sc.mesh_components_device(max_edge, 0, V), lambda: sc.mesh_device(max_edge, 0, V), a.reps)
                        tf, tm2 = clock_alternating(lambda: sc.mesh_filtered_device(max_edge, MIN_VERTICES, 0, V), lambda: sc.mesh_device(max_edge, 0, V), a.reps)
                        d_comp = 17 * W * H * V + 32 * sum(nv)
                        d_filt = 21 * W * H * V + 28 * sum(nv) + 32 * sum(kv) + 12 * sum(kf)
                        out["runs"].append({
                            "config": name, "size": [W, H], "views": V, "selection": sel, "max_edge": label, "max_edge_mm": None if label == "inf" else round(med, 6),
                            "vertices_per_view": round(sum(nv) / V), "faces_per_view": round(sum(nf) / V), "components_per_view": round(sum(nc) / V),
                            "kept_vertices_per_view": round(sum(kv) / V), "kept_faces_per_view": round(sum(kf) / V),
                            "components_us_per_call": round(tc * 1e6, 1), "components_us_per_view": round(tc * 1e6 / V, 2),
                            "filtered_us_per_call": round(tf * 1e6, 1), "filtered_us_per_view": round(tf * 1e6 / V, 2),
                            "mesh_us_per_call": round(tm * 1e6, 1), "mesh_us_per_call_beside_filtered": round(tm2 * 1e6, 1),
                            "components_over_mesh": round(tc / tm, 2), "filtered_over_mesh": round(tf / tm2, 2),
                            "components_design_bytes_per_view": d_comp // V, "components_design_tbs": round(d_comp / tc / 1e12, 3),
                            "filtered_design_bytes_per_view": d_filt // V, "filtered_design_tbs": round(d_filt / tf / 1e12, 3)})
                        continue
                    if a.normals:
                        _, nv, nf = sc.mesh_device(max_edge, 0, V)
                        assert sc.mesh_normals_device(max_edge, 0, V)[2] == nv
                        tn, tm = clock_alternating(lambda: sc.mesh_normals_device(max_edge, 0, V), lambda: sc.mesh_device(max_edge, 0, V), a.reps)
                        design = 2 * W * H * V + 24 * sum(nv)
                        out["runs"].append({
                            "config": name, "size": [W, H], "views": V, "selection": sel, "max_edge": label, "max_edge_mm": None if label == "inf" else round(med, 6),
                            "vertices_per_view": round(sum(nv) / V), "faces_per_view": round(sum(nf) / V),
                            "normals_us_per_call": round(tn * 1e6, 1), "normals_us_per_view": round(tn * 1e6 / V, 2),
                            "mesh_us_per_call": round(tm * 1e6, 1), "normals_over_mesh": round(tn / tm, 2),
                            "design_bytes_per_view": design // V, "design_tbs": round(design / tn / 1e12, 3),
                            "design_over_achievable": round(design / tn / 1e12 / ACHIEVABLE_TBS, 3)})
                        continue
                    _, nv, nf = sc.mesh_device(max_edge, 0, V)
                    t = clock(lambda: sc.mesh_device(max_edge, 0, V), a.reps)
                    design = 4 * W * H * V + 48 * sum(nv) + 12 * sum(nf)
                    algorithmic = 13 * W * H * V + 12 * sum(nv) + 12 * sum(nf)
                    out["runs"].append({
                        "config": name, "size": [W, H], "views": V, "selection": sel, "max_edge": label, "max_edge_mm": None if label == "inf" else round(med, 6),
                        "vertices_per_view": round(sum(nv) / V), "faces_per_view": round(sum(nf) / V),
                        "mesh_us_per_call": round(t * 1e6, 1), "mesh_us_per_view": round(t * 1e6 / V, 2),
                        "compact_views_us_per_call": round(t_compact * 1e6, 1), "mesh_over_compact": round(t / t_compact, 2),
                        "design_bytes_per_view": design // V, "algorithmic_bytes_per_view": algorithmic // V,
                        "design_tbs": round(design / t / 1e12, 3), "design_over_achievable": round(design / t / 1e12 / ACHIEVABLE_TBS, 3),
                        "design_over_peak": round(design / t / 1e12 / PEAK_TBS, 3)})
    if a.components or a.smooth or a.lod or a.fill:
        with open(a.out, "w") as f:
            f.write(json.dumps(out) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
