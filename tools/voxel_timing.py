"""The voxel grid (sl3d_voxel_grid -- two memsets, k_voxel_insert, k_voxel_count, k_compact_scan, k_voxel_scatter) over the
registered cloud of 1 and of 16 synthetic 1920x1080 views (a turntable: 22.5 degrees a view about the vertical through the centroid of view
0), leaf at 2 and at 8 median distances between row neighbours, both modes, min_points 1, with the run collapse and without it.

The form without the collapse is no runtime path of the library: the tool builds two measurement libraries of its own into
build/voxel_timing/ -- sl3d_voxel.hip compiled with -DSL3D_VOXEL_TIMING (an event between the launches and sl3d_voxel_launch_times to
read them) and, for the second, -DSL3D_VOXEL_NO_COLLAPSE, linked with the objects of 3dscan_amd/csrc as make left them -- and runs one
child process per library (SL3D_LIB).  A library that is already there and newer than its sources is kept.

Per case: the whole call between the context's HIP events (sl3d_timer_start / sl3d_timer_stop around the asynchronous call, counts ==
NULL, xyz_in == NULL), and the five parts of the same calls by the events inside; the median of --reps calls after 5.  Beside it, on the
same context over the same views and timed by the same events: sl3d_register_views (with its compaction and its read-back of the counts)
and sl3d_compact_views.  On one view the result is held against the NumPy restatement (tests/voxel_reference.py) before anything is timed,
and the share of points that are heads of a run of equal keys inside a wave -- what is left of the atomics -- is recorded.
There is no bar to meet.  Not measured: hardware counters (atomic requests, L2 hit rates), other sizes and leaves, clouds without
organised order, min_points > 1, the host-cloud route.
Written to --out (default profiles/voxel_timing.json) and printed.  usage: voxel_timing.py [--reps N] [--out PATH]"""
import argparse
import ctypes as C
import importlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
CSRC = os.path.join(ROOT, "3dscan_amd", "csrc")
BUILD = os.path.join(ROOT, "build", "voxel_timing")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-Wno-unused-function"]   # the Makefile's
VARIANTS = {"collapse": [], "no_collapse": ["-DSL3D_VOXEL_NO_COLLAPSE"]}
PARTS = ("memsets_us", "insert_us", "count_us", "scan_us", "scatter_us")
W, H, N, FW = 1920, 1080, 10, 2
VIEWS = (1, 16)
LEAVES = (2, 8)
WARMUP = 5


def build(variant):
    """the measurement library of a variant; built here unless it is there and newer than the kernels' sources"""
    lib = os.path.join(BUILD, f"libsl3d_{variant}.so")
    srcs = [os.path.join(CSRC, f) for f in ("sl3d_voxel.hip", "sl3d_voxel.h", "sl3d_block.h", "sl3d_internal.h")]
    if os.path.exists(lib) and all(os.path.getmtime(lib) >= os.path.getmtime(s) for s in srcs):
        return lib
    objs = sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".o") and f != "sl3d_voxel.o")
    if len(objs) < 10:
        sys.exit("voxel_timing: build the library first (make -C 3dscan_amd/csrc): its objects are linked into the measurement libraries")
    os.makedirs(BUILD, exist_ok=True)
    obj = os.path.join(BUILD, f"sl3d_voxel_{variant}.o")
    subprocess.check_call(["hipcc", *FLAGS, "-DSL3D_VOXEL_TIMING", *VARIANTS[variant], "-c", os.path.join(CSRC, "sl3d_voxel.hip"), "-o", obj])
    subprocess.check_call(["hipcc", *FLAGS, "-shared", "-o", lib, *objs, obj, "-ldl"])
    return lib


def leg(reps):
    """one library (SL3D_LIB), every case; prints the runs as one JSON line"""
    import numpy as np
    try:
        import torch  # noqa: F401  (its ROCm stack first, as tests/conftest.py)
    except Exception:
        pass
    import voxel_reference as VR
    syn = importlib.import_module("3dscan_amd.synth")
    scm = importlib.import_module("3dscan_amd.scanner")
    runs = []

    def timed(sc, call, after=None):
        t, extra = [], []
        for rep in range(reps + WARMUP):
            sc.timer_start()
            call()
            ms = sc.timer_stop()
            if rep >= WARMUP:
                t.append(ms * 1e3)
                if after:
                    extra.append(after())
        return round(float(np.median(t)), 2), [round(float(np.percentile(t, q)), 2) for q in (10, 90)], extra

    with scm.Scanner(W, H, W, H, N, N, FW, FW, max_views=max(VIEWS)) as sc:
        L = sc.L
        L.sl3d_voxel_launch_times.argtypes, L.sl3d_voxel_launch_times.restype = [C.POINTER(C.c_float)], C.c_int
        sc.set_calibration(*syn.cal_tuple(syn.synth_rig(W, H, W, H)))
        for v in range(max(VIEWS)):
            sc.synth_view(v, noise=1, view_id=v)
        sc.set_masks(syn.default_mask(W, H))
        sc.run(0, max(VIEWS))
        xyz, valid = sc.points(0)
        both = (valid[:, 1:] == 1) & (valid[:, :-1] == 1)
        spacing = float(np.median(np.linalg.norm(xyz[:, 1:].astype(np.float64) - xyz[:, :-1], axis=-1)[both]))
        axis = [float(v) for v in xyz[valid == 1].astype(np.float64).mean(axis=0)]
        total = C.c_int64(0)

        def parts():
            ms = (C.c_float * 5)()
            if L.sl3d_voxel_launch_times(ms) != 0:
                sys.exit("voxel_timing: sl3d_voxel_launch_times failed")
            return [v * 1e3 for v in ms]

        for n in VIEWS:
            def register():
                sc._chk(L.sl3d_register_views(sc._h, 0, n, *axis, 22.5, None, 0, C.byref(total)), "sl3d_register_views")
            reg_us, reg_p, _ = timed(sc, register)
            cmp_us, cmp_p, _ = timed(sc, lambda: sc.compact_views(0, n))
            register()
            for k in LEAVES:
                leaf = float(np.float32(k * spacing))
                for centroid in (True, False):
                    heads = None
                    if n == 1:   # the result against the restatement, and what the collapse leaves of the atomics
                        reg = sc.register_views(0, n, *axis, 22.5)
                        got, ref = sc.voxel_grid(leaf, 1, centroid, stats=True), VR.grid(reg, leaf, 1, centroid)
                        if got[3] != ref[3] or any(not np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(got[:3], ref[:3])):
                            sys.exit(f"voxel_timing: leaf {leaf}, centroid {centroid}: the grid differs from the restatement")
                        key = VR.key(VR.cell(reg, leaf)[0])
                        head = np.concatenate([[True], key[1:] != key[:-1]])
                        head[::64] = True
                        heads = round(float(head.mean()), 4)
                    _, stats = sc.voxel_grid_device(leaf, 1, centroid)
                    flags = scm.VOXEL_CENTROID if centroid else scm.VOXEL_FIRST
                    us, p, extra = timed(sc, lambda: sc._chk(L.sl3d_voxel_grid(sc._h, None, 0, leaf, 1, flags, None, None), "sl3d_voxel_grid"), after=parts)
                    med = np.median(np.array(extra), axis=0)
                    runs.append({"views": n, "leaf_spacings": k, "leaf": round(leaf, 5), "mode": "centroid" if centroid else "first",
                                 "points": stats[0], "dropped": stats[1], "cells": stats[2], "points_per_cell": round(stats[0] / max(stats[2], 1), 2),
                                 "run_heads_share": heads, "grid_us": us, "grid_us_p10_p90": p,
                                 **{name: round(float(v), 2) for name, v in zip(PARTS, med)},
                                 "register_views_us": reg_us, "register_views_us_p10_p90": reg_p, "compact_views_us": cmp_us,
                                 "compact_views_us_p10_p90": cmp_p, "grid_over_register_views": round(us / reg_us, 3),
                                 "grid_over_compact_views": round(us / cmp_us, 3), "ns_per_point": round(us * 1e3 / max(stats[0], 1), 4)})
        print(json.dumps({"pixel_spacing_mm": round(spacing, 5), "axis": [round(v, 3) for v in axis], "runs": runs}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "voxel_timing.json"))
    ap.add_argument("--leg", action="store_true", help="(internal) run the cases on the library SL3D_LIB names")
    a = ap.parse_args()
    if a.leg:
        return leg(a.reps)
    out = {"tool": "voxel_timing", "size": [W, H], "n_gray": N, "reps": a.reps, "warmup": WARMUP, "rot_step_deg": 22.5, "min_points": 1,
           "timer": "HIP events around the asynchronous call (counts == NULL) and between its launches (measurement builds), medians over the "
                    "repetitions; register_views_us includes its compaction and its read-back of the counts",
           "not_measured": ["hardware counters", "other sizes and leaves", "clouds without organised order", "min_points > 1", "the host-cloud route"],
           "variants": {}}
    for variant in VARIANTS:
        lib = build(variant)
        res = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", "--reps", str(a.reps)], env=dict(os.environ, SL3D_LIB=lib),
                             stdout=subprocess.PIPE, text=True)
        if res.returncode != 0:
            sys.exit(f"voxel_timing: the {variant} leg failed ({res.returncode})")
        out["variants"][variant] = json.loads(res.stdout.strip().splitlines()[-1])
    on, off = (out["variants"][v]["runs"] for v in VARIANTS)
    out["collapse_speedup"] = [{"views": a_["views"], "leaf_spacings": a_["leaf_spacings"], "mode": a_["mode"],
                                "insert": round(b_["insert_us"] / a_["insert_us"], 3), "grid": round(b_["grid_us"] / a_["grid_us"], 3)}
                               for a_, b_ in zip(on, off)]
    with open(a.out, "w") as f:
        f.write(json.dumps(out) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
