"""The scan of a SL3D_FLAG_DIRECT_GRAY context (the Gray frames against the fringe mean, no inverse Gray frame read) at 1920x1080 with
10 Gray planes per axis, over 1 and over 16 views, against the same scan without the flag, the two alternating in one process, each timed
with its context's HIP events (sl3d_timer_start / sl3d_timer_stop around the asynchronous call).  Two pairs:
  one_axis  (a) SL3D_FLAG_SUBPIXEL | SL3D_FLAG_ANCHOR_PERIODS | SL3D_FLAG_ONLY_VERTICAL | SL3D_FLAG_DIRECT_GRAY: one launch of k_direct_gray<0, true>
            (b) the same without SL3D_FLAG_DIRECT_GRAY: one launch of k_one_axis<0, true>
  two_axes  (a) SL3D_FLAG_SUBPIXEL | SL3D_FLAG_ANCHOR_PERIODS | SL3D_FLAG_DIRECT_GRAY: one launch of k_direct_gray<2, true>
            (b) the same without SL3D_FLAG_DIRECT_GRAY: one launch of k_subpixel_fused<true>
(b) is code the flag does not touch.  Before anything is timed the points and valid planes (two axes: and the residual plane) of (a) over
all 16 views are compared bit for bit with the staged route -- sl3d_run on a SL3D_FLAG_KEEP_STAGES context with the same flags --; a
difference ends the tool with an error.  How far (a) and (b) agree is recorded too: they decode the lit pixels alike, the unlit ones under
noise both to noise.  Every shape is warmed up; the medians over the repetitions are reported with p10 / p90, the ratio (a) / (b) of the
medians and p10 / p90 of the ratios of the alternating pairs.  Required: (a) at or below (b) at both view counts of both pairs -- (a) reads
strictly fewer bytes with the same arithmetic; the estimates from the bytes alone are 28 / 38 = 0.74 (one axis) and 45 / 65 = 0.69 (two
axes).  The tool ends with an error if (a) is above (b) anywhere.
The capture: synthetic 1080p views (fringe width 2, 10 Gray planes per axis, camera noise +-2, synth_rig: an undistorted projector with a
horizontal baseline), the plane tilted differently per view, generated on the device with the same arguments on every context.
Not measured: other sizes and Gray depths, the horizontal form, the unanchored forms, hardware counters, the host pipeline's rate (where
the upload of 10 or 20 planes fewer per view counts most).
Written to --out (default profiles/direct_gray_timing.json) and printed.  usage: direct_gray_timing.py [--reps N] [--out PATH]"""
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

W, H, N, FW, F = 1920, 1080, 10, 2, 3
VIEWS = (1, 16)
WARMUP = 10
PAIRS = (("one_axis", 0, 28 / 38), ("two_axes", None, 45 / 65))


def _bits(a):
    return a.view(np.uint32 if a.dtype == np.float32 else a.dtype)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "direct_gray_timing.json"))
    a = ap.parse_args()
    syn = importlib.import_module("3dscan_amd.synth")
    scm = importlib.import_module("3dscan_amd.scanner")
    V = max(VIEWS)
    out = {"tool": "direct_gray_timing", "size": [W, H], "n_gray": N, "fringe_width": FW, "n_fringe": F, "noise": 2, "reps": a.reps, "warmup": WARMUP,
           "timer": "HIP events around the asynchronous call, median over the repetitions, the two routes alternating",
           "not_measured": ["other sizes and Gray depths", "the horizontal form", "the unanchored forms", "hardware counters", "the host pipeline's rate"],
           "pairs": {}}

    def prepare(sc):
        sc.set_calibration(*syn.cal_tuple(syn.synth_rig(W, H, W, H)))
        for v in range(V):
            sc.synth_view(v, plane=(0.0, 0.05 - 0.005 * v, 0.05 + 0.003 * v), noise=2)
            sc.set_mask(syn.default_mask(W, H), view=v)

    def planes(sc, v, residual):
        xyz, valid = sc.points(v)
        return [valid, xyz] + ([sc.residuals(v)] if residual else [])

    ok = True
    for pair, axis, estimate in PAIRS:
        common = dict(max_views=V, subpixel=True, anchored=True, only_axis=axis)
        rec = {"estimate_from_bytes_direct_over_inverse": round(estimate, 3), "runs": []}
        with scm.Scanner(W, H, W, H, N, N, FW, FW, direct_gray=True, **common) as direct, scm.Scanner(W, H, W, H, N, N, FW, FW, **common) as inverse:
            for sc in (direct, inverse):
                prepare(sc)
            rec["kernels"] = {"direct": direct.fused_kernel_name(1), "inverse": inverse.fused_kernel_name(1)}
            # the planes of (a) against the staged route, bit for bit, before anything is timed
            direct.run(0, V)
            inverse.run(0, V)
            n_direct = n_inverse = n_both = 0
            with scm.Scanner(W, H, W, H, N, N, FW, FW, keep_stages=True, direct_gray=True, **common) as keep:
                prepare(keep)
                keep.run(0, V)
                for v in range(V):
                    got, want = planes(direct, v, axis is None), planes(keep, v, axis is None)
                    if not all(np.array_equal(_bits(g), _bits(w)) for g, w in zip(got, want)):
                        sys.exit(f"{pair}, view {v}: the direct launch and the staged route differ ({[int((_bits(g) != _bits(w)).sum()) for g, w in zip(got, want)]} elements)")
                    vb = inverse.points(v)[1]
                    n_direct += int((got[0] == 1).sum())
                    n_inverse += int((vb == 1).sum())
                    n_both += int(((vb == 1) & (got[0] == 1)).sum())
            rec["planes_equal_bit_for_bit_with_the_staged_route"] = True
            rec["valid_pixels"] = {"direct": n_direct, "inverse": n_inverse, "both": n_both}
            for n_views in VIEWS:
                t = {"direct": [], "inverse": []}
                for rep in range(a.reps + WARMUP):
                    direct.timer_start()
                    direct.run(0, n_views)
                    ta = direct.timer_stop()
                    inverse.timer_start()
                    inverse.run(0, n_views)
                    tb = inverse.timer_stop()
                    if rep >= WARMUP:
                        t["direct"].append(ta)
                        t["inverse"].append(tb)
                med = {k: float(np.median(v)) * 1e3 for k, v in t.items()}
                run = {"views": n_views}
                for k, v in t.items():
                    run[k + "_us"] = round(med[k], 2)
                    run[k + "_us_p10_p90"] = [round(float(np.percentile(v, q)) * 1e3, 2) for q in (10, 90)]
                ratios = np.asarray(t["direct"]) / np.asarray(t["inverse"])
                run.update({"direct_over_inverse": round(med["direct"] / med["inverse"], 3),
                            "direct_over_inverse_p10_p90": [round(float(np.percentile(ratios, q)), 3) for q in (10, 90)],
                            "direct_is_not_slower": med["direct"] <= med["inverse"]})
                ok = ok and run["direct_is_not_slower"]
                rec["runs"].append(run)
        out["pairs"][pair] = rec
    with open(a.out, "w") as f:
        f.write(json.dumps(out) + "\n")
    print(json.dumps(out))
    if not ok:
        sys.exit("a direct launch is slower than the launch that reads the inverse frames")


if __name__ == "__main__":
    main()
