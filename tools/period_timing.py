"""sl3d_repair_periods at 1920x1080: one call per axis, radius 4 and 8, timed with the context's HIP events
(sl3d_timer_start / sl3d_timer_stop around the one asynchronous call), and sl3d_unwrap_phase of the same axis of the same view of the same
context timed the same way in the same repetition -- the yardstick: one pointwise launch over the same planes.  A repetition runs stage 3,
stage 4 (timed) and the repair (timed) of an axis, so the two alternate and every repair starts from the planes stage 4 left; the medians
over the repetitions and their ratio are reported.
The capture: a synthetic 1080p view (fringe width 16, 7 Gray planes per axis, camera noise +-2) whose Gray / inverse frames are then
shifted by one pixel along the coded direction of each axis, so that about one pixel in sixteen carries the wrong period -- the band a
real rig shows.  --shift 0 times the call on the unshifted capture (nothing to repair: the apply launch reads the jump plane only).
Bytes the design moves per call: jumps 5 B/px read (absolute phase, valid byte) + 1 B/px written (+ 4 B per pixel with j != 0: its code);
apply 1 B/px read + 16 B per repaired pixel (code and wrapped phase read, code and absolute phase written).
Written to --out (default profiles/period_repair_timing.json) and printed.  usage: period_timing.py [--reps N] [--shift S] [--out PATH]"""
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

W, H, N, FW = 1920, 1080, 7, 16
RADII = (4, 8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--shift", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "period_repair_timing.json"))
    a = ap.parse_args()
    syn = importlib.import_module("3dscan_amd.synth")
    scm = importlib.import_module("3dscan_amd.scanner")
    out = {"tool": "period_timing", "size": [W, H], "n_gray": N, "fringe_width": FW, "gray_shift_px": a.shift, "reps": a.reps,
           "timer": "HIP events around one asynchronous call, median over the repetitions", "runs": []}
    with scm.Scanner(W, H, W, H, N, N, FW, FW, keep_stages=True) as sc:
        sc.set_calibration(*syn.cal_tuple(syn.synth_rig(W, H, W, H)))
        sc.set_mask(syn.default_mask(W, H))
        sc.synth_view(0, noise=2)
        for axis in (0, 1):
            if a.shift:
                planes = sc.frames(axis)
                sc.set_frames_range(axis, 3, [np.roll(p, -a.shift, axis=1 - axis) for p in planes[3:]])
        for axis in (0, 1):
            for radius in RADII:
                t_unwrap, t_repair = [], []
                counts = None
                for rep in range(a.reps + 10):
                    sc.compute_wrapped_phase(axis)
                    sc.timer_start()
                    sc.unwrap_phase(axis)
                    tu = sc.timer_stop()
                    if rep == 0:
                        counts = sc.repair_periods(axis, radius)          # (the counts, once; synchronises)
                        continue
                    sc.timer_start()
                    sc.repair_periods(axis, radius, want_counts=False)
                    tr = sc.timer_stop()
                    if rep >= 10:                                          # (the first repetitions warm up both)
                        t_unwrap.append(tu)
                        t_repair.append(tr)
                mu, mr = float(np.median(t_unwrap)) * 1e3, float(np.median(t_repair)) * 1e3
                px = W * H
                model = 7 * px + 20 * counts[0] + 4 * counts[1]
                out["runs"].append({"axis": axis, "radius": radius, "repaired": counts[0], "unrepairable": counts[1],
                                    "repair_us": round(mr, 2), "repair_us_p10_p90": [round(float(np.percentile(t_repair, q)) * 1e3, 2) for q in (10, 90)],
                                    "unwrap_us": round(mu, 2), "unwrap_us_p10_p90": [round(float(np.percentile(t_unwrap, q)) * 1e3, 2) for q in (10, 90)],
                                    "repair_over_unwrap": round(mr / mu, 3), "model_bytes": model, "model_tbs": round(model / (mr * 1e-6) / 1e12, 3)})
    with open(a.out, "w") as f:
        f.write(json.dumps(out) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
