"""The exposure fusion (sl3d_fuse_exposures, one launch of k_fuse_exposures) at 1920x1080 with 10 Gray planes per axis, both axes
coded (46 planes in use per view), over E = 2, 3 and 4 exposures, timed with the context's HIP events (sl3d_timer_start / sl3d_timer_stop
around the asynchronous call, counts == NULL).  Beside it two yardsticks:
  copy_view     sl3d_copy_view of one view on the same context, timed the same way (frame stack + mask + band: a little more than 2 x 46 planes)
  bytes_model   (E + 1) * 46 * pixels bytes at 8 TB/s: every plane in use read once and written once, nothing else
and the ratio of the launch to both.  No threshold is set on the time.
The capture: synthetic 1080p views generated on the device (fringe width 2, camera noise +-2), exposure e at gain 0.8 * 4^(e - 1) for e >= 1
and 0.2 for e = 0 -- the second exposure is the well exposed one, the later ones clip --, so nearly every lane's pixels choose one exposure
(the common case of pass 2); the share of each exposure in the map is recorded.  Before anything is timed the counts are checked against
the map (bincount of map & 7, bytes with bit 7) and their sum against the pixel count; a difference ends the tool with an error.
Not measured: other sizes and Gray depths, one-axis and direct-Gray contexts (fewer planes in use), scenes whose choice changes from
pixel to pixel (pass 2 then loads from several exposures), hardware counters.
Written to --out (default profiles/exposure_fusion_timing.json) and printed.  usage: exposure_fusion_timing.py [--reps N] [--out PATH]"""
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
EXPOSURES = (2, 3, 4)
GAINS = (0.2, 0.8, 3.2, 12.8)
WARMUP = 10
HBM_BYTES_PER_S = 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "exposure_fusion_timing.json"))
    a = ap.parse_args()
    syn = importlib.import_module("3dscan_amd.synth")
    scm = importlib.import_module("3dscan_amd.scanner")
    planes = 2 * (F + 2 * N)
    out = {"tool": "exposure_fusion_timing", "size": [W, H], "n_gray": N, "n_fringe": F, "planes_in_use": planes, "gains": list(GAINS), "saturation": 255,
           "reps": a.reps, "warmup": WARMUP, "timer": "HIP events around the asynchronous call, median over the repetitions",
           "not_measured": ["other sizes and Gray depths", "one-axis and direct-Gray contexts", "scenes whose choice changes from pixel to pixel",
                            "hardware counters"],
           "runs": []}

    def timed(sc, call):
        t = []
        for rep in range(a.reps + WARMUP):
            sc.timer_start()
            call()
            ms = sc.timer_stop()
            if rep >= WARMUP:
                t.append(ms * 1e3)
        return round(float(np.median(t)), 2), [round(float(np.percentile(t, q)), 2) for q in (10, 90)]

    dst = len(GAINS)
    with scm.Scanner(W, H, W, H, N, N, FW, FW, n_fringe=F, max_views=dst + 1) as sc:
        sc.set_calibration(*syn.cal_tuple(syn.synth_rig(W, H, W, H)))
        for e, g in enumerate(GAINS):
            sc.synth_view(e, noise=2, gain=g, view_id=0)
        sc.set_masks(syn.default_mask(W, H))
        copy_us, copy_p = timed(sc, lambda: sc.copy_view(0, dst))
        out["copy_view_us"], out["copy_view_us_p10_p90"] = copy_us, copy_p
        for E in EXPOSURES:
            counts = sc.fuse_exposures(0, E, dst)
            m = sc.exposure_map(dst)
            if int(counts[:E].sum()) != W * H or not np.array_equal(counts[:E], np.bincount((m & 7).ravel(), minlength=E)) or \
                    int(counts[E]) != int((m & 0x80).astype(bool).sum()):
                sys.exit(f"E = {E}: the counts {counts.tolist()} and the map disagree")
            us, p = timed(sc, lambda: sc.fuse_exposures(0, E, dst, counts=False))
            model = (E + 1) * planes * W * H / HBM_BYTES_PER_S * 1e6
            out["runs"].append({"exposures": E, "fuse_us": us, "fuse_us_p10_p90": p, "bytes_model_us": round(model, 2),
                                "fuse_over_bytes_model": round(us / model, 3), "fuse_over_copy_view": round(us / copy_us, 3),
                                "share_of_each_exposure": [round(float(c) / (W * H), 4) for c in counts[:E]],
                                "share_clipped_in_every_exposure": round(float(counts[E]) / (W * H), 4)})
    with open(a.out, "w") as f:
        f.write(json.dumps(out) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
