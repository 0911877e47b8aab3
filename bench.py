#!/usr/bin/env python3
"""Benchmark of the fused decode -> unwrap -> correspond -> triangulate kernel (BASELINE.json metric).

    python bench.py --gpus N --steps K --warmup W [--full]

A plain run does what the headline needs and nothing else: set-up, warm-up, the K timed steps, --dump-outputs if given, and the
line.  --full adds everything else the benchmark measures or checks, after the headline: the compacted clouds leg, the side
figures (other rigs, sizes and launch patterns, one scan from idle, a device copy), the CPU baseline that also checks one view of
the GPU result, the host buffer paths, and for N > 1 the assembly variants that are never the headline.

N > 1: one process per GPU over torch.distributed (backend nccl = RCCL).  Started by torch.distributed.run (the driver's
way: RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* in the environment) each process is a rank; started plainly, `python
bench.py --gpus N` spawns its N ranks itself as fresh child processes -- before this process has touched the GPU, and
never by exec -- and prints rank 0's JSON line.

Workload (configs[1] of BASELINE.json): 1920x1080 camera, 3 phase-shift + 10 Gray-code bit planes per axis,
reference-faithful two-axis mode (every Gray frame is thresholded against its inverse frame, so a view is
2*(3+10+10) = 46 frames), synthetic captures resident in HBM.  A step is ONE launch of the fused kernel over a batch of
`--views` views per GPU (default 16, i.e. 2 GB of frames + results: larger than the 256 MiB Infinity Cache, so the kernel
really streams from HBM).  With N GPUs every view is sharded by image rows (1080/N rows per GPU) and the batch grows to
N*views views, so per-GPU work is fixed (weak scaling); the per-pixel map needs no collective (the mask halo comes from
the input mask).  `value` is that compute-only rate.  The assembly of the clouds on rank 0 -- the north star's "single RCCL
gather" -- is measured too and reported as `with_assembly`: end to end, pipelined per chunk of views on a communication
stream beside the compute stream, dense (xyz + valid) and, with --full or --check, compacted (valid points only, compacted
by the fused kernel).

The defaults (300 warm-up + 2000 timed launches, ~1 s of GPU time) let the clocks settle: the kernel runs the package
into its power limit (~1.4 kW), and a 25 ms run from idle measures the ramp, not the steady state.  For the same reason
the set-up ends with --precondition-ms (0.4 s) of launches before the W warm-up steps, whatever W and K are.

Prints ONE JSON line (rank 0).
"""
import argparse
import hashlib
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E peak, /opt/skills/guides/MI355X_MICROARCH.md
DUMP_MAX_PIXELS = 1 << 21   # --dump-outputs: 24 B per pixel (f64 index + 3 x f32 xyz + f32 valid) -> at most 50.3 MB


def measured_traffic(px_per_launch, kernel="dense"):
    """HBM bytes per launch of the fused kernel (kernel = "dense") or of its compacting instantiation ("clouds") from the latest
    COMMITTED PMC run (tools/profile.sh + tools/summarize_profile.py: FETCH_SIZE and WRITE_SIZE in separate rocprofv3 passes,
    scaled by the factors calibrated on tools/membench in the same session), scaled to the pixels of this launch.  Not
    measured in this run: the source file is named beside the number.  (None, None) if no profile has been committed."""
    import glob
    pat = "r[0-9]*_traffic.json" if kernel == "dense" else "r[0-9]*_traffic_clouds.json"
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", pat)))
    if not files:
        return None, None
    t = json.load(open(files[-1]))
    scale = px_per_launch / float(t.get("pixels_per_launch") or (t["algorithmic_bytes_per_launch"] / 60.0))
    return round(t["hbm_bytes_per_launch"] * scale), os.path.relpath(files[-1], ROOT)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=300)
    ap.add_argument("--scaling", choices=("weak", "strong"), default="weak",
                    help="N > 1: weak (default) = --views views per GPU per step, the batch grows with N; strong = BASELINE configs[3] as it is "
                         "stated: --total-views views (64) row-sharded over the N GPUs, the same total work for every N")
    ap.add_argument("--total-views", type=int, default=64, help="--scaling strong: views per step over all GPUs (configs[3]: 64)")
    ap.add_argument("--views", type=int, default=16, help="views per GPU per step")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--ngray", type=int, default=10)
    ap.add_argument("--fringe-width", type=int, default=2)
    ap.add_argument("--noise", type=int, default=2)
    ap.add_argument("--precondition-ms", type=float, default=400.0,
                    help="part of the SETUP, before the W warm-up steps: run the kernel for this long so that the clocks have "
                         "left the idle state whatever W is (the package is power-managed; see profiles/README.md). 0 disables")
    ap.add_argument("--rig", default="reference", choices=["reference", "distorted", "radial", "general"],
                    help="reference = the reference's calibration rescaled (BASELINE workload); distorted = the same rig with "
                         "projector distortion and camera tangential terms (table path); general = skewed camera matrix as well "
                         "(everything evaluated in the kernel) -- the other two are sweeps / side figures only")
    ap.add_argument("--full", action="store_true",
                    help="after the headline, also measure and check everything else: the compacted clouds leg, the side figures (other "
                         "rigs, sizes and launch patterns, device copy rate), the CPU baseline with its check of the GPU result, the host "
                         "buffer paths and (N>1) the assembly variants that are never the headline. Off by default: a plain run sets up, "
                         "warms up, times the steps and prints the line")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline and the host buffer figures")
    ap.add_argument("--no-clouds", action="store_true", help="with --full: skip the frames -> compacted clouds leg (A/B builds of the dense kernel only)")
    ap.add_argument("--no-side", action="store_true", help="with --full: skip the side figures (1 view latency, other rigs, N=9)")
    ap.add_argument("--no-assemble", action="store_true", help="skip the assembly measurements (N>1)")
    ap.add_argument("--shim-timing", action="store_true",
                    help="with --full: also time the Level-1 drop-in path (tools/shim_bench.cpp: compiles with g++, writes BMP files, minutes "
                         "of wall time); off by default so that the driver's line depends on the GPU only")
    ap.add_argument("--one-view-cold-only", action="store_true",
                    help="run only side.one_view_cold (one view per launch, a different resident view each launch: frames from HBM, not from "
                         "the Infinity Cache) and print it -- the command tools/profile.sh puts under rocprofv3 for that figure")
    ap.add_argument("--idle-samples", type=int, default=20, help="samples per variant of side.one_scan_from_idle (0 = skip it; each sample sleeps --idle-sleep s)")
    ap.add_argument("--idle-sleep", type=float, default=1.0, help="idle time in front of every sample of side.one_scan_from_idle, seconds")
    ap.add_argument("--idle-only", action="store_true", help="run only side.one_scan_from_idle and print it")
    ap.add_argument("--families-only", action="store_true",
                    help="run only the 16-view launches of the other kernel families (rig classes 2 / 3 / 0, 9 and 14 Gray planes) and print them: "
                         "the command behind profiles/rNN_families_kernel_stats.csv")
    ap.add_argument("--cold-views", type=int, default=8, help="resident views the one-view-cold figure rotates over (8 x 97.5 MB of frames > 256 MiB)")
    ap.add_argument("--backend", default="nccl", help="torch.distributed backend for N>1 (nccl = RCCL; gloo only for plumbing tests)")
    ap.add_argument("--devices", default="", help="comma-separated HIP device per rank (default: LOCAL_RANK). Repeating a device "
                                                  "is refused with nccl and allowed with gloo (plumbing tests on one GPU)")
    ap.add_argument("--chunks", type=int, default=4, help="chunks of views the assembly pipeline works in")
    ap.add_argument("--assembly-timeout", type=float, default=240.0, help="seconds the assembly legs (N>1) may take before the line is printed without them")
    ap.add_argument("--rendezvous-timeout", type=float, default=180.0, help="seconds init_process_group / a collective may wait for the other ranks (N>1)")
    ap.add_argument("--check", action="store_true", help="add SHA-256 digests of the assembled results (dense and compacted) to the line")
    ap.add_argument("--cpu-sample-rows", type=int, default=0, help="rows of one view timed on the CPU (0 = whole view)")
    ap.add_argument("--dump-outputs", metavar="DIR", default="",
                    help="after the timed steps, write what the last timed launch computed (xyz and valid of every view; a fixed seeded "
                         "sample of the pixels above %d of them) to DIR/{pixel_index,xyz,valid}.npy, float32 / float64, at most 64 MB"
                         % DUMP_MAX_PIXELS)
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.dump_outputs and (args.gpus > 1 or args.idle_only or args.one_view_cold_only or args.families_only):
        ap.error("--dump-outputs writes the outputs of the timed launches of one GPU: not with --gpus > 1 or the *-only modes")
    if args.shim_timing and not args.full:
        ap.error("--shim-timing adds to the side figures of --full: give --full as well")
    return args


class _DevMem:
    """Expose a raw device pointer to torch (zero copy) through the CUDA array interface."""

    def __init__(self, ptr, nbytes):
        self.__cuda_array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (int(ptr), False), "version": 2}


def dev_tensor(torch, ptr, nbytes, dtype, device):
    return torch.as_tensor(_DevMem(ptr, nbytes), device=device).view(dtype)


def usable_cores():
    """Cores this process may really use: the affinity mask, capped by the cgroup CPU quota (cpu.max = "quota period")."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        q, p = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if q != "max":
            n = min(n, max(1, int(int(q) / int(p))))
    except Exception:
        pass
    return n


def cpu_baseline(args, cap, cal, gpu_valid, gpu_xyz):
    """The oracle (CPU restatement of the reference loop: single thread, [col][row] arrays, pow() per bit,
    fenv per pixel, stage-7 tables rebuilt per scan as triangulate() does) timed on one view of the
    same workload; its results also check the GPU output of that view."""
    import numpy as np
    from oracle.oracle import Oracle

    W, H = args.width, args.height
    rows = args.cpu_sample_rows or H
    pv = [p[:rows] for p in cap["planes_v"]]
    ph = [p[:rows] for p in cap["planes_h"]]
    syn = importlib.import_module("3dscan_amd.synth")
    mask = syn.default_mask(W, H)[:rows]
    # above 2^24 pixels the reference's float pixel index (7/triangulation.cpp:264-265) goes wrong; the product uses integer
    # rows / columns, so the oracle is asked for the same there
    big = W * H > (1 << 24)
    o = Oracle(W, rows, W, H, args.ngray, args.ngray, args.fringe_width, args.fringe_width, exact_index=big)
    o.set_mask(mask)
    o.set_calibration(*cal)
    times = []
    for _ in range(5):
        o.invalidate_tables()
        t0 = time.perf_counter()
        o.run_scan(pv, ph)
        times.append(time.perf_counter() - t0)
    t = sorted(times)[len(times) // 2]
    v = o.valid_map(2) == 1
    I = np.s_[0:rows - 3]  # the oracle treats the sample as its own image: skip its last rows
    ok = bool(np.array_equal(gpu_valid[:rows][I] == 1, v[I]))
    ref = o.intersection_points()[I][v[I]]
    got = gpu_xyz[:rows][I][v[I]].astype(np.float64) if ok else None
    rel = float(np.max(np.linalg.norm(got - ref, axis=-1) / np.linalg.norm(ref, axis=-1))) if ok and len(ref) else None
    # (b) of SURVEY 8d: the same maths fused, row-major, OpenMP over rows on all host cores (bit-identical results)
    par = None
    try:
        tp = []
        ncores = usable_cores()
        pxyz, pvalid, nthreads = o.run_scan_rowmajor(pv, ph, threads=ncores)   # warm-up: thread pool, first touch of the outputs
        for _ in range(5):
            t0 = time.perf_counter()
            o.run_scan_rowmajor(pv, ph, threads=ncores, out=(pxyz, pvalid))
            tp.append(time.perf_counter() - t0)
        tpar = sorted(tp)[len(tp) // 2]
        same = bool(np.array_equal(pvalid == 1, v) and np.array_equal(pxyz[v], o.intersection_points().astype(np.float32)[v]))
        par = {"value": round(W * rows / tpar / 1e6, 3), "unit": "Mpixels/s", "cores": int(nthreads),
               "sample": f"same view, fused row-major restatement, OpenMP over rows on the {ncores} cores the cgroup quota / affinity grant "
                         f"(of {os.cpu_count()} visible), median of 5 runs ({tpar:.3f} s each)",
               "bit_identical_to_single_thread": same}
    except Exception as e:
        par = {"error": repr(e)}
    return {
        "value": round(W * rows / t / 1e6, 4), "unit": "Mpixels/s", "cores": 1, "kind": "port", "all_cores": par,
        "sample": f"1 view {W}x{rows} of the same workload (N={args.ngray}, two axes), single thread, reference loop order and "
                  f"[col][row] layout, median of 5 runs ({t:.2f} s each)",
        "gpu_matches_oracle": {"valid_map_bit_exact": ok, "max_rel_point_error": rel},
    }


def rig_calibration(syn, np, rig, W, H, PW, PH):
    cal_d = syn.synth_rig(W, H, PW, PH)
    if rig in ("distorted", "general"):
        cal_d["dp"] = np.array([-0.05, 0.02, 0.001, -0.0005, 0.0])
        cal_d["dc"] = np.array(cal_d["dc"], dtype=np.float64) + np.array([0.0, 0.0, 0.0008, -0.0006, 0.0])
    if rig == "radial":   # a projector with k1, k2 only, as both of the reference's OpenCV projector calibrations are (RIG 3)
        cal_d["dp"] = np.array([-0.05, 0.02, 0.0, 0.0, 0.0])
    if rig == "general":
        Kc = np.array(cal_d["Kc"], dtype=np.float64).reshape(3, 3).copy()
        Kc[0, 1] = 0.35   # skew: the camera matrix is no longer "plain", so the camera-frame solve does not apply (RIG 0)
        cal_d["Kc"] = Kc.ravel()
    if rig == "rig0":     # K[1][0] != 0: not an upper-triangular camera matrix -- the un-pipelined general kernel (rig class 0)
        Kc = np.array(cal_d["Kc"], dtype=np.float64).reshape(3, 3).copy()
        Kc[1, 0] = 1e-3
        cal_d["Kc"] = Kc.ravel()
    return syn.cal_tuple(cal_d)


def steady_rate(sc, n_views, px_per_launch, alg_bytes_px, launches, precondition_ms=200.0, clouds=False):
    """Launch `launches` times back to back after a short preconditioning; -> (Mpx/s, roofline fraction, ms per launch)."""
    run = (lambda: sc.run_clouds(0, n_views)) if clouds else (lambda: sc.run(0, n_views))
    t_pre = time.perf_counter()
    while (time.perf_counter() - t_pre) * 1e3 < precondition_ms:
        for _ in range(20):
            run()
        sc.synchronize()
    sc.timer_start()
    for _ in range(launches):
        run()
    ms = sc.timer_stop() / launches
    return round(px_per_launch / ms / 1e3, 1), round(alg_bytes_px * px_per_launch / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4), round(ms, 4)


def device_copy_rate(torch, dev, nbytes=1 << 30, reps=20):
    """What a plain device-to-device copy reaches on this box (the roofline also against a measured copy bandwidth):
    read + written bytes / time of `reps` copies of 1 GiB, torch events on the current stream."""
    src = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    src.fill_(7)
    dst = torch.empty_like(src)
    for _ in range(3):
        dst.copy_(src)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        dst.copy_(src)
    e1.record()
    e1.synchronize()
    return 2.0 * nbytes * reps / (e0.elapsed_time(e1) * 1e-3) / 1e9


def one_view_cold(args, scm, syn, np, dev_index, launches=2000, clouds=False, serial=False):
    """The reference's real call pattern (m_tech_project_console.cpp:366-395: ONE scan per loop iteration) measured from HBM: `cold_views`
    views are resident (8 x 97.5 MB of frames + 8 x 27 MB of results: three times the 256 MiB Infinity Cache), every launch processes ONE
    view and the next launch a DIFFERENT one, round robin -- by the time a view comes round again 7 x 124 MB have gone through the cache.
    HIP events on the context's stream around `launches` back-to-back launches.  Since round 6 launches that follow each other overlap
    (launch lanes, csrc/sl3d_ctx.h: two internal streams in turn, the tail of one launch under the ramp of the next): launch_us is the
    time per launch of the SERIES -- what a pipelined caller pays per scan -- and `serial` = SL3D_FLAG_SERIAL_LAUNCHES beside it, every
    launch on the one stream: what a LONE launch takes."""
    W, H, N, fw = args.width, args.height, args.ngray, args.fringe_width
    V = max(2, args.cold_views)
    full_mask = syn.default_mask(W, H)
    with scm.Scanner(W, H, W, H, N, N, fw, fw, max_views=V, device=dev_index, serial_launches=serial) as sc:
        sc.set_calibration(*rig_calibration(syn, np, args.rig, W, H, W, H))
        for v in range(V):
            sc.set_mask(full_mask, view=v)
            sc.synth_view(v, plane=(0.75 * v, 0.05, 0.05 - 0.003 * v), view_id=v, noise=args.noise)
        sc.synchronize()
        run = (lambda v: sc.run_clouds(v, 1)) if clouds else (lambda v: sc.run(v, 1))
        t_pre = time.perf_counter()
        while (time.perf_counter() - t_pre) * 1e3 < 200.0:
            for i in range(40):
                run(i % V)
            sc.synchronize()
        sc.timer_start()
        for i in range(launches):
            run(i % V)
        ms = sc.timer_stop() / launches
        on_lanes = sc.launch_counts()[1]
        to_host = None
        if clouds:
            # the consumer the reference has (8/save_point_cloud.cpp:85-104 fills a HOST cloud per scan): launch + the cloud in pinned
            # host memory, wall clock per scan -- the fused kernel, then ONE gap-closing kernel that scans the segment counts on entry
            # and stores over PCIe (which is what bounds it: 12 B per valid point)
            pin = sc.pinned((W * H * 3,), np.float32)
            ts, npts = [], 0
            for i in range(24):
                t0 = time.perf_counter()
                run(i % V)
                npts = sc.download_cloud_into(i % V, pin)
                ts.append(time.perf_counter() - t0)
            t = sorted(ts)[len(ts) // 2]
            to_host = {"us_per_scan": round(t * 1e6, 1), "points": npts, "pcie_GBps": round(12.0 * npts / t / 1e9, 1),
                       "how": "sl3d_run_clouds(1 view) + sl3d_download_clouds into pinned memory, wall clock, median of 24"}
        alg = 20 + 4 * N
        # what this launch really moves: the camera-side table (8 B/px for the radial model of the reference rig, 16 with tangential
        # terms) is read once per LAUNCH, and nothing amortises it when a launch is one view
        tab = sc.camera_table_bytes_per_pixel(1)   # (4 since round 6: the small-launch form of a radial table; 16 with tangential terms)
        if tab is None:
            tab = 8 if args.rig in ("reference", "radial") else 16
        moved = alg + tab
        if serial:
            return {"launch_us": round(ms * 1e3, 2), "frac": round(alg * W * H / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                    "frac_on_moved_bytes": round(moved * W * H / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                    "note": "SL3D_FLAG_SERIAL_LAUNCHES: every launch on the context's one stream (the figure up to round 5; what a lone launch takes)"}
        lone = {} if clouds else {"serial_launches": one_view_cold(args, scm, syn, np, dev_index, launches=launches, serial=True)}
        return {"value": round(W * H / ms / 1e3, 1), "unit": "Mpixels/s", "launch_us": round(ms * 1e3, 2), "kernel": sc.fused_kernel_name(1, clouds=clouds),
                "frac": round(alg * W * H / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4), "algorithmic_bytes_per_pixel": alg,
                "frac_on_moved_bytes": round(moved * W * H / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4), "moved_bytes_per_pixel": moved,
                "resident_views": V, "launches": launches, **({"to_host": to_host} if to_host else {}), **lone,
                "launches_overlap": "consecutive launches run on two internal streams in turn (launch lanes): launch_us = time of the series / launches",
                "launches_on_lanes": on_lanes,
                "note": f"1 view per launch, a different one of {V} resident views each launch (frames + results {V * (alg + 0) * W * H / 2**20:.0f} MiB "
                        f"> 256 MiB Infinity Cache): the frames come from HBM"}


def per_scan_device(args, scm, syn, np, torch, dev_index, scans=400, clouds=False, eager=False, lasso=False, serial=False):
    """What ONE iteration of the reference's scan loop costs on the device once the frames are resident (m_tech_project_console.cpp:
    366-395): a NEW selection mask (image_scissor's result, here already in device memory: no PCIe in this figure) and ONE one-view
    launch, a different resident view and a different mask every scan (frames from HBM, as in one_view_cold).  HIP events on the
    context's stream around `scans` such scans.  Default route (since round 6): ONE launch -- the fused kernel evaluates the selection
    itself (H0 / S3b / S3d: 3/wrapped_phase.cpp:106-115, :253-279 inside k_fused, a MASKIN launch).  eager: the two-kernel route of
    SL3D_FLAG_EAGER_MASK (k_mask_prepare, then the fused kernel); mask_us = that loop with the mask preparation alone.
    lasso: every selection is a rectangle of the share the reference's real captures select (358,580 of 1,920,000 pixels, BASELINE.md
    section 1), at a slightly different place each scan -- the launch then takes the gated kernels, whose plane requests wait for the
    valid bits (the views' previous selections were as sparse: sparse_views)."""
    W, H, N, fw = args.width, args.height, args.ngray, args.fringe_width
    V = max(2, args.cold_views)
    rng = np.random.default_rng(5)
    masks = np.stack([syn.default_mask(W, H) for _ in range(V)])
    for v in range(V):   # every mask differs a little (a few holes), all of them dense: the small-launch kernel, like one_view_cold
        ys, xs = rng.integers(8, H - 8, 12), rng.integers(8, W - 8, 12)
        for y, x in zip(ys, xs):
            masks[v, y:y + 3, x:x + 5] = 0
    if lasso:
        share = 358580.0 / 1920000.0
        mh, mw = int(round(H * share ** 0.5)), int(round(W * share ** 0.5))
        masks[:] = 0
        for v in range(V):
            y0, x0 = (H - mh) // 2 + 3 * v, (W - mw) // 2 + 5 * v
            masks[v, y0:y0 + mh, x0:x0 + mw] = 1
    with scm.Scanner(W, H, W, H, N, N, fw, fw, max_views=V, device=dev_index, eager_mask=eager, serial_launches=serial) as sc:
        sc.set_calibration(*rig_calibration(syn, np, args.rig, W, H, W, H))
        d_masks = torch.from_numpy(masks).to(torch.device("cuda", dev_index))
        torch.cuda.synchronize()
        ptr, vs = d_masks.data_ptr(), W * H
        sc.set_masks_device(ptr, W, vs, 0, V)
        for v in range(V):
            sc.synth_view(v, plane=(0.75 * v, 0.05, 0.05 - 0.003 * v), view_id=v, noise=args.noise)
        sc.synchronize()
        run = (lambda v: sc.run_clouds(v, 1)) if clouds else (lambda v: sc.run(v, 1))

        def scan(i):
            v = i % V
            sc.set_masks_device(ptr + ((i + 3) % V) * vs, W, 0, v, 1)   # view v gets another mask than last time
            run(v)

        t_pre = time.perf_counter()
        while (time.perf_counter() - t_pre) * 1e3 < 200.0:
            for i in range(40):
                scan(i)
            sc.synchronize()
        sc.timer_start()
        for i in range(scans):
            scan(i)
        us = sc.timer_stop() / scans * 1e3
        kernel = sc.last_fused_kernel_name()
        alg = 20 + 4 * N
        out = {"scan_us": round(us, 2), "value": round(W * H / us, 1), "unit": "Mpixels/s",
               "frac": round(alg * W * H / (us * 1e-6) / 1e9 / HBM_PEAK_GBS, 4), "kernel": kernel, "resident_views": V, "scans": scans}
        if lasso:
            out["selected_fraction"] = round(float(masks[0].mean()), 4)
            out["frac"] = None   # (a gated launch moves the planes of the selected quads only: the frame's algorithmic bytes are not its traffic)
        if serial:
            out["note"] = "SL3D_FLAG_SERIAL_LAUNCHES: one launch per scan, every launch on the context's one stream (what a lone scan takes)"
            return out
        if not eager:
            out["launches_per_scan"] = 1
            out["note"] = ("per scan: sl3d_set_masks on a device-resident mask (recorded, nothing launched) + sl3d_run" + ("_clouds" if clouds else "") +
                           " of ONE view, a different view and mask each scan: ONE kernel, which evaluates the selection (the boundary removal of "
                           "stage 3 included) itself and leaves the band / 0-1 planes and the quad count k_mask_prepare would have left; frac = the "
                           "launch's algorithmic bytes (60 B/px) over its time")
            out["launches_overlap"] = ("consecutive scans run on two internal streams in turn (launch lanes): scan_us = time of the series / scans; "
                                       "serial_launches = every launch on the one stream")
            out["serial_launches"] = per_scan_device(args, scm, syn, np, torch, dev_index, scans=scans, clouds=clouds, lasso=lasso, serial=True)
            out["two_kernel_route"] = per_scan_device(args, scm, syn, np, torch, dev_index, scans=scans, clouds=clouds, eager=True, lasso=lasso)
            return out
        sc.timer_start()
        for i in range(scans):
            sc.set_masks_device(ptr + ((i + 3) % V) * vs, W, 0, i % V, 1)
        mask_us = sc.timer_stop() / scans * 1e3
        sc.timer_start()
        for i in range(scans // 8):
            sc.set_masks_device(ptr, W, vs, 0, V)
        batch_us = sc.timer_stop() / (scans // 8) * 1e3
        mask_bytes = W * H + (W + 32) * (H + 4) + W * H      # read the mask, write the 0/1 plane with its halo and the valid-byte plane
        out.update({"launches_per_scan": 2, "mask_us": round(mask_us, 2), "masks_of_%d_views_one_launch_us" % V: round(batch_us, 2),
                    "mask_kernel": {"kernel": "sl3d::k_mask_prepare<4, 16, 64>" if ((W + 15) // 16 * 16) * H > (6 << 20) else "sl3d::k_mask_prepare<4, 4, 256>",
                                    "algorithmic_bytes": mask_bytes,
                                    "frac": round(mask_bytes / (mask_us * 1e-6) / 1e9 / HBM_PEAK_GBS, 4)},
                    "note": "SL3D_FLAG_EAGER_MASK (the route up to round 5): k_mask_prepare + the fused kernel per scan; frac = the fused kernel's "
                            "algorithmic bytes over the time of BOTH kernels"})
        return out


def one_scan_from_idle(args, scm, syn, np, dev_index):
    """The reference's real duty cycle (m_tech_project_console.cpp:331-401): between two scans the loop projects and captures ~46
    frames -- seconds in which the GPU falls back to its idle clocks.  Every sample: sleep `--idle-sleep` seconds, then ONE scan, timed
    on the device (HIP events on the context's stream) and on the host (call to completion):
      resident     : a new pinned mask (sl3d_set_mask) + one one-view launch on frames that are already in HBM
      with_upload  : the Level-2 call as a caller of sl3d.h makes it -- the view's 46 frames from pinned memory (2 x sl3d_set_frames),
                     the mask, the launch
    median and p90 over `--idle-samples` samples each; `steady` = the same calls back to back (no sleep)."""
    W, H, N, fw = args.width, args.height, args.ngray, args.fringe_width
    n, nap = max(3, args.idle_samples), args.idle_sleep
    out = {"sleep_s": nap, "samples": n}
    with scm.Scanner(W, H, W, H, N, N, fw, fw, max_views=2, device=dev_index) as sc:
        sc.set_calibration(*rig_calibration(syn, np, args.rig, W, H, W, H))
        mask = sc.pinned((H, W), np.uint8)
        mask[:] = syn.default_mask(W, H)
        for v in range(2):
            sc.set_mask(mask, view=v)
            sc.synth_view(v, plane=(0.75 * v, 0.05, 0.05), view_id=v, noise=args.noise)
        sc.synchronize()
        fv, fh = sc.frames(0, 0), sc.frames(1, 0)
        pv, ph = sc.pinned((len(fv), H, W), np.uint8), sc.pinned((len(fh), H, W), np.uint8)
        pv[:], ph[:] = np.stack(fv), np.stack(fh)
        lv, lh = list(pv), list(ph)

        def scan(upload, clouds):
            t0 = time.perf_counter()
            sc.timer_start()
            if upload:
                sc.set_frames(0, lv, view=0)
                sc.set_frames(1, lh, view=0)
            sc.set_mask(mask, view=0)
            (sc.run_clouds if clouds else sc.run)(0, 1)
            dev_ms = sc.timer_stop()
            return dev_ms * 1e3, (time.perf_counter() - t0) * 1e6

        def series(upload, clouds, pause):
            dev, host = [], []
            for _ in range(n):
                if pause:
                    sc.synchronize()
                    time.sleep(pause)
                d, h = scan(upload, clouds)
                dev.append(d)
                host.append(h)
            dev.sort(); host.sort()
            return {"device_us": {"median": round(dev[n // 2], 1), "p90": round(dev[(9 * n) // 10], 1)},
                    "host_us": {"median": round(host[n // 2], 1), "p90": round(host[(9 * n) // 10], 1)}}

        for key, (upload, clouds) in (("resident", (False, False)), ("resident_clouds", (False, True)), ("with_upload", (True, False))):
            for _ in range(3):
                scan(upload, clouds)
            out[key] = {"steady": series(upload, clouds, 0.0), "from_idle": series(upload, clouds, nap)}
            s, i = out[key]["steady"]["device_us"]["median"], out[key]["from_idle"]["device_us"]["median"]
            out[key]["idle_penalty"] = round(i / s, 2) if s > 0 else None
    return out


def config2_12mp(args, scm, syn, np, dev_index, W=4096, H=3000, views=3, fw=4, launches=150):
    """BASELINE configs[2]: a 4096x3000 (12.3 Mpx) capture stack on one MI355X, N Gray planes per axis, `views` views resident and
    processed per launch (3 x 737 MB of traffic; the small-launch instantiation at several views per lane), steady state, HIP events."""
    N = args.ngray
    full_mask = syn.default_mask(W, H)
    with scm.Scanner(W, H, W, H, N, N, fw, fw, max_views=views, device=dev_index) as sc:
        sc.set_calibration(*rig_calibration(syn, np, args.rig, W, H, W, H))
        sc.set_masks(full_mask, first_view=0, n_views=views)
        for v in range(views):
            sc.synth_view(v, plane=(0.75 * v, 0.05, 0.05 - 0.003 * v), view_id=v, noise=args.noise)
        sc.run(0, views)      # (the masks are consumed: every timed launch is an ordinary one)
        sc.synchronize()
        v, f, ms = steady_rate(sc, views, views * W * H, 20 + 4 * N, launches)
        return {"value": v, "unit": "Mpixels/s", "frac": f, "ms_per_launch": ms, "width": W, "height": H, "views_per_launch": views,
                "algorithmic_bytes_per_pixel": 20 + 4 * N, "kernel": sc.last_fused_kernel_name(),
                "note": "BASELINE configs[2]: 4096x3000, 3 phase + 2x%d Gray frames per axis, %d views per launch" % (N, views)}


def side_figures(args, scm, syn, np, dev_index, families_only=False):
    """Other instantiations of the same kernel on the same box, steady state, kernel-only (HIP events): never `value`.
    families_only (--families-only, what runs under rocprofv3 for profiles/rNN_families_kernel_stats.csv): the 16-view launches of the
    other kernel families alone -- rig classes 2, 3 and 0, 9 and 14 Gray planes."""
    W, H, N, fw = args.width, args.height, args.ngray, args.fringe_width
    out = {}
    full_mask = syn.default_mask(W, H)

    def ctx(rig, n_gray, views, proj=None, fw_override=None, **kw):
        PW, PH = (proj, min(proj, H)) if proj else (W, H)
        f_ = fw_override or fw
        sc = scm.Scanner(W, H, PW, PH, n_gray, n_gray, f_, f_, max_views=views, device=dev_index, **kw)
        sc.set_calibration(*rig_calibration(syn, np, rig, W, H, PW, PH))
        for v in range(views):
            sc.set_mask(full_mask, view=v)
            sc.synth_view(v, plane=(0.75 * v, 0.05, 0.05 - 0.003 * v), view_id=v, noise=args.noise)
        sc.synchronize()
        return sc

    try:
        if not families_only:
            with ctx("reference", N, 1) as sc:   # the reference's real usage: one view per scan (m_tech_project_console.cpp:372-395)
                v, f, ms = steady_rate(sc, 1, W * H, 20 + 4 * N, 2000)
                out["one_view_cache_resident"] = {"value": v, "unit": "Mpixels/s", "frac_of_hbm_peak_but_served_by_the_infinity_cache": f,
                                                  "launch_us": round(ms * 1e3, 2),
                                                  "note": "the SAME view launched back to back: its 124 MB working set sits in the 256 MiB Infinity Cache, so this is "
                                                          "not an HBM figure (round 3 reported it as one_view_latency); one_view_cold is"}
            out["one_view_cold"] = one_view_cold(args, scm, syn, np, dev_index)
            out["one_view_cold_clouds"] = one_view_cold(args, scm, syn, np, dev_index, launches=1000, clouds=True)
            import torch
            if args.idle_samples > 0:
                out["one_scan_from_idle"] = one_scan_from_idle(args, scm, syn, np, dev_index)
            out["per_scan_device"] = per_scan_device(args, scm, syn, np, torch, dev_index)
            out["per_scan_device_clouds"] = per_scan_device(args, scm, syn, np, torch, dev_index, scans=200, clouds=True)
            out["per_scan_device_19pct_selection"] = per_scan_device(args, scm, syn, np, torch, dev_index, scans=200, lasso=True)
        # (distorted: projector k1,k2,p1,p2 + camera tangential terms; general: a skewed camera matrix as well -- since round 3 both
        # take the pipelined table kernel, RIG 2; the un-pipelined general kernel is left with perspective rows in K)
        for rig, key in (("distorted", "rig2_distorted_projector"), ("general", "rig2_general_skewed_camera"), ("radial", "rig3_radial_projector")):
            with ctx(rig, N, args.views) as sc:
                v, f, ms = steady_rate(sc, args.views, args.views * W * H, 20 + 4 * N, 400)
                out[key] = {"value": v, "unit": "Mpixels/s", "frac": f, "ms_per_launch": ms, "kernel": sc.last_fused_kernel_name()}
        with ctx("reference", N - 1, args.views, proj=min(W, fw << (N - 1))) as sc:   # (a shorter Gray code covers a smaller projector)
            v, f, ms = steady_rate(sc, args.views, args.views * W * H, 20 + 4 * (N - 1), 400)
            out[f"n_gray_{N - 1}"] = {"value": v, "unit": "Mpixels/s", "frac": f, "ms_per_launch": ms, "algorithmic_bytes_per_pixel": 20 + 4 * (N - 1),
                                      "kernel": sc.last_fused_kernel_name()}
        # The kernel families and BASELINE configurations no other figure of this line times (round 5's review): the un-pipelined general
        # kernel (rig class 0: a camera matrix that is not upper triangular), more than 12 Gray planes per axis (the per-plane-test
        # kernels, every rig class on the general kernel), and BASELINE configs[2] (4096x3000, 3 views per launch: what fits beside
        # the headline's buffers).  Each names the instantiation that ran.
        with ctx("rig0", N, args.views) as sc:
            v, f, ms = steady_rate(sc, args.views, args.views * W * H, 20 + 4 * N, 300)
            out["rig0_general"] = {"value": v, "unit": "Mpixels/s", "frac": f, "ms_per_launch": ms, "kernel": sc.last_fused_kernel_name(),
                                   "note": "camera K[1][0] != 0: rig class 0, the un-pipelined kernel that evaluates every rig"}
        with ctx("reference", 14, args.views, fw_override=1) as sc:
            v, f, ms = steady_rate(sc, args.views, args.views * W * H, 20 + 4 * 14, 200)
            out["n_gray_14"] = {"value": v, "unit": "Mpixels/s", "frac": f, "ms_per_launch": ms, "algorithmic_bytes_per_pixel": 20 + 4 * 14,
                                "kernel": sc.last_fused_kernel_name(), "note": "14 Gray planes per axis (fringe width 1): the per-plane-test kernel"}
        if not families_only:
            out["config2_12mp"] = config2_12mp(args, scm, syn, np, dev_index)
    except Exception as e:
        out["error"] = repr(e)
    # the Level-1 drop-in path: the reference's six stage calls + save_point_cloud() through the shim at the reference's own
    # 1600x1200 (tools/shim_bench.cpp: host wall time per scan, BMP files / memory, device-side [col][row] globals vs host transposes)
    # (behind --shim-timing since round 4: it needs a host compiler and disk I/O; the committed figure is profiles/r04_shim_scan_ms.json)
    if args.shim_timing and not families_only:
        try:
            sys.path.insert(0, os.path.join(ROOT, "tools"))
            import shim_timing
            out["shim_scan_ms"] = shim_timing.run(scans=5)
        except Exception as e:
            out["shim_scan_ms"] = {"error": repr(e)}
    return out


_JSON_FD = None


def claim_stdout():
    """fd 1 carries the JSON line and nothing else: from here on whatever a library writes to stdout (Gloo's connection notes, an
    RCCL banner, a stray print) lands on stderr; emit() writes the line to the descriptor stdout was."""
    global _JSON_FD
    if _JSON_FD is None:
        sys.stdout.flush()
        _JSON_FD = os.dup(1)
        os.dup2(2, 1)


def emit(line):
    sys.stdout.flush()
    os.write(_JSON_FD if _JSON_FD is not None else 1, (line + "\n").encode())


def main():
    args = parse()
    claim_stdout()
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    if os.environ.get("NCCL_DEBUG", "").upper() in ("", "VERSION"):
        os.environ["NCCL_DEBUG"] = "WARN"   # no RCCL version banner on stdout next to the JSON line
    dmod = importlib.import_module("3dscan_amd.distributed")   # imports neither torch nor the HIP runtime
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        # plain `python bench.py --gpus N`: this process stays off the GPU and starts the N ranks as fresh children
        out = dmod.spawn_ranks(os.path.abspath(__file__), sys.argv[1:], args.gpus)
        lines = [l for l in out.splitlines() if l.startswith("{")]
        if not lines:
            raise SystemExit("rank 0 printed no JSON line:\n" + out)
        emit(lines[-1])
        return
    rank, local_rank, world = dmod.env_ranks()
    if world != args.gpus:
        raise SystemExit(f"WORLD_SIZE={world} but --gpus {args.gpus}: start with torch.distributed.run --nproc-per-node {args.gpus}, "
                         f"or without it (bench.py then spawns its ranks itself)")

    import numpy as np
    # torch first: its bundled HIP runtime must be the one libsl3d.so binds to (one runtime per process)
    import torch
    import torch.distributed as dist

    ndev = torch.cuda.device_count()   # counting does not initialise the GPU
    devs = [int(d) for d in args.devices.split(",")] if args.devices else list(range(world))
    if len(devs) != world:
        raise SystemExit(f"--devices names {len(devs)} devices for {world} ranks")
    if max(devs) >= ndev:
        raise SystemExit(f"rank {rank}: device {max(devs)} requested but only {ndev} GPU(s) are visible (--gpus {world} needs {world})")
    if world > 1 and args.backend == "nccl" and len(set(devs)) != world:
        raise SystemExit("RCCL needs one GPU per rank: --devices repeats a device (use --backend gloo for single-GPU plumbing tests)")
    dev_index = devs[rank]
    torch.cuda.set_device(dev_index)
    dev = torch.device("cuda", dev_index)
    def identity():
        """what the driver needs to confirm N ranks on N GPUs: the device's PCI bus id and the RCCL this process binds"""
        info = {}
        try:
            p = torch.cuda.get_device_properties(dev_index)
            info["pci_bus_id"] = "%04x:%02x:%02x.0" % (getattr(p, "pci_domain_id", 0), getattr(p, "pci_bus_id", -1) & 0xff, getattr(p, "pci_device_id", 0) & 0xff)
            info["uuid"] = str(getattr(p, "uuid", ""))
        except Exception as e:
            info["pci_bus_id"] = "unknown (%r)" % (e,)
        try:
            info["rccl_version"] = ".".join(str(x) for x in torch.cuda.nccl.version())
        except Exception as e:
            info["rccl_version"] = "unknown (%r)" % (e,)
        return info

    rank_report = [{"rank": 0, "device": dev_index, "gpu": torch.cuda.get_device_name(dev_index), "comm_size": 1, **identity()}]
    if world > 1:
        import datetime
        # a bounded rendezvous: a rank that never shows up (partial node, a rank that died on start) fails the others within
        # --rendezvous-timeout seconds, with a non-zero exit, instead of leaving them in init_process_group
        tmo = datetime.timedelta(seconds=args.rendezvous_timeout)
        if args.backend == "nccl":
            dist.init_process_group("nccl", device_id=dev, timeout=tmo)
        else:
            dist.init_process_group(args.backend, timeout=tmo)
        # what every rank really got: its device and the size of the communicator it is part of, on stderr per rank and
        # (gathered) in rank 0's line -- the first collective of the run, so a broken fabric shows up here, not in the timing
        mine = {"rank": rank, "device": dev_index, "gpu": torch.cuda.get_device_name(dev_index), "comm_size": dist.get_world_size(),
                "backend": dist.get_backend(), "pid": os.getpid(), **identity()}
        print(f"[bench rank {rank}/{world}] device {dev_index} ({mine['gpu']}), communicator of {mine['comm_size']} ranks, backend {mine['backend']}",
              file=sys.stderr, flush=True)
        rank_report = [None] * world
        dist.all_gather_object(rank_report, mine)
        if any(r["comm_size"] != world for r in rank_report) or (args.backend == "nccl" and (len({r["device"] for r in rank_report}) != world or
                                                                                               len({r["pci_bus_id"] for r in rank_report}) != world)):
            raise SystemExit(f"rank {rank}: inconsistent job: {rank_report}")
    red_dev = dev if args.backend == "nccl" else None  # where the tiny timing reductions live

    syn = importlib.import_module("3dscan_amd.synth")
    scm = importlib.import_module("3dscan_amd.scanner")
    W, H, N, fw, V = args.width, args.height, args.ngray, args.fringe_width, args.views
    PW, PH = W, H
    row0, rows = dmod.shard_rows(H, world, rank)
    # weak scaling (default): the batch grows with the GPU count, each GPU holds `rows` rows of every view.  strong: configs[3] itself --
    # a fixed batch of --total-views views, each row-sharded over the N GPUs (at N = 1: all rows of all views on one GPU)
    n_views = args.total_views if args.scaling == "strong" else V * world
    if args.scaling == "strong":
        V = n_views // world if n_views % world == 0 else max(1, n_views // world)   # (views a rotating assembly leaves on each rank)

    if args.idle_only:
        emit(json.dumps({"one_scan_from_idle": one_scan_from_idle(args, scm, syn, np, dev_index)}))
        return
    if args.one_view_cold_only:
        emit(json.dumps({"one_view_cold": one_view_cold(args, scm, syn, np, dev_index, launches=max(args.steps, 200))}))
        return
    if args.families_only:
        emit(json.dumps({"families": side_figures(args, scm, syn, np, dev_index, families_only=True)}))
        return

    # ---- synthetic inputs, generated on the device, resident in HBM before the timed region ----
    # every view is a different plane seen by the same rig, with its own noise stream (sl3d_synth_view / k_synth)
    cal = rig_calibration(syn, np, args.rig, W, H, PW, PH)
    compute_stream = torch.cuda.Stream(device=dev)   # the context launches on it, so torch events can order communication after it
    sc = scm.Scanner(W, rows, PW, PH, N, N, fw, fw, max_views=n_views, device=dev_index, full_size=(W, H), origin=(0, row0),
                     stream=compute_stream.cuda_stream)
    sc.set_calibration(*cal)
    full_mask = syn.default_mask(W, H)
    sc.set_masks(full_mask, 0, n_views)     # one copy, ONE launch of k_mask_prepare for every view
    for v in range(n_views):
        sc.synth_view(v, plane=(0.75 * v, 0.05, 0.05 - 0.003 * v), view_id=v, noise=args.noise)
    sc.synchronize()

    def barrier():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    # before anything has warmed the device: 20 launches from idle clocks, no preconditioning (side.cold_20_steps -- how much of
    # `value` hangs on the preconditioning below is then part of the driver's record).  A plain run launches them too and only
    # leaves the figure out of its line: they are part of the set-up the timed steps follow (over a batch of few views, whose masks
    # are deferred, the first of them is the MASKIN launch that prepares the masks set above), and they take milliseconds
    cold20 = None
    if world == 1:
        sc.timer_start()
        for _ in range(20):
            sc.run(0, n_views)
        cms = sc.timer_stop() / 20
        cold20 = {"value": round(n_views * rows * W / cms / 1e3, 1), "unit": "Mpixels/s", "ms_per_step": round(cms, 4),
                  "frac": round((2 * 3 + 4 * N + 14) * n_views * rows * W / (cms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                  "note": "the first 20 launches of the process, idle clocks, no preconditioning, HIP events"}
    # setup: bring the device out of its idle power state (reported in the JSON; not part of the W + K steps)
    t_pre = time.perf_counter()
    while (time.perf_counter() - t_pre) * 1e3 < args.precondition_ms:
        for _ in range(50):
            sc.run(0, n_views)
        sc.synchronize()
    for _ in range(args.warmup):
        sc.run(0, n_views)
    barrier()
    t0 = time.perf_counter()
    sc.timer_start()                       # HIP event on the stream the kernel is launched on
    for _ in range(args.steps):
        sc.run(0, n_views)
    ev_ms = sc.timer_stop()                # second event, waited for
    kernel_name = sc.last_fused_kernel_name()   # the instantiation the timed launches RAN (recorded by the library at the launch)
    barrier()
    dt = time.perf_counter() - t0
    dt = dmod.max_over_ranks(dt, red_dev)
    ev_ms = dmod.max_over_ranks(ev_ms, red_dev)
    # before any later leg launches on this context again: the results of the last timed launch
    dumped = dump_outputs(np, sc, n_views, rows, W, args.dump_outputs) if args.dump_outputs else None

    px_per_launch = n_views * rows * W                     # pixels one launch processes on one GPU
    px_per_step = n_views * H * W                          # ... and all ranks together
    value = args.steps * px_per_step / dt / 1e6
    alg_bytes_px = 2 * 3 + 4 * N + 1 + 13                  # read 2F+2Nv+2Nh frame bytes + 1 mask, write xyz f32 + valid
    launch_s = ev_ms / 1e3 / args.steps
    achieved = alg_bytes_px * px_per_launch / launch_s / 1e9

    traffic, traffic_src = measured_traffic(px_per_launch) if alg_bytes_px == 60 else (None, None)

    out = {
        "metric": "Mpixels/s decode+unwrap+triangulate @1920×1080",
        "value": round(value, 1), "unit": "Mpixels/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": round(dt / args.steps * 1e3, 4), "higher_is_better": True, "scaling": args.scaling, "vs_baseline": None,
        "dtype": "f64", "data": "synthetic (planes through the reference rig, generated on the device, a different plane and noise stream per view)",
        "config": {"workload": f"configs[1]: {W}x{H} camera, 3 phase-shift + {N} Gray-code bit planes per axis, two axes, "
                               f"Gray frames thresholded against inverse frames (46 frames/view); one step = one fused-kernel "
                               f"launch over {n_views} views ({rows} rows of each) per GPU, frames resident in HBM"
                               + (f"; configs[3]: a fixed batch of {n_views} views row-sharded over {world} GPU(s)" if args.scaling == "strong" else ""),
                   "views_per_gpu_per_step": V, "views_per_step": n_views, "rows_per_gpu": rows, "frames_per_view": 2 * (3 + 2 * N),
                   "projector": f"{PW}x{PH}", "fringe_width": fw, "sharding": "image rows" if world > 1 else "none",
                   "rig": args.rig, "setup_preconditioning_ms": args.precondition_ms},
        "roofline": {"bound": "hbm", "achieved": round(achieved, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                     "frac": round(achieved / HBM_PEAK_GBS, 4),
                     "traffic": traffic, "traffic_source": traffic_src and f"{traffic_src} (committed PMC run of this command, scaled to this launch; not measured in this run)",
                     "kernel": kernel_name, "algorithmic_bytes_per_pixel": alg_bytes_px,
                     "pixels_per_launch": px_per_launch, "avg_launch_ms": round(launch_s * 1e3, 4)},
    }
    if dumped:
        out["dump_outputs"] = dumped

    # end to end from device-resident frames to compacted clouds: ONE launch, the compaction of
    # 8/save_point_cloud.cpp:85-104 happens inside the fused kernel (sl3d_run_clouds), plus the read-back of the counts;
    # a side figure, never `value`
    # Every collective of this leg (barrier, MAX over ranks, the all-ranks-ok vote) sits OUTSIDE the per-rank try blocks and is
    # executed by every rank in the same order whatever happened locally: an exception on one rank can never leave the others
    # in a mismatched collective.  (--full only: a plain run prints the headline without it.)
    if args.full:
        def all_ok(ok):
            return dmod.max_over_ranks(0.0 if ok else 1.0, red_dev) == 0.0

        kernel_name_clouds = sc.fused_kernel_name(n_views, clouds=True)
        cl_err, counts, te, kms = None, [], 0.0, 0.0
        reps = max(20, args.steps // 10)
        if args.no_clouds:
            cl_err = "skipped (--no-clouds)"
        else:
            try:
                for _ in range(20):
                    sc.run_clouds(0, n_views)
                counts = sc.cloud_counts(0, n_views, want_device_copy=False)[2]
            except Exception as e:
                cl_err = repr(e)
        if all_ok(cl_err is None):
            barrier()
            t0 = time.perf_counter()
            try:
                for _ in range(reps):
                    sc.run_clouds(0, n_views)
                    counts = sc.cloud_counts(0, n_views, want_device_copy=False)[2]
            except Exception as e:
                cl_err = repr(e)
            barrier()
            te = dmod.max_over_ranks((time.perf_counter() - t0) / reps, red_dev)
            try:
                sc.timer_start()
                for _ in range(reps):
                    sc.run_clouds(0, n_views)
                kms = sc.timer_stop() / reps
            except Exception as e:
                cl_err = cl_err or repr(e)
            kms = dmod.max_over_ranks(kms, red_dev)
            if not all_ok(cl_err is None):
                cl_err = cl_err or "another rank failed"
        else:
            cl_err = cl_err or "another rank failed"
        if cl_err is None:
            vf = sum(counts) / float(px_per_launch)
            cl_bytes_px = 2 * 3 + 4 * N + 1 + 1 + 12 * vf   # frames + mask byte read, valid byte + 12 B per VALID pixel written
            cl_achieved = cl_bytes_px * px_per_launch / (kms * 1e-3) / 1e9
            cl_traffic, cl_traffic_src = measured_traffic(px_per_launch, "clouds") if alg_bytes_px == 60 else (None, None)
            out["to_compacted_clouds"] = {"value": round(px_per_step / te / 1e6, 1), "unit": "Mpixels/s", "ms_per_step": round(te * 1e3, 4),
                                          "kernel_only": {"value": round(px_per_step / kms / 1e3, 1), "ms_per_launch": round(kms, 4)},
                                          "valid_points_per_step_rank0": int(sum(counts)), "valid_fraction_rank0": round(vf, 4),
                                          "algorithmic_bytes_per_pixel": round(cl_bytes_px, 2),
                                          "roofline": {"bound": "hbm", "achieved": round(cl_achieved, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                                       "frac": round(cl_achieved / HBM_PEAK_GBS, 4), "traffic": cl_traffic,
                                                       "traffic_source": cl_traffic_src and f"{cl_traffic_src} (committed PMC run of this command, scaled to this launch; not measured in this run)",
                                                       "kernel": kernel_name_clouds, "launches": "the fused kernel + k_seg_scan (both between the HIP events)",
                                                       "avg_launch_ms": round(kms, 4)},
                                          "how": "sl3d_run_clouds: the fused kernel writes SEGMENTED ordered clouds (every wave compacts its 256 scan pixels into its own "
                                                 "slot: no tile waits for another) + one scan launch for offsets and totals; value = launches + the wait for the "
                                                 "per-view counts; kernel_only = both launches between HIP events"}
        else:
            out["to_compacted_clouds"] = {"error": cl_err}

    digests = {}
    if world > 1 and not args.no_assemble:
        # The assembly legs talk RCCL point to point between all ranks; `value` above is already measured.  Should a leg ever
        # stall (a fabric problem on the node), the line is still printed: after --assembly-timeout seconds every rank leaves,
        # rank 0 with the line it has.
        import threading

        def give_up():
            if rank == 0:
                out["with_assembly"] = {"error": f"assembly legs did not finish within {args.assembly_timeout} s"}
                out["compute_only"] = {"value": out["value"], "unit": "Mpixels/s", "ms_per_step": out["ms_per_step"]}
                out["value"], out["ms_per_step"], out["value_is"] = 0.0, None, "no assembled variant was measured (timeout)"
                out["ranks"] = rank_report
                emit(json.dumps(out))
            os._exit(3)   # non-zero on every rank: the launcher (spawn_ranks / torchrun / CI) must see that the run did not complete

        watchdog = threading.Timer(args.assembly_timeout, give_up)
        watchdog.daemon = True
        watchdog.start()
        out["with_assembly"] = measure_assembly(args, torch, dist, dmod, sc, compute_stream, dev, n_views, V, rows, W, H, rank, world, px_per_step, digests)
        watchdog.cancel()
        # N > 1: `value` is what a consumer of the ASSEMBLED result gets -- compute AND the exchange that puts every view's stripes
        # together, --steps steps between barriers, MAX over ranks -- not the compute-only rate, which is 8 x one GPU by construction
        # (the stripes never talk to each other while they compute) and moves to `compute_only`
        wa = out["with_assembly"]
        out["compute_only"] = {"value": out["value"], "unit": "Mpixels/s", "ms_per_step": out["ms_per_step"],
                               "note": "the fused kernel on every rank's stripe, no exchange: scales with N by construction; not the headline"}
        if wa.get("headline"):
            h = wa[wa["headline"]]
            out["value"], out["ms_per_step"], out["value_is"] = h["headline_value"], h["headline_ms_per_step"], wa["headline"]
        else:   # no assembled variant could be measured: the line says so and carries NO throughput claim
            out["value"], out["ms_per_step"], out["value_is"] = 0.0, None, "no assembled variant was measured: " + str(wa.get("error"))
    elif world > 1:
        out["value_is"] = "compute_only (--no-assemble): NOT an assembled figure"
    elif args.check:
        digests = single_rank_digests(np, sc, n_views)
    if args.check:
        out["check"] = digests

    if rank == 0 and world == 1 and args.full and not args.no_side:
        out["side"] = side_figures(args, scm, syn, np, dev_index)
        out["side"]["cold_20_steps"] = cold20
        try:   # the same roofline against what a device copy reaches on this very box, right now (never `frac`)
            copy = device_copy_rate(torch, dev)
            out["roofline"]["device_copy"] = {"GBps": round(copy, 1), "frac_of_it": round(achieved / copy, 4),
                                              "how": "torch copy_ of 1 GiB device to device, (read + written bytes) / time, 20 copies"}
        except Exception as e:
            out["roofline"]["device_copy"] = {"error": repr(e)}

    if rank == 0 and world == 1 and args.full and not args.no_cpu_baseline:
        sc.run(0, n_views)
        xyz, valid = sc.points(0)
        try:
            cap0 = {"planes_v": sc.frames(0, 0), "planes_h": sc.frames(1, 0)}  # the very bytes the GPU processed
            out["cpu_baseline"] = cpu_baseline(args, cap0, cal, valid, xyz)
            # what the C ABI delivers when the boundary hands over HOST buffers (never `value`):
            # (a) serial: upload of the 46 frames of one view, one launch, download of xyz + valid, pageable numpy memory
            stack_v, stack_h = np.stack(cap0["planes_v"]), np.stack(cap0["planes_h"])   # planes back to back: one 2-D copy per axis
            ts = []
            for _ in range(5):
                t0 = time.perf_counter()
                sc.set_frames(0, list(stack_v), view=0)
                sc.set_frames(1, list(stack_h), view=0)
                sc.run(0, 1)
                sc.points(0)
                ts.append(time.perf_counter() - t0)
            t = sorted(ts)[2]
            out["host_buffers_one_view"] = {"value": round(W * rows / t / 1e6, 1), "unit": "Mpixels/s", "ms": round(t * 1e3, 2),
                                            "note": "H2D of 46 frames (one 2-D copy per axis) + launch + D2H of xyz and valid for ONE view, pageable host memory"}
            # (b) pipelined: sl3d_process_views, 12 host-resident views through the view slots on three HIP streams, pinned memory
            nv = 12
            fr = sc.pinned((nv, 2 * (3 + 2 * N), rows, W), np.uint8)
            fr[:] = np.stack(cap0["planes_v"] + cap0["planes_h"])[None]
            px = sc.pinned((nv, rows, W, 3), np.float32)
            pv = sc.pinned((nv, rows, W), np.uint8)
            sc.process_views(fr, xyz=px, valid=pv)
            ts = []
            for _ in range(3):
                t0 = time.perf_counter()
                sc.process_views(fr, xyz=px, valid=pv)
                ts.append(time.perf_counter() - t0)
            t = sorted(ts)[1]
            same = bool(np.array_equal(pv[nv - 1], valid) and np.array_equal(px[nv - 1], xyz, equal_nan=True))
            out["host_buffers_pipelined"] = {"value": round(nv * W * rows / t / 1e6, 1), "unit": "Mpixels/s", "ms_per_view": round(t / nv * 1e3, 2),
                                             "note": f"{nv} host-resident views, upload / kernel / download overlapped on 3 streams, pinned memory",
                                             "equals_resident_result": same}
            # (c) the per-scan mask hand-over of the reference's loop (selected_region changes every scan)
            pm = sc.pinned(full_mask.shape, np.uint8)
            pm[:] = full_mask
            for name, src in (("pinned", pm), ("pageable", full_mask)):
                sc.synchronize()
                ts = []
                for _ in range(20):
                    t0 = time.perf_counter()
                    sc.set_mask(src, view=0)
                    tcall = time.perf_counter() - t0
                    sc.synchronize()
                    ts.append((tcall, time.perf_counter() - t0))
                ts.sort()
                out.setdefault("set_mask_us", {})[name] = {"call": round(ts[10][0] * 1e6, 1), "until_ready": round(sorted(x[1] for x in ts)[10] * 1e6, 1)}
        except Exception as e:  # the baseline must never take the GPU number down with it
            out["cpu_baseline"] = {"error": repr(e)}
    sc.close()
    if world > 1:
        out["ranks"] = rank_report
    if rank == 0:
        emit(json.dumps(out))
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def single_rank_digests(np, sc, n_views):
    """SHA-256 of what an assembly on rank 0 must reproduce: the dense xyz + valid planes and the compacted clouds of every view."""
    sc.run(0, n_views)
    hd, hc = hashlib.sha256(), hashlib.sha256()
    for v in range(n_views):
        xyz, val = sc.points(v)
        hd.update(xyz.tobytes()); hd.update(val.tobytes())
    for c in sc.fused_clouds(0, n_views):
        hc.update(c.tobytes())
    return {"dense_sha256": hd.hexdigest(), "compact_sha256": hc.hexdigest()}


def dump_outputs(np, sc, n_views, rows, W, out_dir, seed=0):
    """--dump-outputs: what a caller of the timed launch receives, the dense xyz and the valid map of every view, as DIR/xyz.npy
    (n, 3) float32 (0 where the pixel is invalid) and DIR/valid.npy (n,) float32 (0 / 1).  DIR/pixel_index.npy (n,) float64 holds
    each pixel's flat index into [view][row][col]: every pixel up to DUMP_MAX_PIXELS, above that a sorted sample drawn with a
    fixed seed, so two runs with the same arguments write the same pixels."""
    px_view = rows * W
    total = n_views * px_view
    if total <= DUMP_MAX_PIXELS:
        idx = np.arange(total, dtype=np.int64)
    else:
        idx = np.sort(np.random.default_rng(seed).choice(total, size=DUMP_MAX_PIXELS, replace=False))
    xyz = np.empty((len(idx), 3), dtype=np.float32)
    valid = np.empty(len(idx), dtype=np.float32)
    bounds = np.searchsorted(idx, np.arange(n_views + 1) * px_view)
    for v in range(n_views):
        lo, hi = bounds[v], bounds[v + 1]
        if lo < hi:
            p, m = sc.points(v)
            local = idx[lo:hi] - v * px_view
            xyz[lo:hi] = p.reshape(-1, 3)[local]
            valid[lo:hi] = m.reshape(-1)[local]
    # the library's NaN marks an invalid pixel, which valid.npy already says: the files hold finite numbers only (a NaN at a
    # VALID pixel would be a defect and is kept)
    xyz[valid == 0] = 0.0
    os.makedirs(out_dir, exist_ok=True)
    np.save(os.path.join(out_dir, "pixel_index.npy"), idx.astype(np.float64))
    np.save(os.path.join(out_dir, "xyz.npy"), xyz)
    np.save(os.path.join(out_dir, "valid.npy"), valid)
    return {"dir": out_dir, "files": ["pixel_index.npy", "xyz.npy", "valid.npy"], "pixels": int(len(idx)), "of_pixels": int(total),
            "sample_seed": seed if len(idx) < total else None}


def syn_full_mask(W, H):
    import importlib
    return importlib.import_module("3dscan_amd.synth").default_mask(W, H)


def measure_assembly(args, torch, dist, dmod, sc, compute_stream, dev, n_views, V, rows, W, H, rank, world, px_per_step, digests):
    """End to end WITH the assembly of the clouds on rank 0 (the north star's single gather), pipelined: the batch is cut
    into chunks of views; chunk k's stripes leave on the communication stream (one grouped batch of sends that land in place
    in the root's dense planes) while the compute stream already runs chunk k+1.  dense = xyz + valid (13 B/px);
    compact = the valid points only, compacted by the fused kernel (counts first).  Also the rotating-roots all_to_all
    (every rank assembles its share of the views: all links busy), as one blocking collective after the compute.
    A plain run times the dense variants only, the candidates for the headline (and compact when --check digests it); --full adds
    host_parallel, compact, compact on a 19 % selection and the whole-views sharding."""
    res = {}
    nccl = args.backend == "nccl"
    import numpy as np_mod
    try:
        b = sc.device_buffers()
        pitch = b.frame_pitch
        pts = dev_tensor(torch, b.points, n_views * b.points_view_stride, torch.float32, dev).view(n_views, rows, pitch * 3)
        val = dev_tensor(torch, b.valid, n_views * b.valid_view_stride, torch.uint8, dev).view(n_views, rows, pitch)
        rows_by_rank = [dmod.shard_rows(H, world, r)[1] for r in range(world)]
        asm = dmod.RootAssembler(rows_by_rank)
        comm = asm.comm_stream
        root = rank == 0
        out_pts = torch.empty((n_views, H, pitch * 3), dtype=torch.float32, device=dev) if root else None
        out_val = torch.empty((n_views, H, pitch), dtype=torch.uint8, device=dev) if root else None
        nchunks = max(1, min(args.chunks, n_views))
        bounds = [n_views * k // nchunks for k in range(nchunks + 1)]
        chunks = [(bounds[k], bounds[k + 1] - bounds[k]) for k in range(nchunks) if bounds[k + 1] > bounds[k]]
        ev_run = [torch.cuda.Event() for _ in chunks]
        ev_comm = [torch.cuda.Event() for _ in chunks]

        def barrier():
            dist.barrier()
            torch.cuda.synchronize()

        def timed(step, reps):
            step(first=True)
            barrier()
            t0 = time.perf_counter()
            for _ in range(reps):
                step(first=False)
            comm.synchronize()
            barrier()
            return dmod.max_over_ranks((time.perf_counter() - t0) / reps, dev if nccl else None)

        steps_of = {}   # variant -> its step function (the headline variant is timed once more, for exactly --steps steps)

        # ---- dense: xyz + valid of every stripe to rank 0 ----
        def dense_step(first):
            for k, (f, n) in enumerate(chunks):
                if not first:
                    compute_stream.wait_event(ev_comm[k])      # the chunk's results may be overwritten only once they have left
                sc.run(f, n)
                ev_run[k].record(compute_stream)
                with torch.cuda.stream(comm):
                    comm.wait_event(ev_run[k])
                    asm.gather_dense(range(f, f + n), pts, val, out_pts, out_val)
                    ev_comm[k].record(comm)

        reps = max(3, min(50, args.steps // 40))
        steps_of["dense_root_gather"] = dense_step
        t = timed(dense_step, reps)
        res["dense_root_gather"] = {"value": round(px_per_step / t / 1e6, 1), "unit": "Mpixels/s", "ms_per_step": round(t * 1e3, 3),
                                    "bytes_into_root_per_step": int((n_views * (H - rows_by_rank[0]) * pitch * 13)),
                                    "chunks": len(chunks), "overlapped_with_compute": True}
        if args.check and root:
            h = hashlib.sha256()
            for v in range(n_views):
                h.update(out_pts[v].view(H, pitch, 3)[:, :W].contiguous().cpu().numpy().tobytes())
                h.update(out_val[v][:, :W].contiguous().cpu().numpy().tobytes())
            digests["dense_sha256"] = h.hexdigest()

        if args.full:
            # ---- host_parallel: the reference's consumer is the HOST -- every rank downloads its own rows of every view over its own
            # GPU's PCIe link (what sl3d_group_download_points does for a single-process caller), no xGMI hop to a root ----
            try:
                hp = sc.pinned((n_views, rows, W, 3), np_mod.float32)
                hv = sc.pinned((n_views, rows, W), np_mod.uint8)
                herr = None
            except Exception as e:
                herr = repr(e)

            def host_step(first):
                for k, (f, n) in enumerate(chunks):
                    sc.run(f, n)
                if herr is None:
                    sc.download_views(0, n_views, hp, hv)     # 2-D copies on the compute stream, then one wait

            if herr is None:
                steps_of["host_parallel"] = host_step   # (measured and reported; never a headline candidate: see the end of this function)
            t = timed(host_step, max(2, reps // 4))
            res["host_parallel"] = ({"value": round(px_per_step / t / 1e6, 1), "unit": "Mpixels/s", "ms_per_step": round(t * 1e3, 3),
                                     "bytes_to_host_per_rank_per_step": int(n_views * rows * W * 13),
                                     "note": "every rank: fused kernel, then its own rows of every view D2H into pinned host memory over its own PCIe link"}
                                    if herr is None else {"error": herr})

        if args.full or args.check:   # (never a headline candidate; --check digests it)
            # ---- compact: the valid points only, compacted by the fused kernel ----
            sc.run_clouds(0, n_views)
            cptr, cstride, _ = sc.cloud_counts(0, n_views)
            clouds = dev_tensor(torch, cptr, n_views * cstride * 12, torch.float32, dev)
            out_cloud = torch.empty(n_views * H * pitch * 3, dtype=torch.float32, device=dev) if root else None
            state = {}

            def compact_step(first):
                off = 0
                offs_all, counts_all = [], []
                for k, (f, n) in enumerate(chunks):
                    if not first:
                        compute_stream.wait_event(ev_comm[k])
                    sc.run_clouds(f, n)
                    counts = sc.cloud_counts(f, n)[2]                # waits for this chunk's kernel: the payload sizes come from it
                    with torch.cuda.stream(comm):
                        allc = asm.gather_counts(counts)
                        tot = [sum(allc[r][i] for r in range(world)) for i in range(n)]
                        offs = [3 * (off + sum(tot[:i])) for i in range(n)]
                        asm.gather_compact(range(f, f + n), clouds, cstride, allc, out_cloud, offs)
                        ev_comm[k].record(comm)
                    offs_all += offs
                    counts_all += tot
                    off += sum(tot)
                state["offs"], state["counts"] = offs_all, counts_all

            steps_of["compact_root_gather"] = compact_step
            t = timed(compact_step, reps)
            res["compact_root_gather"] = {"value": round(px_per_step / t / 1e6, 1), "unit": "Mpixels/s", "ms_per_step": round(t * 1e3, 3),
                                          "points_per_step": int(sum(state["counts"])), "chunks": len(chunks), "overlapped_with_compute": True}
            if args.check and root:
                h = hashlib.sha256()
                for o, c in zip(state["offs"], state["counts"]):
                    h.update(out_cloud[o:o + 3 * c].cpu().numpy().tobytes())
                digests["compact_sha256"] = h.hexdigest()

        if args.full:
            # ---- the same on the reference's own kind of selection: 358,580 of 1,920,000 pixels (18.7 %) lie inside the lasso of its real
            # captures -- the one case in which the north star's SINGLE-root gather carries a fifth of the bytes.
            # Every view gets a centred rectangle of that share; afterwards the full-frame masks are back.
            try:
                share = 358580.0 / 1920000.0
                mh, mw = int(round(H * share ** 0.5)), int(round(W * share ** 0.5))
                lasso = np_mod.zeros((H, W), np_mod.uint8)
                lasso[(H - mh) // 2:(H - mh) // 2 + mh, (W - mw) // 2:(W - mw) // 2 + mw] = 1
                sc.set_masks(lasso, 0, n_views)
                t = timed(compact_step, reps)
                res["compact_root_gather_19pct_selection"] = {"value": round(px_per_step / t / 1e6, 1), "unit": "Mpixels/s", "ms_per_step": round(t * 1e3, 3),
                                                              "points_per_step": int(sum(state["counts"])), "selected_fraction": round(float(lasso.mean()), 4),
                                                              "note": "compact_root_gather with the share of the frame the reference's real captures select; never the headline"}
            except Exception as e:
                res["compact_root_gather_19pct_selection"] = {"error": repr(e)}
            finally:
                sc.set_masks(syn_full_mask(W, H), 0, n_views)
                sc.run(0, n_views)
                sc.synchronize()

        # ---- rotating roots: one all_to_all after the compute (every rank assembles V of the views) ----
        if nccl and n_views == V * world:   # (a strong-scaled batch that does not divide by N has no equal shares to rotate)
            def rot_step(first):
                sc.run(0, n_views)
                ev_run[0].record(compute_stream)
                torch.cuda.current_stream().wait_event(ev_run[0])
                dmod.assemble_rotating(pts, V)
                dmod.assemble_rotating(val, V)
                torch.cuda.current_stream().synchronize()
            steps_of["dense_rotating_all_to_all"] = rot_step
            t = timed(rot_step, reps)
            res["dense_rotating_all_to_all"] = {"value": round(px_per_step / t / 1e6, 1), "unit": "Mpixels/s", "ms_per_step": round(t * 1e3, 3),
                                                "overlapped_with_compute": False,
                                                "note": "every rank assembles the views v with v mod N == rank (dense planes): all links carry traffic, no single root"}
            # the same exchange PIPELINED: chunk k's all_to_all on the communication stream while chunk k + 1 computes; view i of a
            # chunk goes to rank i % N (every chunk uses every link)
            if all(n % world == 0 for _, n in chunks):
                def rot_pipe_step(first):
                    for k, (f, n) in enumerate(chunks):
                        if not first:
                            compute_stream.wait_event(ev_comm[k])
                        sc.run(f, n)
                        ev_run[k].record(compute_stream)
                        with torch.cuda.stream(comm):
                            comm.wait_event(ev_run[k])
                            state["rot"] = (dmod.assemble_rotating_interleaved(pts[f:f + n], rows_by_rank),
                                            dmod.assemble_rotating_interleaved(val[f:f + n], rows_by_rank))
                            ev_comm[k].record(comm)
                steps_of["dense_rotating_pipelined"] = rot_pipe_step
                t = timed(rot_pipe_step, reps)
                res["dense_rotating_pipelined"] = {"value": round(px_per_step / t / 1e6, 1), "unit": "Mpixels/s", "ms_per_step": round(t * 1e3, 3),
                                                   "chunks": len(chunks), "overlapped_with_compute": True,
                                                   "note": "view i of a chunk is assembled on rank i mod N: one all_to_all per chunk on the communication stream"}
        if args.full:
            # ---- the OTHER sharding of a batch of independent views ("implement the specified one, measure both"): whole views
            # per GPU instead of row stripes -- rank r takes V whole views, every view's dense planes are complete on one GPU (the very
            # end state of the rotating assemblies above) and NOTHING is exchanged.  Reported beside the row-sharded variants, never the
            # headline: BASELINE's configs[3] and the north star specify row stripes + a gather
            try:
                import importlib
                syn_ = importlib.import_module("3dscan_amd.synth")
                scm_ = importlib.import_module("3dscan_amd.scanner")
                with scm_.Scanner(W, H, W, H, args.ngray, args.ngray, args.fringe_width, args.fringe_width, max_views=V, device=dev.index) as sw:
                    sw.set_calibration(*rig_calibration(syn_, np_mod, args.rig, W, H, W, H))
                    sw.set_masks(syn_.default_mask(W, H), 0, V)
                    for j in range(V):
                        vid = rank * V + j
                        sw.synth_view(j, plane=(0.75 * vid, 0.05, 0.05 - 0.003 * vid), view_id=vid, noise=args.noise)
                    for _ in range(5):
                        sw.run(0, V)
                    sw.synchronize()

                    def whole_step(first):
                        sw.run(0, V)
                        if first:
                            sw.synchronize()

                    def timed_whole(reps):
                        whole_step(True)
                        barrier()
                        t0 = time.perf_counter()
                        for _ in range(reps):
                            whole_step(False)
                        sw.synchronize()
                        barrier()
                        return dmod.max_over_ranks((time.perf_counter() - t0) / reps, dev if nccl else None)

                    t = timed_whole(max(reps, args.steps))
                    res["whole_views_no_exchange"] = {"value": round(px_per_step / t / 1e6, 1), "unit": "Mpixels/s", "ms_per_step": round(t * 1e3, 4),
                                                      "note": f"the other sharding of the same batch: {V} WHOLE views per GPU instead of row stripes of {n_views}; every view is "
                                                              "complete on one GPU (the end state of the rotating assemblies) with no exchange at all; not the headline"}
            except Exception as e:
                res["whole_views_no_exchange"] = {"error": repr(e)}
        # ---- the headline of an N > 1 line: the best ASSEMBLED variant, timed once more over exactly --steps steps between barriers
        # (the calibration runs above decide which; the choice is the same on every rank: the figures are MAX-over-ranks already) ----
        # Candidates: only variants that leave COMPLETE DENSE views on a rank -- the gather to the root and the rotating assemblies.
        # host_parallel (every rank keeps its own rows in its own host buffer: nobody holds an assembled view) and compact_root_gather
        # (another payload: clouds, not dense planes) are reported beside it, never as `value`.  The choice is rank 0's,
        # handed to every rank: a variant that failed on ONE rank only must not make the ranks time different collectives.
        names = sorted(k for k in steps_of if k.startswith("dense_"))
        ok_here = [1.0 if "value" in res.get(k, {}) else 0.0 for k in names]
        ok_all = [dmod.max_over_ranks(-x, dev if nccl else None) == -1.0 for x in ok_here]   # (min over ranks through the max reduction)
        cand = [k for k, ok in zip(names, ok_all) if ok]
        pick = float(names.index(max(cand, key=lambda k: res[k]["value"]))) if (cand and rank == 0) else -1.0
        pick = int(dmod.max_over_ranks(pick, dev if nccl else None))
        best = names[pick] if pick >= 0 else None
        if best is not None:
            t = timed(steps_of[best], args.steps)
            res[best]["headline_value"] = round(px_per_step / t / 1e6, 1)
            res[best]["headline_ms_per_step"] = round(t * 1e3, 4)
            res["headline"] = best
    except Exception as e:
        import traceback
        res["error"] = repr(e) + " | " + traceback.format_exc().splitlines()[-3].strip()
    return res


if __name__ == "__main__":
    main()
