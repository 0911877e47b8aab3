#!/usr/bin/env python3
"""Generates the committed golden fixtures from the reference's own data artefacts.

Run in the build container only (it reads /root/reference, which does not exist
on the GPU box):   python tests/golden/make_golden.py

What it does
 1. Loads the real 1600x1200 captures stage 3/4 compute on (the Gray_captured_image_*.bmp
    re-saves of 3/wrapped_phase.cpp:46-52 and 4/phase_unwrap.cpp:79-86,118-125) and the four
    known-answer images the reference wrote (Wrapped_phase_image.bmp, Unwrapped_phase_*.bmp).
 2. PINS THE ORACLE: replays oracle stages 3 and 4 on the full frames and requires the debug
    images to equal the reference's KAT images on every pixel (358,580 valid px per axis).
 2b. PINS T0: the oracle's cvRodrigues2 / cvTranspose / cvGEMM restatements must reproduce, bit for bit, the 12 doubles of
    Triangulation/Relative_geometry/proj_cam_rot_mat.xml + proj_cam_trans_vect.xml that the reference's stage 6 computed with
    OpenCV itself from the rotation / translation vectors stage 7 reads (6/system_calibration.cpp:1488-1516).
 3. Runs oracle stages 5 and 7 on the full frames with the reference's 8 calibration XMLs
    (unpinned stages: these outputs are regression goldens, not reference answers) and CORROBORATES them with an
    independent fp64 NumPy restatement of the same stages (independent_stage_5_7: no code shared with oracle/):
    identical 355,608 correspondences and 3-D points within 1e-12 of their norm are required on the full scan.
 4. Writes small crops (inputs + expected outputs) to tests/golden/*.npz and the calibration
    to tests/golden/calibration.json.  Only derived data is written: no reference source.
 5. PINS THE PATTERN GENERATOR (N1): the oracle's fringe / Gray / inverse-Gray / binary patterns must equal the 45
    pattern images the reference generated (Generated_patterns/**) on every pixel; their 1-D profiles go to
    tests/golden/patterns_ref.npz  (`python tests/golden/make_golden.py patterns` runs this step alone).
 6. PINS T0-T3 AND O1 on the reference's own point cloud (Point_cloud/test data/point_cloud_2.ply): the integer tuple of every
    vertex, per-coordinate byte tables of a capture that decodes to them, and the oracle's literal stages 3 -> 8 reproducing the
    PLY's floats in order; writes tests/golden/ply_stage7.npz  (`python tests/golden/make_golden.py ply` runs this step alone).
"""
import json
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
from oracle.oracle import Oracle  # noqa: E402

REF = "/root/reference/M_tech_project_console/"
W, H, PW, PH = 1600, 1200, 1280, 720          # global_cv.h:49-53
N_V, N_H, FW, NCODES_V, NCODES_H = 6, 5, 32, 40, 23  # common_variables.h:6-9,23-24


def bmp(path):
    from PIL import Image
    im = Image.open(REF + path)
    assert im.mode == "L" and im.size == (W, H), (path, im.mode, im.size)
    return np.array(im)


def xml_data(path):
    txt = open(REF + path).read()
    return [float(x) for x in re.search(r"<data>(.*?)</data>", txt, re.S).group(1).split()]


def dilate3(m):
    p = np.pad(m, 1)
    out = np.zeros_like(m)
    for dy in range(3):
        for dx in range(3):
            out |= p[dy:dy + m.shape[0], dx:dx + m.shape[1]]
    return out


def erode3(m):
    p = np.pad(m, 1)
    out = np.ones_like(m)
    for dy in range(3):
        for dx in range(3):
            out &= p[dy:dy + m.shape[0], dx:dx + m.shape[1]]
    return out


def shift(m, dx, dy):
    out = np.zeros_like(m)
    h, w = m.shape
    out[max(dy, 0):h + min(dy, 0), max(dx, 0):w + min(dx, 0)] = m[max(-dy, 0):h + min(-dy, 0), max(-dx, 0):w + min(-dx, 0)]
    return out


def independent_projection_matrices(cal):
    """T0 of independent_stage_5_7: Rodrigues (cvRodrigues2, vector -> matrix) and A = K [R|t] for camera and projector."""
    f64 = np.float64

    def rodrigues(r):
        r = np.asarray(r, f64)
        th = np.sqrt(r @ r)
        if th < np.finfo(f64).eps:
            return np.eye(3)
        k = r / th
        Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
        return np.cos(th) * np.eye(3) + (1 - np.cos(th)) * np.outer(k, k) + np.sin(th) * Kx

    def proj_matrix(K, r, t):
        return np.asarray(K, f64).reshape(3, 3) @ np.hstack([rodrigues(r), np.asarray(t, f64).reshape(3, 1)])

    return proj_matrix(cal["Kc"], cal["rc"], cal["tc"]), proj_matrix(cal["Kp"], cal["rp"], cal["tp"])


def independent_undistort_reproject(u, v, K, d):
    """T1 of independent_stage_5_7: cvUndistortPoints (5 fixed-point iterations, no R / P) then K (x, y, 1) and the division by w."""
    f64 = np.float64
    K = np.asarray(K, f64).reshape(3, 3)
    k1, k2, p1, p2, k3 = [f64(c) for c in d]
    x0 = (u - K[0, 2]) / K[0, 0]
    y0 = (v - K[1, 2]) / K[1, 1]
    xx, yy = x0.copy(), y0.copy()
    for _ in range(5):
        r2 = xx * xx + yy * yy
        icdist = 1.0 / (1.0 + ((k3 * r2 + k2) * r2 + k1) * r2)
        dx = 2 * p1 * xx * yy + p2 * (r2 + 2 * xx * xx)
        dy = p1 * (r2 + 2 * yy * yy) + 2 * p2 * xx * yy
        xx = (x0 - dx) * icdist
        yy = (y0 - dy) * icdist
    h = np.stack([xx, yy, np.ones_like(xx)], -1) @ K.T
    return h[..., 0] / h[..., 2], h[..., 1] / h[..., 2]


def independent_triangulate(c, r, x, y, cal, Ac, Ap, undist=None):
    """T1-T3 of independent_stage_5_7 on integer tuples (camera col c, row r, projector x, y) -> fp64 points [n, 3].
    undist: optional (camera u, v [H, W], projector u, v [PH, PW]) tables of independent_undistort_reproject (the same values)."""
    f64 = np.float64
    if undist is None:
        uc, vc = independent_undistort_reproject(np.asarray(c, f64), np.asarray(r, f64), cal["Kc"], cal["dc"])
        up, vp = independent_undistort_reproject(np.asarray(x, f64), np.asarray(y, f64), cal["Kp"], cal["dp"])
    else:
        uc, vc, up, vp = undist[0][r, c], undist[1][r, c], undist[2][y, x], undist[3][y, x]
    # T2: P (4x3), F (4)
    P = np.stack([Ac[0, :3] - uc[:, None] * Ac[2, :3], Ac[1, :3] - vc[:, None] * Ac[2, :3],
                  Ap[0, :3] - up[:, None] * Ap[2, :3], Ap[1, :3] - vp[:, None] * Ap[2, :3]], axis=1)
    Fv = np.stack([Ac[2, 3] * uc - Ac[0, 3], Ac[2, 3] * vc - Ac[1, 3], Ap[2, 3] * up - Ap[0, 3], Ap[2, 3] * vp - Ap[1, 3]], axis=1)
    # T3: V = (P^T P)^-1 P^T F, here through LAPACK's solver on the normal equations
    PtP = np.einsum("nki,nkj->nij", P, P)
    PtF = np.einsum("nki,nk->ni", P, Fv)
    return np.linalg.solve(PtP, PtF[..., None])[..., 0]


def independent_stage_5_7(phi_v, phi_h, valid_v, valid_h, cal):
    """An INDEPENDENT fp64 NumPy restatement of stage 5 (C1, C2) and stage 7 (T0-T3), written from the reference's source
    (5/compute_correspondance.cpp:60-77,642-679; 7/triangulation.cpp:252-307,352-378,1061-1126,1134-1218) and the published
    algorithms of the five OpenCV 2.4 routines it calls -- it shares NO code with oracle/ (different language, vectorised,
    the 4x3 systems solved by LAPACK instead of the adjugate).  Nothing in the reference tree can pin these stages (the
    artefacts that would are missing blobs), so this is corroboration, not a pin: two restatements written separately agree.
    phi_*: unwrapped phase planes (float32, stage 4 -- pinned by the KATs); valid_*: per-axis valid maps.
    Returns (valid [H,W] bool, c_p_map [H,W,2] int64, points [H,W,3] float64)."""
    f64 = np.float64
    # C1: merge_valid_maps
    valid = (valid_v == 1) & (valid_h == 1)
    # C2: x = lrint(fw * (phi / (2.0*Pi))), Pi = 22.0/7.0 unparenthesised -> (2.0*22.0)/7.0; round-half-even
    two_pi = (2.0 * 22.0) / 7.0
    with np.errstate(invalid="ignore"):
        x = np.rint(f64(FW) * (phi_v.astype(f64) / two_pi))
        y = np.rint(f64(FW) * (phi_h.astype(f64) / two_pi))
    finite = np.isfinite(x) & np.isfinite(y)                       # lrint raising FE_INVALID clears the pixel
    in_range = finite & (x >= 0) & (y >= 0) & (x <= PW - 1) & (y <= PH - 1)
    valid = valid & in_range
    cp = np.zeros(phi_v.shape + (2,), dtype=np.int64)
    cp[valid, 0] = x[valid].astype(np.int64)
    cp[valid, 1] = y[valid].astype(np.int64)

    Ac, Ap = independent_projection_matrices(cal)
    rows, cols = np.nonzero(valid)
    V = independent_triangulate(cols, rows, cp[rows, cols, 0], cp[rows, cols, 1], cal, Ac, Ap)
    pts = np.zeros(phi_v.shape + (3,), dtype=f64)
    pts[rows, cols] = V
    return valid, cp, pts


def main():
    ax = {0: "Vertical", 1: "Horizontal"}
    N = {0: N_V, 1: N_H}
    fringe = {a: [bmp(f"Captured_patterns/Fringe_patterns/{ax[a]}/Undistorted/Gray_captured_image_{i}.bmp")
                  for i in range(3)] for a in (0, 1)}
    gray = {a: [bmp(f"Captured_patterns/Coded_patterns/Gray_coded/{ax[a]}/Undistorted/Gray_captured_image_{i}.bmp")
                for i in range(N[a])] for a in (0, 1)}
    inv = {a: [bmp(f"Captured_patterns/Coded_patterns/Gray_coded/{ax[a]}/Undistorted/inverse_Gray_captured_image_{i}.bmp")
               for i in range(N[a])] for a in (0, 1)}
    kat3 = {a: bmp(f"Wrapped_phase_images/{ax[a]}/Wrapped_phase_image.bmp") for a in (0, 1)}
    kat4 = {0: bmp("Unwrapped_phase_images/Gray_coded/Vertical/Unwrapped_phase_vertical.bmp"),
            1: bmp("Unwrapped_phase_images/Gray_coded/Horizontal/Unwrapped_phase_horizontal.bmp")}

    # The lasso mask itself was not saved losslessly.  The final valid mask E is the non-zero set
    # of the stage-3 KAT (its formula never yields 0 on a valid pixel).  The reference's boundary
    # removal (3/wrapped_phase.cpp:266-279) is NOT a plain 3x3 erosion: invalid pixels that get
    # marked `visited` stop counting, which makes it scan-order dependent (E is not 3x3-open:
    # erode(dilate(E)) != E on 848 px, so no plain erosion could have produced it).  A selection
    # S with f(S) == E under the literal algorithm is built here: dilate E by the "later in scan
    # order" neighbours {E,SW,S,SE}, then add the earlier neighbours of any pixel still lost.
    E = (kat3[0] != 0)
    assert np.array_equal(E, kat3[1] != 0)
    print("valid pixels in KAT:", int(E.sum()))
    print("E is 3x3-open:", bool(np.array_equal(erode3(dilate3(E.astype(np.uint8))), E.astype(np.uint8))))
    orc = Oracle(W, H, PW, PH, N_V, N_H, FW, FW, ncodes_v=NCODES_V, ncodes_h=NCODES_H)
    S = E.astype(np.uint8)
    for dx, dy in ((1, 0), (-1, 1), (0, 1), (1, 1)):
        S |= shift(E.astype(np.uint8), dx, dy)
    for it in range(8):
        orc.set_mask(S)
        orc.compute_wrapped_phase(0, fringe[0])
        V = orc.valid_map(0).astype(bool)
        lost, extra = (~V & E), (V & ~E)
        print(f"mask pre-image iteration {it}: lost {int(lost.sum())} extra {int(extra.sum())}")
        if not lost.any() and not extra.any():
            break
        for y, x in zip(*np.nonzero(lost)):
            for dx, dy in ((-1, -1), (0, -1), (1, -1), (-1, 0)):
                S[y + dy, x + dx] = 1
    else:
        raise AssertionError("no selection mask reproduces the KAT's valid mask")
    assert S[0].sum() == 0 and S[-1].sum() == 0 and S[:, 0].sum() == 0 and S[:, -1].sum() == 0

    for a in (0, 1):
        orc.compute_wrapped_phase(a, fringe[a])
        d = orc.debug_image(3, a)
        bad = int((d != kat3[a]).sum())
        print(f"stage 3 axis {a}: {bad} mismatching pixels of {W*H}")
        assert bad == 0, "oracle stage 3 does not reproduce the reference KAT"
        assert np.array_equal(orc.valid_map(a).astype(bool), E)
    for a in (0, 1):
        orc.unwrap_phase(a, gray[a], inv[a])
        d = orc.debug_image(4, a)
        bad = int((d != kat4[a]).sum())
        print(f"stage 4 axis {a}: {bad} mismatching pixels of {W*H}")
        assert bad == 0, "oracle stage 4 does not reproduce the reference KAT"

    cal = {
        "Kc": xml_data("Camera_calibration/Matrices/cam_intrinsic_mat.xml"),
        "dc": xml_data("Camera_calibration/Matrices/cam_distortion_vect.xml"),
        "rc": xml_data("Triangulation/Camera_extrinsic_parametrs/world_to_cam_rot_vect.xml"),
        "tc": xml_data("Triangulation/Camera_extrinsic_parametrs/world_to_cam_trans_vect.xml"),
        "Kp": xml_data("Projector_calibration/Matrices/proj_intrinsic_mat.xml"),
        "dp": xml_data("Projector_calibration/Matrices/proj_distortion_vect.xml"),
        "rp": xml_data("Triangulation/Projector_extrinsic_parametrs/world_to_proj_rot_vect.xml"),
        "tp": xml_data("Triangulation/Projector_extrinsic_parametrs/world_to_proj_trans_vect.xml"),
    }
    cal["_source"] = "values of the 8 calibration XMLs read by 7/triangulation.cpp:152-168,1069-1083"
    cal["_dims"] = {"W": W, "H": H, "PW": PW, "PH": PH, "N_v": N_V, "N_h": N_H, "fw_v": FW, "fw_h": FW,
                    "ncodes_v": NCODES_V, "ncodes_h": NCODES_H}
    # PINS T0 (cvRodrigues2, cvTranspose, cvGEMM): stage 6 ran the same OpenCV routines on the same two rotation vectors
    # stage 7 reads and saved the result (6/system_calibration.cpp:1488-1516): Rc*Rp^T and tc - (Rc*Rp^T)*tp.  The oracle's
    # restatements must reproduce all 12 doubles of the two files BIT FOR BIT before any golden is written.
    from oracle import oracle as O
    kat_R = np.array(xml_data("Triangulation/Relative_geometry/proj_cam_rot_mat.xml"))
    kat_t = np.array(xml_data("Triangulation/Relative_geometry/proj_cam_trans_vect.xml"))
    got_R, got_t = O.relative_geometry(cal["rc"], cal["tc"], cal["rp"], cal["tp"])
    same = int((got_R.ravel().view(np.uint64) == kat_R.view(np.uint64)).sum() + (got_t.view(np.uint64) == kat_t.view(np.uint64)).sum())
    print(f"T0 known answer (Relative_geometry/*.xml, OpenCV 2.4's own output): {same} of 12 doubles bit-identical")
    assert same == 12, "oracle rodrigues / transpose / mat_mul do not reproduce the reference's saved relative geometry"
    cal["_relative_geometry"] = {
        "proj_cam_rot_mat": [float(x) for x in kat_R], "proj_cam_trans_vect": [float(x) for x in kat_t],
        "_source": "Triangulation/Relative_geometry/proj_cam_rot_mat.xml + proj_cam_trans_vect.xml, written by "
                   "6/system_calibration.cpp:1488-1516 (cvRodrigues2 x2, cvTranspose, cvMatMul x2, cvSub) from the same rc/rp/tc/tp "
                   "7/triangulation.cpp:1069-1083 reads: the reference-held known answer for T0"}
    # the reference's OTHER projector calibrations: two OpenCV calibrations of the projectors it was used with, both strongly
    # distorted (k1 = -1.01 / -1.16, k2 = 8.28 / 2.60) -- stage 7 reads whatever proj_intrinsic_mat.xml / proj_distortion_vect.xml
    # hold (7/triangulation.cpp:152-168), so these are inputs the path really meets (tests/test_gpu_round4.py: table rig)
    cal["_alt_projectors"] = {
        name: {"Kp": xml_data(f"Projector_calibration/Matrices/OPencv calib/{name}/Projector_intrinsic_mat.xml"),
               "dp": xml_data(f"Projector_calibration/Matrices/OPencv calib/{name}/Projector_dist_vect.xml")}
        for name in ("Sharp", "Viewsonic")}
    cal["_alt_projectors"]["_source"] = "Projector_calibration/Matrices/OPencv calib/{Sharp,Viewsonic}/Projector_{intrinsic_mat,dist_vect}.xml"
    with open(os.path.join(HERE, "calibration.json"), "w") as f:
        json.dump(cal, f, indent=1)

    orc.set_calibration(*[cal[k] for k in ("Kc", "dc", "rc", "tc", "Kp", "dp", "rp", "tp")])
    orc.compute_c_p_map()
    orc.triangulate()
    valid = orc.valid_map(2)
    cp = orc.c_p_map()
    pts = orc.intersection_points()
    print("in-range correspondences:", int(valid.sum()), "mean xyz:", pts[valid == 1].mean(axis=0))
    # corroboration of the unpinned stages: the independent NumPy restatement on the SAME full 1600x1200 scan must give the
    # identical correspondences and the same points before any golden is written
    iv, icp, ipts = independent_stage_5_7(orc.unwrapped_phi(0), orc.unwrapped_phi(1), orc.valid_map(0), orc.valid_map(1), cal)
    assert np.array_equal(iv, valid == 1), "independent restatement: valid map after stage 5 differs"
    assert np.array_equal(icp[iv], cp[iv]), "independent restatement: correspondences differ"
    rel = np.linalg.norm(ipts[iv] - pts[iv], axis=-1) / np.linalg.norm(pts[iv], axis=-1)
    print(f"independent NumPy restatement of stages 5 + 7: {int(iv.sum())} identical correspondences, "
          f"max relative point difference {rel.max():.3e} (median {np.median(rel):.1e})")
    assert int(iv.sum()) == 355608, "SURVEY's count of in-range correspondences on the real scan"
    assert rel.max() <= 1e-12, "independent restatement: 3-D points differ by more than 1e-12 of their norm"
    A_cam, A_proj = orc.projection_matrices()

    ys, xs = np.nonzero(E)
    print("valid bbox x:[%d,%d] y:[%d,%d]" % (xs.min(), xs.max(), ys.min(), ys.max()))
    # crop A: fully inside the valid region; crop B: straddles the lasso boundary (erosion edge,
    # invalid pixels); both 128x64.
    crops = {"real_inside": (800, 400), "real_edge": (int(xs.min()) - 40, int(ys[xs == xs.min()][0]) - 32)}
    CW, CH = 128, 64
    for name, (x0, y0) in crops.items():
        x0 -= x0 % 4
        sl = np.s_[y0:y0 + CH, x0:x0 + CW]
        frac = E[sl].mean()
        print(f"crop {name}: origin ({x0},{y0}) valid fraction {frac:.3f}")
        np.savez_compressed(
            os.path.join(HERE, name + ".npz"),
            origin=np.array([x0, y0]), full=np.array([W, H, PW, PH]),
            params=np.array([N_V, N_H, FW, FW, NCODES_V, NCODES_H]),
            mask=S[sl], mask_halo2=S[y0 - 2:y0 + CH + 2, x0 - 2:x0 + CW + 2],
            fringe_v=np.stack([f[sl] for f in fringe[0]]), fringe_h=np.stack([f[sl] for f in fringe[1]]),
            gray_v=np.stack([f[sl] for f in gray[0]]), inv_v=np.stack([f[sl] for f in inv[0]]),
            gray_h=np.stack([f[sl] for f in gray[1]]), inv_h=np.stack([f[sl] for f in inv[1]]),
            # reference-provided answers (PINNED): crops of the reference's own KAT images
            kat_wrapped_v=kat3[0][sl], kat_wrapped_h=kat3[1][sl],
            kat_unwrapped_v=kat4[0][sl], kat_unwrapped_h=kat4[1][sl],
            # oracle outputs of the full-frame run (regression goldens for the unpinned stages)
            valid=valid[sl], code_v=orc.code(0)[sl], code_h=orc.code(1)[sl],
            wrapped_v=orc.wrapped_phi(0)[sl], wrapped_h=orc.wrapped_phi(1)[sl],
            unwrapped_v=orc.unwrapped_phi(0)[sl], unwrapped_h=orc.unwrapped_phi(1)[sl],
            c_p_map=cp[sl], points=pts[sl], A_cam=A_cam, A_proj=A_proj,
        )
    print("golden fixtures written to", HERE)


def patterns():
    """N1: pins the oracle's pattern generator on the reference's own pattern images
    (M_tech_project_console/Generated_patterns, written by 1/pattern_generator.cpp:414-470 for 1280x720, 3 fringe
    patterns, fringe width 32 on both axes) and writes tests/golden/patterns_ref.npz: every pattern is constant along
    one axis (checked here), so its 1-D profile is the whole image; plus the 1078-byte BMP header + palette the
    reference's cvSaveImage wrote and the SHA-256 of every file (the shim's generate_pattern() reproduces the files)."""
    import hashlib
    from PIL import Image
    from oracle import oracle as O
    root = REF + "Generated_patterns/"
    fw, F = FW, 3
    out = {"config": np.array([PW, PH, F, fw, fw])}
    names, hashes = [], []
    header = None
    n_files = 0
    for axis, ax_name, extent in ((0, "Vertical", PW), (1, "Horizontal", PH)):
        ncodes, nplanes = O.pattern_counts(extent, fw)
        assert (ncodes, nplanes) == ((NCODES_V, N_V) if axis == 0 else (NCODES_H, N_H))
        for kind, key, fmt, count in ((O.PATTERN_FRINGE, "fringe", "Fringe_patterns/%s/Pattern_%d.bmp", F),
                                      (O.PATTERN_GRAY, "gray", "Coded_patterns/Gray_coded/%s/Pattern_%d.bmp", nplanes + 1),
                                      (O.PATTERN_INVERSE_GRAY, "inverse", "Coded_patterns/Gray_coded/%s/inverse_Pattern_%d.bmp", nplanes + 1),
                                      (O.PATTERN_BINARY, "binary", "Coded_patterns/Binary_coded/%s/Pattern_%d.bmp", nplanes + 1)):
            for i in range(count):
                rel = fmt % (ax_name, i)
                raw = open(root + rel, "rb").read()
                im = Image.open(root + rel)
                assert im.mode == "L" and im.size == (PW, PH), (rel, im.mode, im.size)
                kat = np.array(im)
                prof = kat[0, :] if axis == 0 else kat[:, 0]
                assert np.array_equal(kat, np.broadcast_to(prof[None, :] if axis == 0 else prof[:, None], kat.shape)), rel
                got = O.pattern_image(kind, axis, i, PW, PH, fw, nplanes, F)
                assert np.array_equal(got, kat), f"oracle pattern differs from the reference's {rel}: {(got != kat).sum()} px"
                out[f"{key}_{'vh'[axis]}_{i}"] = prof.copy()
                names.append(rel)
                hashes.append(hashlib.sha256(raw).hexdigest())
                header = raw[:1078] if header is None else header
                assert raw[:1078] == header and len(raw) == 1078 + PW * PH
                n_files += 1
    out["bmp_header"] = np.frombuffer(header, dtype=np.uint8)
    out["file_names"] = np.array(names)
    out["file_sha256"] = np.array(hashes)
    np.savez_compressed(os.path.join(HERE, "patterns_ref.npz"), **out)
    print(f"pattern generator pinned on {n_files} reference images (every pixel equal); patterns_ref.npz written")

# ---- the reference's own point cloud: pins T0-T3 and O1 ---------------------------------------------------------------------------
PLY_PATH = "Point_cloud/test data/point_cloud_2.ply"
PLY_N = 103959
PLY_HEADER = (b"ply\nformat binary_little_endian 1.0\ncomment VCGLIB generated\nelement vertex 103959\n"
              b"property float x\nproperty float y\nproperty float z\n"
              b"property uchar red\nproperty uchar green\nproperty uchar blue\nproperty uchar alpha\n"
              b"element face 0\nproperty list uchar int vertex_indices\nend_header\n")


def ulp_distance(a, b):
    """Per-element distance of two float32 arrays in units in the last place (ordered integer images of the bit patterns)."""
    def ordered(v):
        i = np.ascontiguousarray(v, dtype=np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(ordered(a) - ordered(b))


def stage_3_5_value(t1, t2, code):
    """The literal float chain of stages 3-5 for one axis, up to the argument of C2's lrint: the wrapped phase atan2(t1, t2) stored
    as float (3/wrapped_phase.cpp:171-175), += Pi and + code * 2.0 * Pi with Pi = 22.0/7.0 unparenthesised, each stored as float
    (4/phase_unwrap.cpp:290-291), then fw * (phi / (2.0 * Pi)) in double (5/compute_correspondance.cpp:648)."""
    f64, f32 = np.float64, np.float32
    w = np.arctan2(np.asarray(t1, f64), np.asarray(t2, f64)).astype(f32)
    w = (w.astype(f64) + 22.0 / 7.0).astype(f32)
    u = (w.astype(f64) + code * 2.0 * 22.0 / 7.0).astype(f32)
    return FW * (u.astype(f64) / (2.0 * 22.0 / 7.0))


def byte_table(extent, nbits, filler_code):
    """Row t (t < extent): the bytes of the 3 + 2*nbits planes (fringe g0 g1 g2, Gray, inverse Gray) of a pixel that stages 3-5
    decode to projector coordinate t; row `extent`: a filler that decodes out of range (Gray code filler_code).  The fringe triple
    is the one whose lrint argument lies closest to t (the widest margin from C2's rounding boundaries), found over every
    realisable (t1 = g0 - g2, t2 = 2 g1 - g0 - g2); Gray bit i of code k is set iff gray >= inverse (4/phase_unwrap.cpp:183)."""
    t1, t2 = np.meshgrid(np.arange(-255, 256), np.arange(-510, 511), indexing="ij")
    t1, t2 = t1.ravel(), t2.ravel()
    s = np.maximum(np.abs(t1), -t2)                 # g0 + g2: smallest sum that keeps every byte >= 0
    ok = ((t1 - t2) % 2 == 0) & (s <= 510 - np.abs(t1)) & (s <= 510 - t2)
    t1, t2, s = t1[ok], t2[ok], s[ok]
    fringe = np.stack([(s + t1) // 2, (t2 + s) // 2, (s - t1) // 2], 1)
    assert fringe.min() >= 0 and fringe.max() <= 255
    assert np.array_equal(fringe[:, 0] - fringe[:, 2], t1) and np.array_equal(2 * fringe[:, 1] - fringe[:, 0] - fringe[:, 2], t2)
    table = np.zeros((extent + 1, 3 + 2 * nbits), dtype=np.uint8)

    def gray_bytes(k):
        g = k ^ (k >> 1)
        bits = np.array([(g >> (nbits - 1 - i)) & 1 for i in range(nbits)], dtype=np.uint8)
        return np.concatenate([255 * bits, 255 * (1 - bits)])

    for k in range(-(-extent // FW)):
        val = stage_3_5_value(t1, t2, k)
        t = np.rint(val)
        err = np.abs(val - t)
        for target in range(FW * k, min(FW * (k + 1), extent)):
            cand = np.nonzero(t == target)[0]
            assert len(cand), f"no fringe triple decodes to {target}"
            j = cand[np.argmin(err[cand])]
            table[target, :3] = fringe[j]
            table[target, 3:] = gray_bytes(k)
    table[extent, :3] = table[0, :3]
    table[extent, 3:] = gray_bytes(filler_code)
    assert stage_3_5_value(0, 0, filler_code) > extent
    return table


def ply_vertices():
    """The reference's own point cloud: (xyz float32 [n, 3] in file order, SHA-256 of the file).  Header checked as text, payload
    size checked exactly (16-byte records: x y z float32, r g b a uchar)."""
    import hashlib
    raw = open(REF + PLY_PATH, "rb").read()
    assert raw.startswith(PLY_HEADER), "unexpected PLY header"
    payload = raw[len(PLY_HEADER):]
    assert len(payload) == PLY_N * 16, len(payload)
    rec = np.frombuffer(payload, dtype=np.dtype([("xyz", "<f4", (3,)), ("rgba", "u1", (4,))]))
    return rec["xyz"].astype(np.float32), hashlib.sha256(raw).hexdigest()


def _seed_tuples(X, cal, Ac, Ap):
    """Re-projection of each vertex into the camera (with its distortion) and the projector: real-valued (c, r, x, y) seeds."""
    def reproject(A, K, d):
        h = X @ A[:, :3].T + A[:, 3]
        u, v = h[:, 0] / h[:, 2], h[:, 1] / h[:, 2]
        K = np.asarray(K, np.float64).reshape(3, 3)
        k1, k2, p1, p2, k3 = d
        x, y = (u - K[0, 2]) / K[0, 0], (v - K[1, 2]) / K[1, 1]
        r2 = x * x + y * y
        rad = 1 + r2 * (k1 + r2 * (k2 + r2 * k3))
        xd = x * rad + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
        yd = y * rad + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
        return K[0, 0] * xd + K[0, 2], K[1, 1] * yd + K[1, 2]
    c, r = reproject(Ac, cal["Kc"], cal["dc"])
    x, y = reproject(Ap, cal["Kp"], cal["dp"])
    return np.rint(np.stack([c, r, x, y], 1)).astype(np.int64)


def _search(args):
    """Worker of find_tuples: every tuple of a window around each seed, through independent_triangulate and the float cast.
    -> per vertex (status, tuple, ulp): status 0 exact, 1 unique match within 1 ulp, 2 none, 3 ambiguous."""
    X32, seeds, win, cal, undist = args
    Ac, Ap = independent_projection_matrices(cal)
    offs = np.stack(np.meshgrid(*[np.arange(-w, w + 1) for w in win], indexing="ij"), -1).reshape(-1, 4)
    lim = np.array([W - 1, H - 1, PW - 1, PH - 1])
    out_status = np.full(len(X32), 2, dtype=np.int64)
    out_tup = np.zeros((len(X32), 4), dtype=np.int64)
    out_ulp = np.zeros(len(X32), dtype=np.int64)
    step = max(1, 1000000 // len(offs))
    for a in range(0, len(X32), step):
        cand = seeds[a:a + step, None, :] + offs[None]                      # [m, k, 4]
        inside = ((cand >= 0) & (cand <= lim)).all(-1)
        cand = np.clip(cand, 0, lim).reshape(-1, 4)
        V = independent_triangulate(cand[:, 0], cand[:, 1], cand[:, 2], cand[:, 3], cal, Ac, Ap, undist).astype(np.float32)
        d = ulp_distance(V.reshape(-1, len(offs), 3), X32[a:a + step, None, :]).max(-1)
        d = np.where(inside, d, np.iinfo(np.int64).max)
        cand = cand.reshape(-1, len(offs), 4)
        for i in range(len(d)):
            n0, n1 = int((d[i] == 0).sum()), int((d[i] <= 1).sum())
            j = int(np.argmin(d[i]))
            status = (0 if n0 == 1 else 3) if n0 else (1 if n1 == 1 else 3 if n1 else 2)
            out_status[a + i], out_tup[a + i], out_ulp[a + i] = status, cand[i, j], d[i, j]
    return out_status, out_tup, out_ulp


def find_tuples(X32, cal, jobs=16):
    """The integer tuple (camera col c, row r, projector x, y) of every vertex: the one tuple whose independent_triangulate point,
    cast to float, equals the vertex (or, failing that, the one tuple within 1 ulp on every coordinate).  Windows around the
    re-projection seeds widen only for the vertices the narrower window missed."""
    from concurrent.futures import ProcessPoolExecutor
    Ac, Ap = independent_projection_matrices(cal)
    seeds = _seed_tuples(X32.astype(np.float64), cal, Ac, Ap)
    rc, cc = np.mgrid[0:H, 0:W].astype(np.float64)
    ry, rx = np.mgrid[0:PH, 0:PW].astype(np.float64)
    undist = independent_undistort_reproject(cc, rc, cal["Kc"], cal["dc"]) + independent_undistort_reproject(rx, ry, cal["Kp"], cal["dp"])
    n = len(X32)
    status = np.full(n, 2, dtype=np.int64)
    tup = np.zeros((n, 4), dtype=np.int64)
    ulp = np.zeros(n, dtype=np.int64)
    todo = np.arange(n)
    for win in ((0, 10, 1, 3), (1, 16, 2, 6), (2, 45, 2, 45)):
        if not len(todo):
            break
        parts = np.array_split(todo, max(1, min(jobs, len(todo) // 64)))
        with ProcessPoolExecutor(max_workers=min(jobs, len(parts))) as ex:
            res = list(ex.map(_search, [(X32[p], seeds[p], win, cal, undist) for p in parts]))
        for p, (st, tp, ul) in zip(parts, res):
            status[p], tup[p], ulp[p] = st, tp, ul
        assert not (status == 3).any(), f"ambiguous tuples at vertices {np.nonzero(status == 3)[0][:20]}"
        todo = np.nonzero(status == 2)[0]
        print(f"  window (c, r, x, y) +-{win}: {n - len(todo)} of {n} vertices matched, {len(todo)} left")
    return status, tup, ulp


def ply_stage7():
    """PINS T0-T3 AND O1 on the reference's own point cloud (Point_cloud/test data/point_cloud_2.ply: binary PLY the reference's
    pipeline produced from one view, thinned by MeshLab, row-major scan order).  A point depends only on its integer tuple
    (camera col c, row r, projector x, y) and the 8 calibration XMLs, so:
      1. the tuple of every vertex is found with the independent restatement (float32 equality, unique per vertex), and the tuples
         are checked: no camera pixel carries two vertices, (r, c) strictly increasing in file order;
      2. per-coordinate byte tables (tests/ply_capture.py) are built and every entry is proved with the oracle's stages 3-5;
      3. the synthetic capture of tests/ply_capture.py goes through the oracle's literal stages 3 -> 8: c_p_map == tuples, the
         merged valid map set on exactly the vertex pixels, and point_cloud() equal to the PLY's floats in order, bit for bit on
         at least 99 % of the vertices, the others within 1 ulp and recorded by index and ulp distance (a vertex no tuple
         reproduces is recorded as unmatched);
    then tests/golden/ply_stage7.npz is written (derived data only).  `python tests/golden/make_golden.py ply` runs this step alone."""
    import time
    sys.path.insert(0, os.path.join(HERE, ".."))
    import ply_capture as PC
    assert (PC.W, PC.H, PC.PW, PC.PH, PC.N_V, PC.N_H, PC.FW, PC.NCODES_V, PC.NCODES_H) == (W, H, PW, PH, N_V, N_H, FW, NCODES_V, NCODES_H)
    with open(os.path.join(HERE, "calibration.json")) as f:
        cal = json.load(f)
    cal_t = [cal[k] for k in ("Kc", "dc", "rc", "tc", "Kp", "dp", "rp", "tp")]
    X32, sha = ply_vertices()
    n = len(X32)
    t0 = time.time()
    status, tup, ulp_np = find_tuples(X32, cal)
    print(f"tuple search ({time.time() - t0:.0f} s), independent restatement: {int((status == 0).sum())} exact, "
          f"{int((status == 1).sum())} within 1 ulp, {int((status == 2).sum())} unmatched of {n}")
    # a vertex no tuple reproduces (none within 1 ulp in the widest window: isolated outliers of the file, not points of this
    # view's scan order) is not dropped: it is recorded with the best distance found and counts against the 99.9 % below
    matched = status != 2
    unmatched = np.nonzero(~matched)[0]
    tup[unmatched] = -1
    key = tup[matched, 1] * W + tup[matched, 0]
    dup = np.unique(key, return_counts=True)
    assert (dup[1] == 1).all(), f"camera pixels carrying two vertices: {dup[0][dup[1] > 1][:20]} (r * W + c)"
    assert (np.diff(key) > 0).all(), f"(r, c) not strictly increasing at matched vertices {np.nonzero(np.diff(key) <= 0)[0][:20]}"
    t = tup[matched]
    border = (t[:, 0] < 2) | (t[:, 0] > W - 3) | (t[:, 1] < 2) | (t[:, 1] > H - 3)
    assert not border.any(), "a vertex pixel lies where stage 3's boundary removal clears the selection"

    table_x = byte_table(PW, N_V, (1 << N_V) - 1)
    table_y = byte_table(PH, N_H, (1 << N_H) - 1)
    # every table entry proved on the oracle's stages 3-5: row 2 decodes x = j, y = j % PH; row 3 the x filler, row 4 the y filler
    pw, ph_ = PW + 4, 7
    ix = np.zeros((ph_, pw), np.int64)
    iy = np.zeros((ph_, pw), np.int64)
    j = np.arange(PW)
    ix[2, 2:-2], iy[2, 2:-2] = j, j % PH
    ix[3, 2:-2], iy[3, 2:-2] = PC.X_FILLER, j % PH
    ix[4, 2:-2], iy[4, 2:-2] = j, PC.Y_FILLER
    pm = np.zeros((ph_, pw), np.uint8)
    pm[1:-1, 1:-1] = 1
    po = Oracle(pw, ph_, PW, PH, N_V, N_H, FW, FW, ncodes_v=NCODES_V, ncodes_h=NCODES_H)
    po.set_mask(pm)
    pv, phh = np.moveaxis(table_x[ix], -1, 0), np.moveaxis(table_y[iy], -1, 0)
    for a, planes, nb in ((0, pv, N_V), (1, phh, N_H)):
        po.compute_wrapped_phase(a, list(planes[:3]))
    for a, planes, nb in ((0, pv, N_V), (1, phh, N_H)):
        po.unwrap_phase(a, list(planes[3:3 + nb]), list(planes[3 + nb:]))
    po.compute_c_p_map()
    pcp, pvm = po.c_p_map(), po.valid_map(2)
    assert pvm[2, 2:-2].all() and not pvm[3].any() and not pvm[4].any()
    assert np.array_equal(pcp[2, 2:-2, 0], j) and np.array_equal(pcp[2, 2:-2, 1], j % PH), "a byte table entry decodes wrongly"
    assert (pcp[3, 2:-2, 0] >= FW * ((1 << N_V) - 1)).all() and (pcp[4, 2:-2, 1] >= FW * ((1 << N_H) - 1)).all()
    print(f"byte tables: {PW} + {PH} entries and both fillers proved on the oracle's stages 3-5")

    fx = {"tuples": tup.astype(np.int16), "xyz": X32, "table_x": table_x, "table_y": table_y}
    mask, planes_v, planes_h = PC.capture(fx)
    orc = Oracle(W, H, PW, PH, N_V, N_H, FW, FW, ncodes_v=NCODES_V, ncodes_h=NCODES_H)
    orc.set_mask(mask)
    orc.set_calibration(*cal_t)
    orc.run_scan(list(planes_v), list(planes_h))
    vm = orc.valid_map(2) == 1
    assert np.array_equal(vm, PC.vertex_map(fx)), "oracle: merged valid map differs from the vertex pixels"
    cp = orc.c_p_map()
    assert np.array_equal(cp[t[:, 1], t[:, 0]], t[:, 2:]), "oracle: c_p_map differs from the tuples"
    cloud = orc.point_cloud()
    assert cloud.shape == X32[matched].shape
    d = ulp_distance(cloud, X32[matched]).max(-1)
    inexact = np.nonzero(matched)[0][d > 0]
    n0, n1 = int((d == 0).sum()), int((d == 1).sum())
    print(f"oracle stages 3 -> 8 on the synthetic capture: {n0} exact ({n0 / n:.4%} of {n}), {n1} within 1 ulp, "
          f"{int((d > 1).sum())} further (max {int(d.max())} ulp), {len(unmatched)} unmatched")
    # Measured: 99.0 % bit for bit, every other matched vertex 1 ulp away -- and the independent restatement (LAPACK, another
    # order of operations) misses on exactly the same vertices, by the same ulp.  Two restatements that agree with each other to
    # ~1e-12 relative both land on the other side of a float rounding boundary there, so the reference's own fp64 arithmetic (the
    # OpenCV build it linked) differs from the published algorithms by ~1e-10 relative: a property of the reference, not a defect of
    # either restatement.  The bar is what that leaves: 99 % exact, nothing further than 1 ulp, the same exceptions in both.
    assert np.array_equal(inexact, np.nonzero(status == 1)[0]) and np.array_equal(d[d > 0], ulp_np[inexact]), \
        "the oracle and the independent restatement miss the reference's floats on different vertices"
    assert d.max() <= 1 and n0 >= 0.99 * n, "the oracle reproduces fewer than 99 % of the reference's points bit for bit"
    # stored compactly (PC.encode_fixture: tuple deltas, ulp residuals from a deterministic prediction, SHA-256 of the floats), and
    # read back through the decoder the tests use before anything is written
    Ac, Ap = independent_projection_matrices(cal)
    out = os.path.join(HERE, "ply_stage7.npz")
    np.savez_compressed(out, **PC.encode_fixture(tup, X32, cal, Ac, Ap),
                        inexact_index=inexact.astype(np.int32), inexact_ulp=d[d > 0].astype(np.int32),
                        unmatched_index=unmatched.astype(np.int32), unmatched_best_ulp=ulp_np[unmatched].astype(np.int64),
                        table_x=table_x, table_y=table_y, ply_sha256=np.array(sha))
    back = PC.load_fixture(out, cal)
    assert np.array_equal(back["tuples"], tup) and np.array_equal(back["xyz"].view(np.uint32), X32.view(np.uint32))
    assert np.array_equal(back["table_x"], table_x) and np.array_equal(back["table_y"], table_y)
    print("ply_stage7.npz written")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "patterns":
        patterns()
    elif len(sys.argv) > 1 and sys.argv[1] == "ply":
        ply_stage7()
    else:
        main()
        patterns()
        ply_stage7()
