"""PLY output of clouds and meshes (pure NumPy; no GPU, no library call).

The reference's stage 8 writes an ASCII PLY of coloured points (8/save_point_cloud.cpp:56-104) and its user meshed that file by hand;
write_ply stores what Scanner.mesh / Scanner.cloud_rgb return -- vertices in the cloud's order, faces as indices into it -- in the
standard layout every mesh tool reads."""
import numpy as np


def write_ply(path, xyz, faces=None, rgb=None, binary=True, normals=None):
    """Standard PLY: `element vertex` with float x y z (+ float nx ny nz directly after them when normals is given: (n, 3) float32, what
    Scanner.mesh_normals returns; + uchar red green blue when rgb is given: (n, 3) uint8; both in the order of xyz) and,
    when faces is given ((m, 3) integer indices into xyz), `element face` with `property list uchar int vertex_indices`.
    binary: binary_little_endian 1.0, else ascii 1.0 (floats written with 9 significant digits: they read back exactly)."""
    v = np.ascontiguousarray(xyz, dtype=np.float32)
    if v.ndim != 2 or v.shape[1] != 3:
        raise ValueError(f"xyz must have shape (n, 3), not {v.shape}")
    n = v.shape[0]
    nrm = None
    if normals is not None:
        nrm = np.asarray(normals)
        if nrm.shape != (n, 3) or nrm.dtype != np.float32:
            raise ValueError(f"normals must be float32 of shape ({n}, 3), not {nrm.dtype} {nrm.shape}")
    c = None
    if rgb is not None:
        c = np.asarray(rgb)
        if c.shape != (n, 3) or c.dtype != np.uint8:
            raise ValueError(f"rgb must be uint8 of shape ({n}, 3), not {c.dtype} {c.shape}")
    f = None
    if faces is not None:
        f = np.asarray(faces)
        if f.ndim != 2 or f.shape[1] != 3 or not np.issubdtype(f.dtype, np.integer):
            raise ValueError(f"faces must be integers of shape (m, 3), not {f.dtype} {f.shape}")
        if f.size and (int(f.min()) < 0 or int(f.max()) >= n):
            raise ValueError(f"face index out of range [0, {n})")
        f = f.astype("<i4")
    head = ["ply", "format binary_little_endian 1.0" if binary else "format ascii 1.0", f"element vertex {n}",
            "property float x", "property float y", "property float z"]
    if nrm is not None:
        head += ["property float nx", "property float ny", "property float nz"]
    if c is not None:
        head += ["property uchar red", "property uchar green", "property uchar blue"]
    if f is not None:
        head += [f"element face {f.shape[0]}", "property list uchar int vertex_indices"]
    head.append("end_header")
    with open(path, "wb") as out:
        out.write(("\n".join(head) + "\n").encode("ascii"))
        if binary:
            if c is None and nrm is None:
                out.write(v.astype("<f4").tobytes())
            else:
                rec = np.empty(n, dtype=[("p", "<f4", 3)] + ([("n", "<f4", 3)] if nrm is not None else []) + ([("c", "u1", 3)] if c is not None else []))
                rec["p"] = v
                if nrm is not None:
                    rec["n"] = nrm
                if c is not None:
                    rec["c"] = c
                out.write(rec.tobytes())
            if f is not None:
                rec = np.empty(f.shape[0], dtype=[("n", "u1"), ("i", "<i4", 3)])
                rec["n"], rec["i"] = 3, f
                out.write(rec.tobytes())
        else:
            lines = []
            for k in range(n):
                t = " ".join(f"{float(x):.9g}" for x in (v[k] if nrm is None else np.concatenate([v[k], nrm[k]])))
                lines.append(t if c is None else f"{t} {c[k, 0]} {c[k, 1]} {c[k, 2]}")
            if f is not None:
                lines += [f"3 {a} {b} {d}" for a, b, d in f.tolist()]
            if lines:
                out.write(("\n".join(lines) + "\n").encode("ascii"))
