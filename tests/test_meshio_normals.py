"""CPU test of write_ply(..., normals=) (3dscan_amd/meshio.py): nx ny nz directly after x y z and before the colours, in binary and
ASCII, read back by a parser written here from the PLY format; a file written without normals is byte for byte what write_ply wrote
before it knew the argument."""
import numpy as np
import pytest

from conftest import pkg

XYZ = [("float", "x"), ("float", "y"), ("float", "z")]
NRM = [("float", "nx"), ("float", "ny"), ("float", "nz")]
RGB = [("uchar", "red"), ("uchar", "green"), ("uchar", "blue")]


def read_ply(path):
    """-> (format, xyz float32 (n,3), normals float32 (n,3) or None, rgb uint8 (n,3) or None, faces int32 (m,3) or None, header lines)"""
    raw = open(path, "rb").read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    head = raw[:end].decode("ascii").splitlines()
    body = raw[end:]
    assert head[0] == "ply" and head[-1] == "end_header"
    fmt = head[1].split()
    assert fmt[0] == "format" and fmt[2] == "1.0"
    elements, cur = [], None
    for line in head[2:-1]:
        t = line.split()
        if t[0] == "element":
            cur = (t[1], int(t[2]), [])
            elements.append(cur)
        else:
            assert t[0] == "property" and cur is not None
            cur[2].append(tuple(t[1:]))
    assert elements[0][0] == "vertex"
    n, vprops = elements[0][1], elements[0][2]
    assert vprops[:3] == XYZ
    has_n = vprops[3:6] == NRM
    has_rgb = vprops[3 + 3 * has_n:] == RGB
    assert vprops == XYZ + (NRM if has_n else []) + (RGB if has_rgb else [])          # this order and nothing else
    m = None
    if len(elements) > 1:
        assert len(elements) == 2 and elements[1][0] == "face" and elements[1][2] == [("list", "uchar", "int", "vertex_indices")]
        m = elements[1][1]
    nf = 3 + 3 * has_n
    if fmt[1] == "ascii":
        lines = body.decode("ascii").splitlines()
        assert len(lines) == n + (m or 0)
        vt = [l.split() for l in lines[:n]]
        assert all(len(t) == nf + 3 * has_rgb for t in vt)
        flt = np.array([[np.float32(x) for x in t[:nf]] for t in vt], dtype=np.float32).reshape(n, nf)
        rgb = np.array([[int(x) for x in t[nf:]] for t in vt], dtype=np.uint8).reshape(n, 3) if has_rgb else None
        faces = None
        if m is not None:
            ft = [[int(x) for x in l.split()] for l in lines[n:]]
            assert all(len(t) == 4 and t[0] == 3 for t in ft)
            faces = np.array([t[1:] for t in ft], dtype=np.int32).reshape(m, 3)
    else:
        assert fmt[1] == "binary_little_endian"
        vdt = np.dtype([("f", "<f4", nf)] + ([("c", "u1", 3)] if has_rgb else []))
        assert vdt.itemsize == 4 * nf + 3 * has_rgb
        v = np.frombuffer(body, dtype=vdt, count=n)
        flt, rgb = v["f"].copy().reshape(n, nf), (v["c"].copy() if has_rgb else None)
        rest = body[n * vdt.itemsize:]
        faces = None
        if m is not None:
            fdt = np.dtype([("n", "u1"), ("i", "<i4", 3)])
            assert len(rest) == 13 * m
            f = np.frombuffer(rest, dtype=fdt, count=m)
            assert (f["n"] == 3).all()
            faces = f["i"].astype(np.int32)
        else:
            assert len(rest) == 0
    return fmt[1], np.ascontiguousarray(flt[:, :3]), (np.ascontiguousarray(flt[:, 3:]) if has_n else None), rgb, faces, head


def _mesh(rng, n, m):
    xyz = (rng.normal(0, 300, size=(n, 3)) * 10.0 ** rng.integers(-6, 3, size=(n, 1))).astype(np.float32)
    nrm = rng.normal(0, 1, size=(n, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
    nrm[::7] = 0.0                                                       # the zero normal of a vertex in no face
    rgb = rng.integers(0, 256, size=(n, 3)).astype(np.uint8)
    faces = rng.integers(0, max(n, 1), size=(m, 3)).astype(np.int32)
    return xyz, nrm, rgb, faces


@pytest.mark.parametrize("binary", [True, False])
def test_header_order(tmp_path, binary):
    io = pkg("meshio")
    xyz, nrm, rgb, faces = _mesh(np.random.default_rng(2), 5, 3)
    path = str(tmp_path / "h.ply")
    io.write_ply(path, xyz, faces=faces, rgb=rgb, binary=binary, normals=nrm)
    head = read_ply(path)[5]
    assert head == ["ply", "format binary_little_endian 1.0" if binary else "format ascii 1.0", "element vertex 5",
                    "property float x", "property float y", "property float z", "property float nx", "property float ny", "property float nz",
                    "property uchar red", "property uchar green", "property uchar blue",
                    "element face 3", "property list uchar int vertex_indices", "end_header"]


@pytest.mark.parametrize("binary", [True, False])
@pytest.mark.parametrize("with_faces", [True, False])
@pytest.mark.parametrize("with_rgb", [True, False])
def test_write_ply_with_normals_reads_back(tmp_path, binary, with_faces, with_rgb):
    io = pkg("meshio")
    rng = np.random.default_rng(5)
    for n, m in ((257, 411), (1, 0), (0, 0)):
        xyz, nrm, rgb, faces = _mesh(rng, n, m)
        path = str(tmp_path / "m.ply")
        io.write_ply(path, xyz, faces=faces if with_faces else None, rgb=rgb if with_rgb else None, binary=binary, normals=nrm)
        fmt, gx, gn, gc, gf, head = read_ply(path)
        assert fmt == ("binary_little_endian" if binary else "ascii") and f"element vertex {n}" in head
        assert gx.shape == (n, 3) and np.array_equal(gx.view(np.uint32), xyz.view(np.uint32))     # every float exactly
        assert gn is not None and gn.shape == (n, 3) and np.array_equal(gn.view(np.uint32), nrm.view(np.uint32))
        assert (gc is not None) == with_rgb and (gf is not None) == with_faces
        if with_rgb:
            assert np.array_equal(gc, rgb)
        if with_faces:
            assert np.array_equal(gf, faces)


def test_write_ply_refuses_bad_normals(tmp_path):
    io = pkg("meshio")
    path = str(tmp_path / "bad.ply")
    xyz = np.zeros((4, 3), np.float32)
    for bad in (np.zeros((3, 3), np.float32), np.zeros((4, 2), np.float32), np.zeros(12, np.float32), np.zeros((4, 3), np.float64),
                np.zeros((4, 3), np.int32), [[0.0, 0.0, 1.0]] * 4):
        with pytest.raises(ValueError):
            io.write_ply(path, xyz, normals=bad)
    io.write_ply(path, xyz, normals=np.zeros((4, 3), np.float32))
    assert read_ply(path)[2].shape == (4, 3)


HEAD = b"element vertex 3\nproperty float x\nproperty float y\nproperty float z\n"
HEAD_RGB = HEAD + b"property uchar red\nproperty uchar green\nproperty uchar blue\n"
FACE = b"element face 1\nproperty list uchar int vertex_indices\nend_header\n"
P0, P1, P2 = b"\x00" * 12, b"\x00\x00\xc0?\x00\x00\x00\x00\x00\x00\x00\xc0", b"\x00\x00\x00\x00\xcd\xcc\xcc=\xb0\x0f\xa14"
F0 = b"\x03\x00\x00\x00\x00\x01\x00\x00\x00\x02\x00\x00\x00"
# what write_ply wrote for this mesh before it took `normals` (recorded from that version)
BEFORE = {
    (True, True): b"ply\nformat binary_little_endian 1.0\n" + HEAD_RGB + FACE + P0 + b"\xff\x00\x07" + P1 + b"\x01\x02\x03" + P2 + b"\t\x08\xfa" + F0,
    (True, False): b"ply\nformat binary_little_endian 1.0\n" + HEAD + FACE + P0 + P1 + P2 + F0,
    (False, True): b"ply\nformat ascii 1.0\n" + HEAD_RGB + FACE + b"0 0 0 255 0 7\n1.5 0 -2 1 2 3\n0 0.100000001 3.00000011e-07 9 8 250\n3 0 1 2\n",
    (False, False): b"ply\nformat ascii 1.0\n" + HEAD + FACE + b"0 0 0\n1.5 0 -2\n0 0.100000001 3.00000011e-07\n3 0 1 2\n",
}


@pytest.mark.parametrize("binary,with_rgb", sorted(BEFORE))
def test_without_normals_the_file_is_what_it_was(tmp_path, binary, with_rgb):
    io = pkg("meshio")
    xyz = np.array([[0, 0, 0], [1.5, 0, -2], [0, 0.1, 3e-7]], np.float32)
    faces = np.array([[0, 1, 2]], np.int32)
    rgb = np.array([[255, 0, 7], [1, 2, 3], [9, 8, 250]], np.uint8)
    path = str(tmp_path / "b.ply")
    io.write_ply(path, xyz, faces=faces, rgb=rgb if with_rgb else None, binary=binary)
    assert open(path, "rb").read() == BEFORE[(binary, with_rgb)]
    io.write_ply(path, xyz, faces=faces, rgb=rgb if with_rgb else None, binary=binary, normals=None)
    assert open(path, "rb").read() == BEFORE[(binary, with_rgb)]
