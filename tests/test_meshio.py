"""CPU test of 3dscan_amd/meshio.py: write_ply in ASCII and binary, with and without faces / colours, read back by a small parser
written here from the PLY format: header fields, counts, every value; malformed face lists are refused."""
import numpy as np
import pytest

from conftest import pkg


def read_ply(path):
    """-> (format, vertex property list, xyz float32 (n,3), rgb uint8 (n,3) or None, faces int32 (m,3) or None, header lines)"""
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
    assert vprops[:3] == [("float", "x"), ("float", "y"), ("float", "z")]
    has_rgb = len(vprops) == 6
    if has_rgb:
        assert vprops[3:] == [("uchar", "red"), ("uchar", "green"), ("uchar", "blue")]
    else:
        assert len(vprops) == 3
    m = None
    if len(elements) > 1:
        assert len(elements) == 2 and elements[1][0] == "face" and elements[1][2] == [("list", "uchar", "int", "vertex_indices")]
        m = elements[1][1]
    if fmt[1] == "ascii":
        lines = body.decode("ascii").splitlines()
        assert len(lines) == n + (m or 0)
        vt = [l.split() for l in lines[:n]]
        assert all(len(t) == (6 if has_rgb else 3) for t in vt)
        xyz = np.array([[np.float32(x) for x in t[:3]] for t in vt], dtype=np.float32).reshape(n, 3)
        rgb = np.array([[int(x) for x in t[3:]] for t in vt], dtype=np.uint8).reshape(n, 3) if has_rgb else None
        faces = None
        if m is not None:
            ft = [[int(x) for x in l.split()] for l in lines[n:]]
            assert all(len(t) == 4 and t[0] == 3 for t in ft)
            faces = np.array([t[1:] for t in ft], dtype=np.int32).reshape(m, 3)
    else:
        assert fmt[1] == "binary_little_endian"
        vdt = np.dtype([("p", "<f4", 3)] + ([("c", "u1", 3)] if has_rgb else []))
        assert vdt.itemsize == (15 if has_rgb else 12)
        v = np.frombuffer(body, dtype=vdt, count=n)
        xyz, rgb = v["p"].copy(), (v["c"].copy() if has_rgb else None)
        rest = body[n * vdt.itemsize:]
        faces = None
        if m is not None:
            fdt = np.dtype([("n", "u1"), ("i", "<i4", 3)])
            assert fdt.itemsize == 13 and len(rest) == 13 * m
            f = np.frombuffer(rest, dtype=fdt, count=m)
            assert (f["n"] == 3).all()
            faces = f["i"].astype(np.int32)
        else:
            assert len(rest) == 0
    return fmt[1], xyz, rgb, faces, head


def _mesh(rng, n, m):
    xyz = (rng.normal(0, 300, size=(n, 3)) * 10.0 ** rng.integers(-6, 3, size=(n, 1))).astype(np.float32)
    rgb = rng.integers(0, 256, size=(n, 3)).astype(np.uint8)
    faces = rng.integers(0, max(n, 1), size=(m, 3)).astype(np.int32)
    return xyz, rgb, faces


@pytest.mark.parametrize("binary", [True, False])
@pytest.mark.parametrize("with_faces", [True, False])
@pytest.mark.parametrize("with_rgb", [True, False])
def test_write_ply_reads_back(tmp_path, binary, with_faces, with_rgb):
    io = pkg("meshio")
    rng = np.random.default_rng(5)
    for n, m in ((257, 411), (1, 0), (0, 0)):
        xyz, rgb, faces = _mesh(rng, n, m)
        path = str(tmp_path / "m.ply")
        io.write_ply(path, xyz, faces=faces if with_faces else None, rgb=rgb if with_rgb else None, binary=binary)
        fmt, gx, gc, gf, head = read_ply(path)
        assert fmt == ("binary_little_endian" if binary else "ascii")
        assert f"element vertex {n}" in head and (f"element face {m}" in head) == with_faces
        assert gx.shape == (n, 3) and np.array_equal(gx.view(np.uint32), xyz.view(np.uint32))     # every float exactly
        assert (gc is not None) == with_rgb and (gf is not None) == with_faces
        if with_rgb:
            assert np.array_equal(gc, rgb)
        if with_faces:
            assert gf.shape == (m, 3) and np.array_equal(gf, faces)


def test_write_ply_refuses_bad_input(tmp_path):
    io = pkg("meshio")
    path = str(tmp_path / "bad.ply")
    xyz = np.zeros((4, 3), np.float32)
    for faces in (np.array([[0, 1, 4]], np.int32), np.array([[0, -1, 2]], np.int32),      # an id out of range
                  np.zeros((2, 4), np.int32), np.zeros(6, np.int32), np.zeros((2, 3), np.float32)):   # not (m, 3) integers
        with pytest.raises(ValueError):
            io.write_ply(path, xyz, faces=faces)
    with pytest.raises(ValueError):
        io.write_ply(path, np.zeros((4, 2), np.float32))
    with pytest.raises(ValueError):
        io.write_ply(path, xyz, rgb=np.zeros((3, 3), np.uint8))
    with pytest.raises(ValueError):
        io.write_ply(path, xyz, rgb=np.zeros((4, 3), np.float32))
    io.write_ply(path, xyz, faces=np.array([[0, 1, 3]], np.int64))                          # any integer type is taken
    assert np.array_equal(read_ply(path)[3], [[0, 1, 3]])
