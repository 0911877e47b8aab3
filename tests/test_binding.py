"""CPU tests of the ctypes binding itself (3dscan_amd/scanner.py), with a stand-in object in place of libsl3d.so: the prototype table
against include/sl3d.h, the one rule for missing symbols, and the two size-then-fill helpers against Python stand-ins of the C protocol."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "sl3d.h")
SCALARS = {"int": C.c_int, "int32_t": C.c_int, "unsigned": C.c_uint, "unsigned int": C.c_uint, "uint32_t": C.c_uint, "int64_t": C.c_int64,
           "uint64_t": C.c_uint64, "size_t": C.c_size_t, "float": C.c_float, "double": C.c_double}
RETURNS = {"int": C.c_int, "void": None, "const char *": C.c_char_p, "void *": C.c_void_p}


def _header_prototypes():
    """{name: (return type, [parameter kind])} of include/sl3d.h; a kind is a scalar C type or "*" for a pointer or an array."""
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    protos = {}
    for ret, name, params in re.findall(r"^((?:const\s+)?\w+\s*\*?)\s*(sl3d_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", txt, flags=re.M):
        kinds = []
        for p in ([] if params.strip() == "void" else params.split(",")):
            words = p.replace("const", " ").split()
            kinds.append("*" if "*" in p or "[" in p else " ".join(words[:-1]))
        protos[name] = (" ".join(ret.replace("*", " * ").split()), kinds)
    return protos


def _is_pointer(t):
    return t in (C.c_void_p, C.c_char_p) or (isinstance(t, type) and issubclass(t, C._Pointer))


class _Function:
    """What a fresh function of a ctypes library looks like, as far as load_library is concerned."""
    restype = C.c_int
    argtypes = None


class _Library:
    """Stand-in for ctypes.CDLL: every sl3d_* name but those in `missing` is there."""
    missing = ()

    def __init__(self, path):
        self.path = path

    def __getattr__(self, name):
        if not name.startswith("sl3d_") or name in self.missing:
            raise AttributeError(name)
        setattr(self, name, _Function())
        return self.__dict__[name]


def _load(scanner_mod, monkeypatch, missing=(), env=None):
    monkeypatch.setattr(C, "CDLL", type("Lib", (_Library,), {"missing": missing}))
    if env is None:
        monkeypatch.delenv("SL3D_LIB", raising=False)
    else:
        monkeypatch.setenv("SL3D_LIB", env)
    return scanner_mod.load_library(HEADER)    # any file that exists: the stand-in opens nothing


def test_prototype_table_matches_the_header(scanner_mod, monkeypatch):
    """Every function include/sl3d.h declares has, after load_library, the header's return type, parameter count and -- position by
    position -- kind of parameter: integer width and signedness, float or double, size_t, pointer."""
    header = _header_prototypes()
    assert len(header) == 99 and sorted(header) == sorted(scanner_mod.ABI_SYMBOLS)
    L = _load(scanner_mod, monkeypatch)
    for name, (ret, kinds) in header.items():
        fn = L.__dict__[name]
        assert fn.restype is RETURNS[ret], (name, ret, fn.restype)
        assert fn.argtypes is not None and len(fn.argtypes) == len(kinds), (name, kinds, fn.argtypes)
        for k, (kind, t) in enumerate(zip(kinds, fn.argtypes)):
            assert _is_pointer(t) if kind == "*" else t is SCALARS[kind], (name, k, kind, t)


def test_missing_symbol_raises_unless_another_build_is_named(scanner_mod, monkeypatch):
    """One rule for every symbol: without SL3D_LIB a build that lacks one does not load; with SL3D_LIB it loads, the symbol stays
    missing (a call fails with AttributeError) and every other function has its prototype."""
    with pytest.raises(AttributeError):
        _load(scanner_mod, monkeypatch, missing=("sl3d_get_residuals",))
    with pytest.raises(AttributeError):
        _load(scanner_mod, monkeypatch, missing=("sl3d_create",))
    L = _load(scanner_mod, monkeypatch, missing=("sl3d_get_residuals", "sl3d_create"), env=HEADER)
    assert not hasattr(L, "sl3d_get_residuals") and not hasattr(L, "sl3d_create")
    others = [n for n in scanner_mod.ABI_SYMBOLS if n not in L.missing]
    assert len(others) == 97 and all(L.__dict__[n].argtypes is not None for n in others)


def test_only_the_default_path_is_cached(scanner_mod, monkeypatch):
    before = scanner_mod._lib
    a, b = _load(scanner_mod, monkeypatch), _load(scanner_mod, monkeypatch)
    assert a is not b and scanner_mod._lib is before


@pytest.fixture
def handle(scanner_mod):
    """A Scanner that was never created (no library, no device): enough for the helpers, which need L, _h and _chk."""
    sc = object.__new__(scanner_mod.Scanner)
    sc._h, sc.L = "handle", type("L", (), {})()
    yield sc
    sc._h = None


def _write(ptr, rows, ctype, width, base):
    """What the C side does with an output: rows * width consecutive values from `base` on."""
    if rows:
        np.ctypeslib.as_array(C.cast(ptr, C.POINTER(ctype)), shape=(rows * width,))[:] = base + np.arange(rows * width)


VERTS, FACES = (2, 0, 3), (1, 0, 2)     # three views, the middle one empty


def _expected(counts, dtype, width, base):
    total = sum(counts)
    flat = (base + np.arange(total * width)).astype(dtype).reshape((total, width) if width > 1 else (total,))
    ends = np.cumsum(counts)
    return [flat[e - n:e] for n, e in zip(counts, ends)]


def _same(got, want, dtype):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.dtype == dtype and g.shape == w.shape and np.array_equal(g, w)


@pytest.mark.parametrize("with_normals", [True, False])
def test_batched_size_then_fill(handle, with_normals):
    """_fill_views against a stand-in of the C protocol (the argument order of sl3d_get_meshes_lod): counts always written, at most
    `capacity` rows written, null outputs only with capacity 0 -- or, for the optional output, when it is not requested."""
    calls = []

    def get(h, first_view, n_views, step, max_edge, xyz, ids, nrm, vcap, faces, fcap, nv, nf):
        calls.append(((h, first_view, n_views, step, max_edge), (vcap, fcap), nrm is not None))
        assert (xyz is None) == (ids is None) == (vcap == 0) and (faces is None) == (fcap == 0)
        assert nrm is None or vcap > 0
        nv[:], nf[:] = VERTS, FACES
        _write(xyz, min(vcap, sum(VERTS)), C.c_float, 3, 0)
        _write(ids, min(vcap, sum(VERTS)), C.c_int32, 1, 100)
        if nrm is not None:
            _write(nrm, min(vcap, sum(VERTS)), C.c_float, 3, 200)
        _write(faces, min(fcap, sum(FACES)), C.c_int32, 3, 300)
        return 0

    handle.L.get = get
    f32, i32 = (np.float32, 3), (np.int32,)
    (xyz, ids, nrm), (faces,), (nv, nf) = handle._fill_views("get", 1, 3, (4, 2.5), [f32, i32, f32 if with_normals else None], [(np.int32, 3)],
                                                             n_counts=2)
    assert calls == [(("handle", 1, 3, 4, 2.5), (0, 0), False), (("handle", 1, 3, 4, 2.5), (5, 3), with_normals)]
    assert tuple(nv) == VERTS and tuple(nf) == FACES
    _same(xyz, _expected(VERTS, np.float32, 3, 0), np.float32)
    _same(ids, _expected(VERTS, np.int32, 1, 100), np.int32)
    _same(faces, _expected(FACES, np.int32, 3, 300), np.int32)
    assert [a.shape for a in xyz] == [(2, 3), (0, 3), (3, 3)] and [a.shape for a in ids] == [(2,), (0,), (3,)]
    assert [a.shape for a in faces] == [(1, 3), (0, 3), (2, 3)]
    if with_normals:
        _same(nrm, _expected(VERTS, np.float32, 3, 200), np.float32)
    else:
        assert nrm is None


def test_batched_size_then_fill_into_the_callers_array(handle):
    """An array in place of a spec is filled instead of a fresh one, its length is the capacity; one too short stops before the fill."""
    caps = []

    def get(h, first_view, n_views, xyz, cap, n):
        caps.append(cap)
        assert (xyz is None) == (cap == 0)
        n[:] = VERTS
        _write(xyz, min(cap, sum(VERTS)), C.c_float, 3, 0)
        return 0

    handle.L.get = get
    out = np.full((7, 3), -1, dtype=np.float32)
    (clouds,), _ = handle._fill_views("get", 0, 3, (), [out], n_counts=1)
    assert caps == [0, 7] and all(c.base is out for c in clouds) and (out[5:] == -1).all()
    _same(clouds, _expected(VERTS, np.float32, 3, 0), np.float32)
    with pytest.raises(AssertionError):
        handle._fill_views("get", 0, 3, (), [out[:4]], n_counts=1)
    assert caps == [0, 7, 0]


@pytest.mark.parametrize("total", [0, 3])
def test_single_count_size_then_fill(handle, total):
    """_fill against a stand-in of the C protocol (the argument order of sl3d_get_cloud_rgb)."""
    calls = []

    def get(h, view, xyz, rgb, cap, n):
        calls.append(((h, view), cap))
        assert (xyz is None) == (rgb is None) and (xyz is not None or cap == 0)
        n._obj.value = total
        _write(xyz, min(cap, total), C.c_float, 3, 0)
        _write(rgb, min(cap, total), C.c_uint8, 3, 50)
        return 0

    handle.L.get = get
    xyz, rgb = handle._fill("get", (2,), (np.float32, 3), (np.uint8, 3))
    assert calls == [(("handle", 2), 0), (("handle", 2), total)]
    assert xyz.dtype == np.float32 and rgb.dtype == np.uint8 and xyz.shape == rgb.shape == (total, 3)
    assert np.array_equal(xyz, _expected([total], np.float32, 3, 0)[0]) and np.array_equal(rgb, _expected([total], np.uint8, 3, 50)[0])


def test_a_status_stops_the_helpers_after_the_first_call(handle, scanner_mod):
    """A failing size call raises through _chk with the call's name and the handle's last error; nothing is allocated or called again."""
    calls = []
    handle.L.get = lambda *a: calls.append(a) or -4
    handle.L.sl3d_strerror = lambda rc: b"state"
    handle.L.sl3d_last_error = lambda h: b"too early"
    with pytest.raises(scanner_mod.Sl3dError, match="get: state: too early"):
        handle._fill("get", (0,), (np.float32, 3))
    with pytest.raises(scanner_mod.Sl3dError, match="get: state: too early"):
        handle._fill_views("get", 0, 1, (), [(np.float32, 3)], n_counts=1)
    assert len(calls) == 2
