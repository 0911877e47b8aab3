"""CPU tests of the TSDF volume's public face: include/sl3d_tsdf.h -- the header of the five calls, beside include/sl3d.h and
the headers of the other stages -- declares sl3d_tsdf_reset, sl3d_tsdf_integrate, sl3d_tsdf_extract, sl3d_get_tsdf and
sl3d_get_tsdf_surface and the two structures, states both rules and is plain C that compiles alone; the version is at least 0.26; the
binding's table for that header matches it position by position and shares no name with the other tables, the library exports the
symbols, Scanner has the methods and the module the bounds helper; the refusals that need no device."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np

from conftest import ROOT

CALLS = ["sl3d_get_tsdf", "sl3d_get_tsdf_surface", "sl3d_tsdf_extract", "sl3d_tsdf_integrate", "sl3d_tsdf_reset"]
INCLUDE = ["-I", os.path.join(ROOT, "include")]


def _header(name="sl3d_tsdf.h"):
    return open(os.path.join(ROOT, "include", name)).read()


def _code():
    return re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)


def _params(code, fn):
    """the parameter list of a declaration, one normalised string per parameter"""
    m = re.search(r"\bint\s+" + fn + r"\s*\(([^)]*)\)\s*;", code)
    assert m, fn
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def test_the_header_declares_the_calls():
    code = _code()
    assert sorted(set(re.findall(r"\b(sl3d_[a-z0-9_]+)\s*\(", code))) == CALLS
    assert re.findall(r"#define\s+(SL3D_\w+)", code) == ["SL3D_TSDF_H"]
    assert '#include "sl3d_align.h"' in code
    assert _params(code, "sl3d_tsdf_reset") == ["sl3d_ctx *ctx", "const sl3d_tsdf_volume *volume"]
    assert _params(code, "sl3d_tsdf_integrate") == ["sl3d_ctx *ctx", "int first_view", "int n_views", "int first_step", "const double est[4]", "int64_t counts[2]"]
    assert _params(code, "sl3d_tsdf_extract") == ["sl3d_ctx *ctx", "int64_t min_weight", "sl3d_tsdf_surface *device_out", "int64_t counts[3]"]
    assert _params(code, "sl3d_get_tsdf") == ["sl3d_ctx *ctx", "int32_t *sum", "uint32_t *weight", "int64_t capacity", "int64_t *n"]
    assert _params(code, "sl3d_get_tsdf_surface") == ["sl3d_ctx *ctx", "float *xyz", "float *normals", "int32_t *edge", "int64_t capacity", "int64_t *n"]
    assert re.search(r"typedef\s+struct\s*\{\s*float origin\[3\];\s*float voxel;\s*float trunc;\s*int32_t dims\[3\];\s*\}\s*sl3d_tsdf_volume\s*;", code)
    assert re.search(r"typedef\s+struct\s*\{\s*const float \*xyz;\s*const float \*normals;\s*const int32_t \*edge;\s*\}\s*sl3d_tsdf_surface\s*;", code)
    assert "sl3d_tsdf.h" in _header("sl3d.h")                                       # sl3d.h says where the calls are
    for other in ("sl3d.h", "sl3d_fuse.h", "sl3d_filter.h", "sl3d_voxel.h", "sl3d_align.h", "sl3d_align_plane.h"):        # ... and no other header declares them
        assert not any(re.search(r"\b" + fn + r"\s*\(", _header(other)) for fn in CALLS)


def test_the_header_states_the_rules():
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*typedef\s+struct\s*\{\s*float origin", _header(), flags=re.S)
    assert m
    text = " ".join(m.group(1).replace("\n *", "\n").split())
    for phrase in ("v = (k * ny + j) * nx + i", "X_a = ((double)i_a + 0.5) * L + (double)origin[a]", "c_0 = 1, s_0 = 0",
                   "c_{m+1} = c_m * c - s_m * s", "s_{m+1} = s_m * c + c_m * s", "no libm call is involved",
                   "View slot first_view + j of a call is the view with turntable index first_step + j",
                   "P.x = (c_m * x - (-s_m) * z) + tx", "P.y = X.y", "P.z = ((-s_m) * x + c_m * z) + tz",
                   "xc[i] = ((Rc[3i] * P.x + Rc[3i+1] * P.y) + Rc[3i+2] * P.z) + tc[i]", "xc.z <= 0 or not finite: no sample",
                   "u and v stay unrounded doubles", "fu = floor(u) - col0, fv = floor(v) - row0", "before any conversion to an integer",
                   "0 <= fu, fu + 1 < width, 0 <= fv and fv + 1 < height", "a NaN fails", "a = u - floor(u), b = v - floor(v)",
                   "valid == 1 and three finite coordinates", "z_dxdy = ((Rc[6] * q.x + Rc[7] * q.y) + Rc[8] * q.z) + tc[2]",
                   "max z - min z <= T", "zq = ((z00 * (1 - a) + z10 * a) * (1 - b)) + ((z01 * (1 - a) + z11 * a) * b)", "sdf = zq - xc.z",
                   "sdf >= -T", "d = sdf / T, and a d > 1 becomes 1", "q = (int32)rint(d * 32767.0), ties to even", "sum[v] += q; weight[v] += 1",
                   "neither the order of the views nor the number of calls can matter", "past 65535 is refused",
                   "counts[0] = the samples this call took, counts[1] = the voxels with weight > 0", "known iff weight >= min_weight",
                   "f(v) = (double)sum / (double)weight", "(f0 < 0) != (f1 < 0)", "t = f0 / (f0 - f1)", "(float)(X_a(v0) + t * L)",
                   "(f(v+) - f(v-)) * 0.5", "f(v+) - f(v)", "f(v) - f(v-)", "none: 0.0", "n_b = (g_b(v0) * (1 - t)) + (g_b(v1) * t)",
                   "len = sqrt((n0 * n0 + n1 * n1) + n2 * n2)", "otherwise three NaNs", "the normal points out of the object",
                   "edge int32[m] = 3 * v0 + a", "counts = (voxels, known voxels, m)", "a pure function of the two planes and min_weight",
                   "before anything is allocated or enqueued", "a refused call changes nothing", "nx * ny * nz > 2^28", "first_step + n_views > 65535",
                   "min_weight < 1", "capacity < 0", "SL3D_E_STATE: no calibration, or no dense result yet", "sl3d_get_tsdf_surface before an extract",
                   "SL3D_E_UNSUPPORTED: the 65535-view limit", "read points and valid only", "sl3d_destroy frees them",
                   "no group entry point and no shim call"):
        assert phrase in text, phrase


def test_the_header_is_plain_c_and_compiles_alone(tmp_path):
    """C99 with nothing but the standard headers and sl3d_align.h, which it includes itself."""
    src = tmp_path / "inc.c"
    src.write_text('#include "sl3d_tsdf.h"\nint main(void) { sl3d_tsdf_volume v = {{0.0f, 0.0f, 0.0f}, 1.0f, 3.0f, {4, 4, 4}}; sl3d_tsdf_surface s;\n'
                   '    double e[4] = {1.0, 0.0, 0.0, 0.0}; int64_t c[3], n; int32_t sum[64], edge[8]; uint32_t w[64]; float xyz[24], nrm[24];\n'
                   '    sl3d_turntable t; (void)t;\n'
                   '    return sl3d_tsdf_reset(0, &v) == SL3D_OK && sl3d_tsdf_integrate(0, 0, 1, 0, e, c) == SL3D_OK && sl3d_tsdf_extract(0, 1, &s, c) == SL3D_OK\n'
                   '        && sl3d_get_tsdf(0, sum, w, 64, &n) == SL3D_OK && sl3d_get_tsdf_surface(0, xyz, nrm, edge, 8, &n) == SL3D_OK && s.xyz == 0; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", *INCLUDE, "-c", str(src), "-o", str(tmp_path / "inc.o")])
    alone = tmp_path / "alone.c"                                                    # the header and nothing else
    alone.write_text('#include "sl3d_tsdf.h"\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", *INCLUDE, str(alone)])


def test_the_version_is_at_least_0_26(scanner_mod):
    m = re.search(r'#define\s+SL3D_VERSION_STRING\s+"0\.(\d+)\.', _header("sl3d.h"))
    assert m and int(m.group(1)) >= 26
    pkg = __import__("importlib").import_module("3dscan_amd")
    assert int(pkg.__version__.split(".")[1]) >= 26
    assert int(scanner_mod.load_library().sl3d_version().decode().split(".")[1]) >= 26


def test_the_binding_has_the_rows_and_the_methods(scanner_mod):
    S = scanner_mod
    assert S.TSDF_SYMBOLS == ("sl3d_tsdf_reset", "sl3d_tsdf_integrate", "sl3d_tsdf_extract", "sl3d_get_tsdf", "sl3d_get_tsdf_surface")      # the header's order
    code = _code()
    assert tuple(re.findall(r"\bint\s+(sl3d_[a-z0-9_]+)\s*\(", code)) == S.TSDF_SYMBOLS
    assert not set(S.TSDF_SYMBOLS) & (set(S.ABI_SYMBOLS) | set(S.FUSE_SYMBOLS) | set(S.FILTER_SYMBOLS) | set(S.VOXEL_SYMBOLS) | set(S.ALIGN_SYMBOLS)
                                      | set(S.ALIGN_PLANE_SYMBOLS))
    L, lib = S.load_library(), C.CDLL(S.LIB_PATH)
    assert all(hasattr(lib, name) for name in S.TSDF_SYMBOLS)
    assert all(getattr(L, name).restype is C.c_int for name in S.TSDF_SYMBOLS)
    # the header's parameters, position by position: a pointer is void *, the rest by its C type
    ctype = {"int": C.c_int, "int64_t": C.c_int64}

    def expected(fn):
        out = []
        for p in _params(code, fn):
            if "sl3d_tsdf_volume *" in p:
                out.append(C.POINTER(S.TsdfVolume))
            elif "sl3d_tsdf_surface *" in p:
                out.append(C.POINTER(S.TsdfSurface))
            elif p.startswith("int64_t counts[") or p == "int64_t *n":
                out.append(C.POINTER(C.c_int64))
            elif "*" in p or "[" in p:
                out.append(C.c_void_p)
            else:
                out.append(ctype[p.split()[0]])
        return out
    for fn in S.TSDF_SYMBOLS:
        assert getattr(L, fn).argtypes == expected(fn), fn
    assert [f[0] for f in S.TsdfVolume._fields_] == ["origin", "voxel", "trunc", "dims"] and C.sizeof(S.TsdfVolume) == 32
    assert [f[0] for f in S.TsdfSurface._fields_] == ["xyz", "normals", "edge"] and C.sizeof(S.TsdfSurface) == 24
    sig = lambda f: inspect.signature(f).parameters
    assert list(sig(S.Scanner.tsdf_reset)) == ["self", "origin", "voxel", "trunc", "dims"]
    p = sig(S.Scanner.tsdf_integrate)
    assert list(p) == ["self", "first_view", "n_views", "est", "first_step"] and p["first_step"].default == 0
    p = sig(S.Scanner.tsdf_extract)
    assert list(p)[:2] == ["self", "min_weight"] and p["min_weight"].default == 1
    assert list(sig(S.Scanner.tsdf_extract_device)) == ["self", "min_weight"] and list(sig(S.Scanner.tsdf_volume)) == ["self"]
    assert list(sig(S.tsdf_bounds)) == ["cloud", "voxel", "margin"]


def test_the_structures_match_the_header(tmp_path):
    """sizes and offsets of the two structures as a C compiler lays them out"""
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sl3d_tsdf.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu %zu\\n", '
                   'sizeof(sl3d_tsdf_volume), offsetof(sl3d_tsdf_volume, voxel), offsetof(sl3d_tsdf_volume, trunc), offsetof(sl3d_tsdf_volume, dims), '
                   'sizeof(sl3d_tsdf_surface), offsetof(sl3d_tsdf_surface, normals), offsetof(sl3d_tsdf_surface, edge)); return 0; }\n')
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", *INCLUDE, str(src), "-o", exe])
    assert subprocess.check_output([exe]).split() == [b"32", b"12", b"16", b"20", b"24", b"8", b"16"]


def test_the_bounds_helper(scanner_mod):
    import tsdf_reference as TR
    cloud = np.array([[1.2, -3.7, 100.4], [np.nan, 0.0, 0.0], [9.9, 4.1, 111.0], [5.0, 0.0, 105.0]], np.float32)
    for voxel, margin in ((1.0, 2), (0.5, 0), (0.75, 3)):
        origin, dims = scanner_mod.tsdf_bounds(cloud, voxel, margin)
        ro, rd = TR.bounds(cloud, voxel, margin)
        assert origin.dtype == np.float32 and np.array_equal(origin, ro) and dims == rd
        good = cloud[np.isfinite(cloud).all(axis=1)].astype(np.float64)
        lo, hi = origin.astype(np.float64), origin.astype(np.float64) + voxel * np.array(dims)
        assert (lo + margin * voxel <= good.min(axis=0) + 1e-4).all() and (hi - margin * voxel >= good.max(axis=0) - 1e-4).all()
    origin, dims = scanner_mod.tsdf_bounds(cloud, 1.0, 2)
    assert list(origin) == [-1.0, -6.0, 98.0] and dims == (13, 13, 15)


def test_the_refusals_that_need_no_device(scanner_mod):
    """Without a context nothing can be allocated or enqueued: every call is refused with SL3D_E_INVALID_ARG and writes nothing."""
    S = scanner_mod
    L = S.load_library()
    vol = S.TsdfVolume((C.c_float * 3)(0.0, 0.0, 0.0), 1.0, 3.0, (C.c_int32 * 3)(4, 4, 4))
    assert L.sl3d_tsdf_reset(None, C.byref(vol)) == -1
    est = (C.c_double * 4)(1.0, 0.0, 0.0, 0.0)
    counts = (C.c_int64 * 3)(-7, -7, -7)
    assert L.sl3d_tsdf_integrate(None, 0, 1, 0, est, counts) == -1 and list(counts) == [-7] * 3
    out = S.TsdfSurface(1, 2, 3)
    assert L.sl3d_tsdf_extract(None, 1, C.byref(out), counts) == -1 and list(counts) == [-7] * 3 and (out.xyz, out.normals, out.edge) == (1, 2, 3)
    n = C.c_int64(-7)
    words = np.full(8, -7, np.int32)
    assert L.sl3d_get_tsdf(None, words.ctypes.data, None, 8, C.byref(n)) == -1 and n.value == -7 and (words == -7).all()
    assert L.sl3d_get_tsdf_surface(None, None, None, words.ctypes.data, 8, C.byref(n)) == -1 and n.value == -7 and (words == -7).all()
