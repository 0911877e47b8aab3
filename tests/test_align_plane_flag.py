"""CPU tests of the point-to-plane refinement's public face: include/sl3d_align_plane.h -- the header of the five calls, beside
include/sl3d_align.h, which it includes -- declares sl3d_align_normals, sl3d_get_align_normals, sl3d_align_plane_sums, sl3d_align_plane_solve
and sl3d_refine_turntable_plane and the two constants, states the rule and is plain C that compiles alone; the version is at least 0.25;
the binding's table for that header matches it position by position and shares no name with the other tables, the library exports the
symbols, Scanner has the methods and the module the solve; the refusals that need no device."""
import ctypes as C
import inspect
import os
import re
import subprocess

from conftest import ROOT

CALLS = ["sl3d_align_normals", "sl3d_align_plane_solve", "sl3d_align_plane_sums", "sl3d_get_align_normals", "sl3d_refine_turntable_plane"]


def _header(name="sl3d_align_plane.h"):
    return open(os.path.join(ROOT, "include", name)).read()


def _params(code, fn):
    """the parameter list of a declaration, one normalised string per parameter"""
    m = re.search(r"\bint\s+" + fn + r"\s*\(([^)]*)\)\s*;", code)
    assert m, fn
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def test_the_header_declares_the_calls():
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert sorted(set(re.findall(r"\b(sl3d_[a-z0-9_]+)\s*\(", code))) == CALLS
    assert re.findall(r"#define\s+(SL3D_\w+)", code) == ["SL3D_ALIGN_PLANE_H", "SL3D_ALIGN_PLANE_WORDS", "SL3D_ALIGN_PLANE_STEPS"]
    assert re.search(r"#define\s+SL3D_ALIGN_PLANE_WORDS\s+18\b", code) and re.search(r"#define\s+SL3D_ALIGN_PLANE_STEPS\s+8\b", code)
    assert re.search(r'#include\s+"sl3d_align.h"', code) and "typedef" not in code              # the two structures are sl3d_align.h's
    assert _params(code, "sl3d_align_normals") == ["sl3d_ctx *ctx", "int first_view", "int n_views", "float normal_edge"]
    assert _params(code, "sl3d_get_align_normals") == ["sl3d_ctx *ctx", "int view", "float *dst", "size_t row_stride_bytes"]
    assert _params(code, "sl3d_align_plane_sums") == ["sl3d_ctx *ctx", "int first_view", "int n_views", "const double est[4]", "double ox", "double oz",
                                                      "float range", "float max_dist", "float normal_edge", "int window", "int64_t *sums"]
    assert _params(code, "sl3d_align_plane_solve") == ["const int64_t *sums", "int n_pairs", "float range", "double ox", "double oz",
                                                       "const double est_in[4]", "double est_out[4]", "double stats[4]"]
    assert _params(code, "sl3d_refine_turntable_plane") == ["sl3d_ctx *ctx", "int first_view", "int n_views", "float tx", "float ty", "float tz",
                                                            "float rot_step", "float range", "float max_dist", "float normal_edge", "int window",
                                                            "int iterations", "sl3d_turntable *out", "sl3d_align_iteration *log", "int *n_done"]
    assert "sl3d_align_plane.h" in _header("sl3d.h")                                # sl3d.h says where the calls are
    for other in ("sl3d.h", "sl3d_fuse.h", "sl3d_filter.h", "sl3d_voxel.h", "sl3d_align.h"):    # ... and no other header declares them
        assert not any(re.search(r"\b" + fn + r"\s*\(", _header(other)) for fn in CALLS)


def test_the_header_states_the_rule():
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*#define\s+SL3D_ALIGN_PLANE_WORDS", _header(), flags=re.S)
    assert m
    text = " ".join(m.group(1).replace("\n *", "\n").split())
    for phrase in ("valid == 1 and three finite coordinates at the pixel and at its four neighbours", "never the pitch",
                   "a pixel of the window's border has no normal", "(ex * ex + ey * ey) + ez * ez <= (double)normal_edge * (double)normal_edge",
                   "a = right - left, b = down - up", "n.x = (a.y * b.z) - (a.z * b.y)", "n.y = (a.z * b.x) - (a.x * b.z)",
                   "n.z = (a.x * b.y) - (a.y * b.x)", "len2 = (n.x * n.x + n.y * n.y) + n.z * n.z", "len = sqrt(len2)", "len finite and > 0",
                   "(float)(n.x / len)", "all three floats are NaN: no normal", "the residual is squared",
                   "Steps 1 - 4 of the rule in sl3d_align.h are taken over verbatim", "the best candidate's pixel is remembered",
                   "d2 <= (double)max_dist * (double)max_dist", "the best candidate's pixel has a normal", "counted in word 17",
                   "not re-matched with a farther candidate", "UNTRANSFORMED source", "A = n.x * p'x + n.z * p'z", "B = n.z * p'x - n.x * p'z",
                   "D = n.y * ((double)p.y - (double)q.y) - (n.x * q'x + n.z * q'z)", "c A + s B + u n.x + w n.z + D",
                   "u = (1 - c) t'x + s t'z and w = (1 - c) t'z - s t'x", "Qp = 65536.0 / (double)range", "Qn = 65536.0",
                   "in range iff |e| < 262144.0", "(int64)rint(e)", "0 = accepted pairs n", "1 - 15 = the upper triangle, row-major",
                   "16 = sources", "17 = sources lost to a missing normal", "a product below 2^36", "width * height >= 2^25", "below 2^61",
                   "the order of arrival cannot matter", "no float atomics", "the words do not depend on the estimate", "added in 128 bits",
                   "rounded to double once", "scaled by 2^-16 (exact)", "g = (c, s, u, w, 1)", "theta = atan2(s, c)",
                   "SL3D_ALIGN_PLANE_STEPS Gauss-Newton steps", "(0, 0, 1, 0, 0), (0, 0, 0, 1, 0), (-s, c, 0, 0, 0)", "L D L^T",
                   "in the order u, w, theta", "d1 = Hww - l10 * Huw", "d2 = (Htt - l20 * Hut) - l21 * e21", "m = 1 - c', det = m * m + s' * s'",
                   "tx' = ox + t'x / Qp", "rms_plane = sqrt(max(g M g, 0) / N) / Qp", "N < 3", "2^-40 times its diagonal entry",
                   "a single plane, a surface of revolution about the axis", "c' == 1.0", "ty is unobservable under this model and is passed through",
                   "normals of its target views once, before the first pass", "one pass launch and one solve per iteration", "Pi = 22/7",
                   "rms_xz carries rms_plane, rms_y is NaN", "before anything is allocated or enqueued", "a refused call changes nothing",
                   "normal_edge that is NaN, infinite or <= 0", "SL3D_E_STATE if that view's normals were never computed",
                   "read points and valid only", "sl3d_destroy frees them", "always recompute", "no group entry point and no shim call"):
        assert phrase in text, phrase


def test_the_header_is_plain_c_and_compiles_alone(tmp_path):
    """C99 with nothing but the standard headers, sl3d.h and sl3d_align.h, which it includes itself."""
    src = tmp_path / "inc.c"
    src.write_text('#include "sl3d_align_plane.h"\nint main(void) { int64_t w[SL3D_ALIGN_PLANE_WORDS]; double e[4] = {1.0, 0.0, 0.0, 0.0}, o[4], s[4]; int n;\n'
                   '    float nrm[3]; sl3d_turntable t; sl3d_align_iteration log[SL3D_ALIGN_MAX_ITERATIONS];\n'
                   '    return sl3d_align_normals(0, 0, 1, 2.0f) == SL3D_OK && sl3d_get_align_normals(0, 0, nrm, sizeof nrm) == SL3D_OK\n'
                   '        && sl3d_align_plane_sums(0, 0, 2, e, 0.0, 0.0, 1.0f, 1.0f, 2.0f, SL3D_ALIGN_MAX_WINDOW, w) == SL3D_OK\n'
                   '        && sl3d_align_plane_solve(w, 1, 1.0f, 0.0, 0.0, e, o, s) == SL3D_OK\n'
                   '        && sl3d_refine_turntable_plane(0, 0, 2, 0.0f, 0.0f, 0.0f, 20.0f, 1.0f, 1.0f, 2.0f, 2, SL3D_ALIGN_PLANE_STEPS, &t, log, &n) == SL3D_OK\n'
                   '        && t.n == log[0].n; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                           "-o", str(tmp_path / "inc.o")])
    subprocess.check_call(["cc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])
    alone = tmp_path / "alone.c"                                                    # the header and nothing else
    alone.write_text('#include "sl3d_align_plane.h"\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(alone)])


def test_the_version_is_at_least_0_25(scanner_mod):
    m = re.search(r'#define\s+SL3D_VERSION_STRING\s+"0\.(\d+)\.', _header("sl3d.h"))
    assert m and int(m.group(1)) >= 25
    pkg = __import__("importlib").import_module("3dscan_amd")
    assert int(pkg.__version__.split(".")[1]) >= 25
    assert int(scanner_mod.load_library().sl3d_version().decode().split(".")[1]) >= 25


def test_the_binding_has_the_rows_and_the_methods(scanner_mod):
    S = scanner_mod
    assert S.ALIGN_PLANE_SYMBOLS == ("sl3d_align_normals", "sl3d_get_align_normals", "sl3d_align_plane_sums", "sl3d_align_plane_solve",
                                     "sl3d_refine_turntable_plane")                            # the header's order
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert tuple(re.findall(r"\bint\s+(sl3d_[a-z0-9_]+)\s*\(", code)) == S.ALIGN_PLANE_SYMBOLS
    assert not set(S.ALIGN_PLANE_SYMBOLS) & (set(S.ABI_SYMBOLS) | set(S.FUSE_SYMBOLS) | set(S.FILTER_SYMBOLS) | set(S.VOXEL_SYMBOLS) | set(S.ALIGN_SYMBOLS))
    L, lib = S.load_library(), C.CDLL(S.LIB_PATH)
    assert all(hasattr(lib, name) for name in S.ALIGN_PLANE_SYMBOLS)
    assert all(getattr(L, name).restype is C.c_int for name in S.ALIGN_PLANE_SYMBOLS)
    # the header's parameters, position by position: a pointer is void *, the rest by its C type
    ctype = {"int": C.c_int, "float": C.c_float, "double": C.c_double, "size_t": C.c_size_t}

    def expected(fn):
        out = []
        for p in _params(code, fn):
            if "sl3d_turntable *" in p:
                out.append(C.POINTER(S.Turntable))
            elif "sl3d_align_iteration *" in p:
                out.append(C.POINTER(S.AlignIteration))
            elif p == "int *n_done":
                out.append(C.POINTER(C.c_int))
            elif "*" in p or "[" in p:
                out.append(C.c_void_p)
            else:
                out.append(ctype[p.split()[0]])
        return out
    for fn in S.ALIGN_PLANE_SYMBOLS:
        assert getattr(L, fn).argtypes == expected(fn), fn
    assert S.ALIGN_PLANE_WORDS == 18
    p = inspect.signature(S.Scanner.refine_turntable_plane).parameters
    assert list(p) == ["self", "first_view", "n_views", "tx", "ty", "tz", "rot_step", "range", "max_dist", "normal_edge", "window", "iterations"]
    assert p["window"].default == 2 and p["iterations"].default == 20
    p = inspect.signature(S.Scanner.align_plane_sums).parameters
    assert list(p) == ["self", "first_view", "n_views", "est", "ox", "oz", "range", "max_dist", "normal_edge", "window"] and p["window"].default == 2
    assert list(inspect.signature(S.Scanner.align_normals).parameters) == ["self", "first_view", "n_views", "normal_edge"]
    assert list(inspect.signature(S.Scanner.align_normal_plane).parameters) == ["self", "view"]
    assert list(inspect.signature(S.align_plane_solve).parameters) == ["sums", "range", "ox", "oz", "est"]


def test_the_refusals_that_need_no_device(scanner_mod):
    """Without a context nothing can be allocated or enqueued: every call is refused with SL3D_E_INVALID_ARG and writes nothing."""
    S = scanner_mod
    L = S.load_library()
    est = (C.c_double * 4)(1.0, 0.0, 0.0, 0.0)
    sums = (C.c_int64 * 18)(*([-7] * 18))
    assert L.sl3d_align_plane_sums(None, 0, 2, est, 0.0, 0.0, 1.0, 1.0, 2.0, 2, sums) == -1 and list(sums) == [-7] * 18
    out, log, done = S.Turntable(), (S.AlignIteration * 4)(), C.c_int(-7)
    out.n = -7
    assert L.sl3d_refine_turntable_plane(None, 0, 2, 0.0, 0.0, 0.0, 20.0, 1.0, 1.0, 2.0, 2, 4, C.byref(out), log, C.byref(done)) == -1
    assert out.n == -7 and done.value == -7 and log[0].n == 0
    nrm = (C.c_float * 3)(-7.0, -7.0, -7.0)
    assert L.sl3d_align_normals(None, 0, 1, 2.0) == -1
    assert L.sl3d_get_align_normals(None, 0, nrm, 12) == -1 and list(nrm) == [-7.0] * 3
