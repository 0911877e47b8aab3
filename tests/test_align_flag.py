"""CPU tests of the turntable refinement's public face: include/sl3d_align.h -- the header of the four calls, beside include/sl3d.h,
include/sl3d_fuse.h, include/sl3d_filter.h and include/sl3d_voxel.h -- declares sl3d_align_sums, sl3d_align_solve, sl3d_refine_turntable and
sl3d_get_align_camera, the two structures and the three constants, states the rule and is plain C that compiles alone; the version is at
least 0.24; the binding's table for that header matches it position by position and shares no name with the other four tables, the
library exports the symbols, Scanner has the methods and the module the solve; the refusals that need no device."""
import ctypes as C
import inspect
import os
import re
import subprocess

from conftest import ROOT

CALLS = ["sl3d_align_solve", "sl3d_align_sums", "sl3d_get_align_camera", "sl3d_refine_turntable"]


def _header(name="sl3d_align.h"):
    return open(os.path.join(ROOT, "include", name)).read()


def _params(code, fn):
    """the parameter list of a declaration, one normalised string per parameter"""
    m = re.search(r"\bint\s+" + fn + r"\s*\(([^)]*)\)\s*;", code)
    assert m, fn
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def test_the_header_declares_the_calls():
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert sorted(set(re.findall(r"\b(sl3d_[a-z0-9_]+)\s*\(", code))) == CALLS
    assert re.findall(r"#define\s+(SL3D_\w+)", code) == ["SL3D_ALIGN_H", "SL3D_ALIGN_WORDS", "SL3D_ALIGN_MAX_WINDOW", "SL3D_ALIGN_MAX_ITERATIONS"]
    assert re.search(r"#define\s+SL3D_ALIGN_WORDS\s+12\b", code) and re.search(r"#define\s+SL3D_ALIGN_MAX_WINDOW\s+4\b", code)
    assert re.search(r"#define\s+SL3D_ALIGN_MAX_ITERATIONS\s+64\b", code)
    assert _params(code, "sl3d_align_sums") == ["sl3d_ctx *ctx", "int first_view", "int n_views", "const double est[4]", "double ox", "double oz",
                                                "float range", "float max_dist", "int window", "int64_t *sums"]
    assert _params(code, "sl3d_align_solve") == ["const int64_t *sums", "int n_pairs", "float range", "double ox", "double oz", "const double est_in[4]",
                                                 "double est_out[4]", "double stats[4]"]
    assert _params(code, "sl3d_refine_turntable") == ["sl3d_ctx *ctx", "int first_view", "int n_views", "float tx", "float ty", "float tz", "float rot_step",
                                                      "float range", "float max_dist", "int window", "int iterations", "sl3d_turntable *out",
                                                      "sl3d_align_iteration *log", "int *n_done"]
    assert _params(code, "sl3d_get_align_camera") == ["sl3d_ctx *ctx", "double cam[26]"]
    assert re.search(r"typedef\s+struct\s*\{\s*float tx, ty, tz, rot_step;\s*double est\[4\];\s*int64_t n, sources;\s*double rms_xz, rms_y;\s*"
                     r"int32_t degenerate, reserved;\s*\}\s*sl3d_turntable\s*;", code)
    assert re.search(r"typedef\s+struct\s*\{\s*double est\[4\];\s*int64_t n, sources;\s*double rms_xz, rms_y;\s*\}\s*sl3d_align_iteration\s*;", code)
    assert "sl3d_align.h" in _header("sl3d.h")                                      # sl3d.h says where the calls are
    for other in ("sl3d.h", "sl3d_fuse.h", "sl3d_filter.h", "sl3d_voxel.h"):        # ... and no other header declares them
        assert not any(re.search(r"\b" + fn + r"\s*\(", _header(other)) for fn in CALLS)


def test_the_header_states_the_rule():
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*#define\s+SL3D_ALIGN_WORDS", _header(), flags=re.S)
    assert m
    text = " ".join(m.group(1).replace("\n *", "\n").split())
    for phrase in ("p^.x = (c * x - s * z) + tx", "p^.z = (s * x + c * z) + tz", "p^.y = (double)p.y",
                   "xc[i] = ((Rc[3i] * p^.x + Rc[3i+1] * p^.y) + Rc[3i+2] * p^.z) + tc[i]", "xc.z <= 0 or not finite: a source with no candidate",
                   "r2 = xn * xn + yn * yn", "rad = 1 + r2 * (k1 + r2 * (k2 + r2 * k3))", "xd = xn * rad + (2 * p1 * xn * yn + p2 * (r2 + 2 * xn * xn))",
                   "yd = yn * rad + (p1 * (r2 + 2 * yn * yn) + 2 * p2 * xn * yn)", "w = (Kc[6] * xd + Kc[7] * yd) + Kc[8]",
                   "Zero coefficients are multiplied like any others", "cc = rint(u) - col0, rr = rint(v) - row0, ties to even",
                   "magnitude < 2^30", "before any conversion to an integer", "never to the pitch", "d2 = (ex * ex + ey * ey) + ez * ez",
                   "strictly smaller", "ties go to the first", "an overflowed d2 is never chosen", "d2 <= (double)max_dist * (double)max_dist",
                   "Q = 262144.0 / (double)range", "e = ((double)w - o) * Q", "in range iff |e| < 262144.0", "(int64)rint(e)", "UNTRANSFORMED source",
                   "dy = (int64)rint(((double)q.y - (double)p.y) * Q)", "0 = accepted pairs n", "5 = sum (ax * bx + az * bz)", "6 = sum (ax * bz - az * bx)",
                   "11 = sources", "the order of arrival cannot matter", "below 2^37", "width * height >= 2^25", "no float atomics",
                   "pair j is (source view first_view + j + 1, target view first_view + j)", "X = c x - s z, Z = s x + c z, Y = y",
                   "added in 128 bits", "theta = atan2(X, C)", "(I - R') t' = d", "tx' = ox + t'x / Q", "N < 2, or X == 0 and C == 0, or c' == 1.0",
                   "ty is unobservable under this model and is passed through", "before anything is allocated or enqueued",
                   "a refused call changes nothing", "max_dist > range", "window outside 0 .. 4", "iterations outside 1 .. 64",
                   "SL3D_E_STATE: no calibration, or no dense result yet", "read points and valid only", "nor the voxel result",
                   "sl3d_destroy frees them", "no group entry point and no shim call"):
        assert phrase in text, phrase


def test_the_header_is_plain_c_and_compiles_alone(tmp_path):
    """C99 with nothing but the standard headers and sl3d.h, which it includes itself."""
    src = tmp_path / "inc.c"
    src.write_text('#include "sl3d_align.h"\nint main(void) { int64_t w[SL3D_ALIGN_WORDS]; double e[4] = {1.0, 0.0, 0.0, 0.0}, o[4], s[4], cam[26]; int n;\n'
                   '    sl3d_turntable t; sl3d_align_iteration log[SL3D_ALIGN_MAX_ITERATIONS];\n'
                   '    return sl3d_align_sums(0, 0, 2, e, 0.0, 0.0, 1.0f, 1.0f, SL3D_ALIGN_MAX_WINDOW, w) == SL3D_OK && sl3d_align_solve(w, 1, 1.0f, 0.0, 0.0, e, o, s) == SL3D_OK\n'
                   '        && sl3d_refine_turntable(0, 0, 2, 0.0f, 0.0f, 0.0f, 20.0f, 1.0f, 1.0f, 2, 20, &t, log, &n) == SL3D_OK\n'
                   '        && sl3d_get_align_camera(0, cam) == SL3D_OK && t.n == log[0].n; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                           "-o", str(tmp_path / "inc.o")])
    subprocess.check_call(["cc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])
    alone = tmp_path / "alone.c"                                                    # the header and nothing else
    alone.write_text('#include "sl3d_align.h"\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(alone)])


def test_the_version_is_at_least_0_24(scanner_mod):
    m = re.search(r'#define\s+SL3D_VERSION_STRING\s+"0\.(\d+)\.', _header("sl3d.h"))
    assert m and int(m.group(1)) >= 24
    pkg = __import__("importlib").import_module("3dscan_amd")
    assert int(pkg.__version__.split(".")[1]) >= 24
    assert int(scanner_mod.load_library().sl3d_version().decode().split(".")[1]) >= 24


def test_the_binding_has_the_rows_and_the_methods(scanner_mod):
    S = scanner_mod
    assert S.ALIGN_SYMBOLS == ("sl3d_align_sums", "sl3d_align_solve", "sl3d_refine_turntable", "sl3d_get_align_camera")      # the header's order
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert tuple(re.findall(r"\bint\s+(sl3d_[a-z0-9_]+)\s*\(", code)) == S.ALIGN_SYMBOLS
    assert not set(S.ALIGN_SYMBOLS) & (set(S.ABI_SYMBOLS) | set(S.FUSE_SYMBOLS) | set(S.FILTER_SYMBOLS) | set(S.VOXEL_SYMBOLS))
    L, lib = S.load_library(), C.CDLL(S.LIB_PATH)
    assert all(hasattr(lib, name) for name in S.ALIGN_SYMBOLS)
    assert all(getattr(L, name).restype is C.c_int for name in S.ALIGN_SYMBOLS)
    # the header's parameters, position by position: a pointer is void *, the rest by its C type
    ctype = {"int": C.c_int, "float": C.c_float, "double": C.c_double}

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
    for fn in S.ALIGN_SYMBOLS:
        assert getattr(L, fn).argtypes == expected(fn), fn
    assert [f[0] for f in S.Turntable._fields_] == ["tx", "ty", "tz", "rot_step", "est", "n", "sources", "rms_xz", "rms_y", "degenerate", "reserved"]
    assert C.sizeof(S.Turntable) == 88 and S.Turntable.est.offset == 16 and S.Turntable.n.offset == 48 and S.Turntable.degenerate.offset == 80
    assert [f[0] for f in S.AlignIteration._fields_] == ["est", "n", "sources", "rms_xz", "rms_y"] and C.sizeof(S.AlignIteration) == 64
    assert S.ALIGN_WORDS == 12
    p = inspect.signature(S.Scanner.refine_turntable).parameters
    assert list(p) == ["self", "first_view", "n_views", "tx", "ty", "tz", "rot_step", "range", "max_dist", "window", "iterations"]
    assert p["window"].default == 2 and p["iterations"].default == 20
    p = inspect.signature(S.Scanner.align_sums).parameters
    assert list(p) == ["self", "first_view", "n_views", "est", "ox", "oz", "range", "max_dist", "window"] and p["window"].default == 2
    assert list(inspect.signature(S.Scanner.align_camera).parameters) == ["self"]
    assert list(inspect.signature(S.align_solve).parameters) == ["sums", "range", "ox", "oz", "est"]


def test_the_structures_match_the_header(tmp_path):
    """sizes and offsets of the two structures as a C compiler lays them out"""
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sl3d_align.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu\\n", '
                   'sizeof(sl3d_turntable), offsetof(sl3d_turntable, est), offsetof(sl3d_turntable, n), offsetof(sl3d_turntable, rms_xz), '
                   'offsetof(sl3d_turntable, degenerate), sizeof(sl3d_align_iteration), offsetof(sl3d_align_iteration, n), '
                   'offsetof(sl3d_align_iteration, rms_xz)); return 0; }\n')
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    assert subprocess.check_output([exe]).split() == [b"88", b"16", b"48", b"64", b"80", b"64", b"32", b"48"]


def test_the_refusals_that_need_no_device(scanner_mod):
    """Without a context nothing can be allocated or enqueued: every call is refused with SL3D_E_INVALID_ARG and writes nothing."""
    S = scanner_mod
    L = S.load_library()
    est = (C.c_double * 4)(1.0, 0.0, 0.0, 0.0)
    sums = (C.c_int64 * 12)(*([-7] * 12))
    assert L.sl3d_align_sums(None, 0, 2, est, 0.0, 0.0, 1.0, 1.0, 2, sums) == -1 and list(sums) == [-7] * 12
    out, log, done = S.Turntable(), (S.AlignIteration * 4)(), C.c_int(-7)
    out.n = -7
    assert L.sl3d_refine_turntable(None, 0, 2, 0.0, 0.0, 0.0, 20.0, 1.0, 1.0, 2, 4, C.byref(out), log, C.byref(done)) == -1
    assert out.n == -7 and done.value == -7 and log[0].n == 0
    cam = (C.c_double * 26)(*([-7.0] * 26))
    assert L.sl3d_get_align_camera(None, cam) == -1 and list(cam) == [-7.0] * 26
