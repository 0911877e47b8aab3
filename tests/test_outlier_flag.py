"""CPU tests of the outlier filter's public face: include/sl3d_filter.h -- the header of the two calls, beside include/sl3d.h and
include/sl3d_fuse.h -- declares sl3d_filter_outliers, sl3d_get_support and SL3D_FILTER_MAX_RADIUS, states the rule and is plain C; the
version is at least 0.22; the binding's table for that header matches it position by position and shares no name with the other two
tables, the library exports both symbols, Scanner has the two methods."""
import ctypes as C
import inspect
import os
import re
import subprocess

from conftest import ROOT


def _header(name="sl3d_filter.h"):
    return open(os.path.join(ROOT, "include", name)).read()


def test_the_header_declares_the_calls():
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert re.search(r"#define\s+SL3D_FILTER_MAX_RADIUS\s+4\b", code)
    assert re.search(r"\bint\s+sl3d_filter_outliers\s*\(\s*sl3d_ctx\s*\*\s*ctx\s*,\s*int\s+first_view\s*,\s*int\s+n_views\s*,\s*int\s+radius\s*,"
                     r"\s*float\s+max_dist\s*,\s*int\s+min_neighbours\s*,\s*uint32_t\s*\*\s*counts\s*\)\s*;", code)
    assert re.search(r"\bint\s+sl3d_get_support\s*\(\s*sl3d_ctx\s*\*\s*ctx\s*,\s*int\s+view\s*,\s*uint8_t\s*\*\s*out\s*,\s*size_t\s+stride\s*\)\s*;", code)
    assert sorted(set(re.findall(r"\b(sl3d_[a-z0-9_]+)\s*\(", code))) == ["sl3d_filter_outliers", "sl3d_get_support"]
    assert re.findall(r"#define\s+(SL3D_\w+)", code) == ["SL3D_FILTER_H", "SL3D_FILTER_MAX_RADIUS"]
    assert "sl3d_filter.h" in _header("sl3d.h")                     # sl3d.h says where the calls are
    for other in ("sl3d.h", "sl3d_fuse.h"):                         # ... and neither other header declares them
        assert "sl3d_filter_outliers" not in _header(other) and "sl3d_get_support" not in _header(other)


def test_the_header_states_the_rule():
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*#define\s+SL3D_FILTER_MAX_RADIUS", _header(), flags=re.S)
    assert m
    text = " ".join(m.group(1).replace("*", " ").split())
    words = " ".join(re.sub(r"\n \*", "\n", m.group(1)).split())
    for phrase in ("(dx*dx + dy*dy) + dz*dz with dx = (double)p.x - (double)q.x", "thr2 = (double)max_dist * (double)max_dist",
                   "len2(p, q) <= thr2", "counts[2k + 1]"):
        assert phrase in words, phrase
    for phrase in ("as they were when the call was enqueued", "does not see its neighbours' rejections",
                   "A sample is a window pixel whose merged valid byte is 1", "|dr| <= radius, |dc| <= radius and (dr, dc) != (0, 0)",
                   "clipped to the context's window", "padding columns of the pitch are not pixels", "no contraction",
                   "A NaN len2 is not within range", "at most 80", "0xFF at every other window pixel", "support < min_neighbours is rejected",
                   "merged valid byte becomes 0", "0x7FC00000", "intersection_points entry becomes 0", "residual, c_p_map and per-axis planes stay",
                   "min_neighbours == 0 writes the support plane and changes nothing else", "number of samples of view first_view + k on entry",
                   "counts == NULL leaves the call asynchronous", "second pass over the result of the first",
                   "sl3d_run, sl3d_triangulate and sl3d_triangulate_subpixel", "before anything is allocated or enqueued",
                   "radius outside 1..SL3D_FILTER_MAX_RADIUS", "max_dist NaN or <= 0 (+infinity is allowed)", "sl3d_compact_views",
                   "sl3d_run_clouds", "no group entry point and no shim call", "SL3D_FLAG_REPAIR_PERIODS"):
        assert phrase in text, phrase
    g = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int\s+sl3d_get_support", _header(), flags=re.S)
    gtext = " ".join(g.group(1).replace("*", " ").split())
    assert "SL3D_E_STATE: no filter call has written this view" in gtext and "stride < width" in gtext


def test_the_header_is_plain_c(tmp_path):
    """C99 with nothing but the standard headers and sl3d.h, which it includes itself."""
    src = tmp_path / "inc.c"
    src.write_text('#include "sl3d_filter.h"\nint main(void) { uint32_t c[2]; uint8_t s[SL3D_FILTER_MAX_RADIUS];\n'
                   '    return sl3d_filter_outliers(0, 0, 1, SL3D_FILTER_MAX_RADIUS, 1.5f, 8, c) == SL3D_OK && sl3d_get_support(0, 0, s, 4) == SL3D_OK; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                           "-o", str(tmp_path / "inc.o")])
    subprocess.check_call(["cc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def test_the_version_is_at_least_0_22(scanner_mod):
    m = re.search(r'#define\s+SL3D_VERSION_STRING\s+"0\.(\d+)\.', _header("sl3d.h"))
    assert m and int(m.group(1)) >= 22
    pkg = __import__("importlib").import_module("3dscan_amd")
    assert int(pkg.__version__.split(".")[1]) >= 22
    assert int(scanner_mod.load_library().sl3d_version().decode().split(".")[1]) >= 22


def test_the_binding_has_the_rows_and_the_methods(scanner_mod):
    assert scanner_mod.FILTER_SYMBOLS == ("sl3d_filter_outliers", "sl3d_get_support")
    assert not set(scanner_mod.FILTER_SYMBOLS) & (set(scanner_mod.ABI_SYMBOLS) | set(scanner_mod.FUSE_SYMBOLS))
    L = scanner_mod.load_library()
    lib = C.CDLL(scanner_mod.LIB_PATH)
    assert all(hasattr(lib, name) for name in scanner_mod.FILTER_SYMBOLS)
    # the header's parameters, position by position: int / float / size_t scalars, pointers
    assert L.sl3d_filter_outliers.restype is C.c_int and L.sl3d_get_support.restype is C.c_int
    assert L.sl3d_filter_outliers.argtypes == [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.POINTER(C.c_uint)]
    assert L.sl3d_get_support.argtypes == [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]
    p = inspect.signature(scanner_mod.Scanner.filter_outliers).parameters
    assert list(p) == ["self", "radius", "max_dist", "min_neighbours", "first_view", "n_views", "counts"]
    assert p["first_view"].default == 0 and p["n_views"].default == 1 and p["counts"].default is True
    p = inspect.signature(scanner_mod.Scanner.support).parameters
    assert list(p) == ["self", "view"] and p["view"].default == 0
