"""CPU tests of SL3D_FLAG_SUBPIXEL: the value in the header and in the binding, that the bit collides with no other flag,
the Scanner argument, and that a flagged sl3d_create without a device fails as any other does."""
import ctypes
import inspect
import os
import re

import pytest

from conftest import ROOT


def _flags_enum():
    """{name: value} of enum sl3d_flags, parsed from include/sl3d.h with the comments removed."""
    text = open(os.path.join(ROOT, "include", "sl3d.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    body = re.search(r"enum\s+sl3d_flags\s*\{(.*?)\}", text, flags=re.S).group(1)
    out = {}
    for item in body.split(","):
        item = item.strip()
        if item:
            name, value = (s.strip() for s in item.split("="))
            out[name] = int(value.rstrip("uU"), 0)
    return out


def test_the_header_and_the_binding_define_the_flag(scanner_mod):
    flags = _flags_enum()
    assert flags["SL3D_FLAG_SUBPIXEL"] == 128
    assert re.search(r"SL3D_FLAG_SUBPIXEL\s*=\s*128u\b", open(os.path.join(ROOT, "include", "sl3d.h")).read())
    assert scanner_mod.SL3D_FLAG_SUBPIXEL == 128


def test_the_bit_collides_with_no_other_flag(scanner_mod):
    flags = _flags_enum()
    assert len(flags) >= 7
    seen = 0
    for name, value in flags.items():
        assert value and value & (value - 1) == 0, (name, "a flag is one bit")
        assert not seen & value, (name, "two flags share a bit")
        seen |= value
    for name, value in flags.items():                       # the binding's copies are the header's
        assert getattr(scanner_mod, name) == value, name


def test_scanner_accepts_subpixel(scanner_mod):
    p = inspect.signature(scanner_mod.Scanner.__init__).parameters
    assert "subpixel" in p and p["subpixel"].default is False
    assert "run" in (scanner_mod.Scanner.residuals.__doc__ or "")


def test_flagged_create_without_a_device_is_no_device(scanner_mod):
    L = scanner_mod.load_library()
    for flags in (scanner_mod.SL3D_FLAG_SUBPIXEL, scanner_mod.SL3D_FLAG_SUBPIXEL | scanner_mod.SL3D_FLAG_KEEP_STAGES):
        h = ctypes.c_void_p()
        cfg = scanner_mod.Config(64, 32, 0, 0, 0, 0, 64, 64, 3, 3, 3, 8, 8, 0, 0, 1, 0, flags, None)
        rc = L.sl3d_create(ctypes.byref(cfg), ctypes.byref(h))
        if rc == 0:  # a GPU is present: fine, clean up
            L.sl3d_destroy(h)
            pytest.skip("a HIP device is present")
        assert rc == -2 and h.value is None
    with pytest.raises(scanner_mod.Sl3dError):
        scanner_mod.Scanner(64, 32, 64, 64, 3, 3, 8, 8, subpixel=True)
