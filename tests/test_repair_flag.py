"""CPU tests of SL3D_FLAG_REPAIR_PERIODS: the value in the header and in the binding, that the bit collides with no other flag,
the Scanner argument, and that a flagged sl3d_create without a device fails as any other does."""
import ctypes
import inspect
import os
import re

from conftest import ROOT


def _header():
    return open(os.path.join(ROOT, "include", "sl3d.h")).read()


def _flags_enum():
    """{name: value} of enum sl3d_flags, parsed from include/sl3d.h with the comments removed."""
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
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
    assert flags["SL3D_FLAG_REPAIR_PERIODS"] == 256
    assert re.search(r"SL3D_FLAG_REPAIR_PERIODS\s*=\s*256u\b", _header())
    assert scanner_mod.SL3D_FLAG_REPAIR_PERIODS == 256


def test_the_bit_collides_with_no_other_flag(scanner_mod):
    flags = _flags_enum()
    assert len(flags) >= 8
    seen = 0
    for name, value in flags.items():
        assert value and value & (value - 1) == 0, (name, "a flag is one bit")
        assert not seen & value, (name, "two flags share a bit")
        seen |= value
    for name, value in flags.items():                       # the binding's copies are the header's
        assert getattr(scanner_mod, name) == value, name


def test_the_flags_comment_states_the_contract():
    """The radius, what stays with the staged call, and the group's refusal are part of the interface: the header says them."""
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*SL3D_FLAG_REPAIR_PERIODS\s*=", _header(), flags=re.S)
    assert m
    text = " ".join(m.group(1).replace("*", " ").split())
    for phrase in ("radius is fixed at 4", "sl3d_repair_periods", "counts", "n_gray == 0", "sl3d_group_create refuses", "SL3D_FLAG_SUBPIXEL",
                   "sl3d_run + sl3d_compact_views", "bit for bit"):
        assert phrase in text, phrase


def test_scanner_accepts_repaired(scanner_mod):
    p = inspect.signature(scanner_mod.Scanner.__init__).parameters
    assert "repaired" in p and p["repaired"].default is False
    assert "repair_periods" not in p, "that name is the method"
    assert callable(scanner_mod.Scanner.repair_periods)
    assert "SL3D_FLAG_REPAIR_PERIODS" in (scanner_mod.Scanner.__init__.__doc__ or "")


def test_a_group_refuses_the_flag_and_says_why(scanner_mod):
    """The refusal comes before any device is touched: a neighbourhood is clipped to its context's window, so a row stripe would decide
    differently from the whole frame near its seams."""
    R = scanner_mod.SL3D_FLAG_REPAIR_PERIODS
    for flags in (R, R | scanner_mod.SL3D_FLAG_SUBPIXEL, R | scanner_mod.SL3D_FLAG_KEEP_STAGES):
        try:
            scanner_mod.Group(64, 32, 64, 64, 3, 3, 8, 8, devices=[0, 0], flags=flags)
        except scanner_mod.Sl3dError as e:
            text = str(e)
        else:
            raise AssertionError("sl3d_group_create accepted SL3D_FLAG_REPAIR_PERIODS")
        assert scanner_mod.load_library().sl3d_strerror(-5).decode() in text
        assert "SL3D_FLAG_REPAIR_PERIODS" in text and "clipped" in text and "window" in text and "seam" in text, text


def test_flagged_create_without_a_device_is_no_device(scanner_mod):
    L = scanner_mod.load_library()
    R, S, K = scanner_mod.SL3D_FLAG_REPAIR_PERIODS, scanner_mod.SL3D_FLAG_SUBPIXEL, scanner_mod.SL3D_FLAG_KEEP_STAGES
    device = False
    for flags in (R, R | S, R | K, R | S | K):
        h = ctypes.c_void_p()
        cfg = scanner_mod.Config(64, 32, 0, 0, 0, 0, 64, 64, 3, 3, 3, 8, 8, 0, 0, 1, 0, flags, None)
        rc = L.sl3d_create(ctypes.byref(cfg), ctypes.byref(h))
        if rc == 0:  # a GPU is present: the flagged context exists; tests/test_gpu_repair_fused.py takes it from here
            device = True
            assert h.value
            L.sl3d_destroy(h)
        else:
            assert not device and rc == -2 and h.value is None
    if device:
        with scanner_mod.Scanner(64, 32, 64, 64, 3, 3, 8, 8, repaired=True) as sc:
            assert sc.cfg.flags & R
    else:
        try:
            scanner_mod.Scanner(64, 32, 64, 64, 3, 3, 8, 8, repaired=True)
        except scanner_mod.Sl3dError:
            pass
        else:
            raise AssertionError("a flagged Scanner without a device must raise")
