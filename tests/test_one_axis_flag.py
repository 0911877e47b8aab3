"""CPU tests of SL3D_FLAG_ONLY_VERTICAL / SL3D_FLAG_ONLY_HORIZONTAL: the values in the header and in the binding, that the bits
collide with no other flag, what the header's comment promises, the Scanner argument, and every refusal sl3d_create and sl3d_group_create
make before a device is touched -- both flags, either without SL3D_FLAG_SUBPIXEL, either with SL3D_FLAG_REPAIR_PERIODS."""
import ctypes
import inspect
import os
import re

import pytest

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


def _create(scanner_mod, flags):
    """(status, handle value, text of the refusal) of sl3d_create on a small configuration with these flags."""
    L = scanner_mod.load_library()
    h = ctypes.c_void_p()
    cfg = scanner_mod.Config(64, 32, 0, 0, 0, 0, 64, 64, 3, 3, 3, 8, 8, 0, 0, 1, 0, flags, None)
    rc = L.sl3d_create(ctypes.byref(cfg), ctypes.byref(h))
    text = L.sl3d_last_error(None).decode() if rc else ""
    value = h.value
    if rc == 0:
        L.sl3d_destroy(h)
    return rc, value, text


def _refusals(m):
    """(flags, words the text must hold) of every refused combination."""
    V, H, S, R, A, K = (m.SL3D_FLAG_ONLY_VERTICAL, m.SL3D_FLAG_ONLY_HORIZONTAL, m.SL3D_FLAG_SUBPIXEL, m.SL3D_FLAG_REPAIR_PERIODS, m.SL3D_FLAG_ANCHOR_PERIODS,
                        m.SL3D_FLAG_KEEP_STAGES)
    both = ("SL3D_FLAG_ONLY_VERTICAL", "SL3D_FLAG_ONLY_HORIZONTAL", "choose one")
    return [(V | H | S, both), (V | H | S | K, both), (V | H | S | A, both), (V | H, both),
            (V, ("SL3D_FLAG_ONLY_VERTICAL", "add SL3D_FLAG_SUBPIXEL")), (V | K, ("SL3D_FLAG_ONLY_VERTICAL", "add SL3D_FLAG_SUBPIXEL")),
            (H, ("SL3D_FLAG_ONLY_HORIZONTAL", "add SL3D_FLAG_SUBPIXEL")), (H | K, ("SL3D_FLAG_ONLY_HORIZONTAL", "add SL3D_FLAG_SUBPIXEL")),
            (V | S | R, ("SL3D_FLAG_ONLY_VERTICAL", "SL3D_FLAG_REPAIR_PERIODS", "no one-axis form")),
            (V | S | R | K, ("SL3D_FLAG_ONLY_VERTICAL", "SL3D_FLAG_REPAIR_PERIODS", "no one-axis form")),
            (H | S | R, ("SL3D_FLAG_ONLY_HORIZONTAL", "SL3D_FLAG_REPAIR_PERIODS", "no one-axis form"))]


def test_the_header_and_the_binding_define_the_flags(scanner_mod):
    flags = _flags_enum()
    assert flags["SL3D_FLAG_ONLY_VERTICAL"] == 1024 and flags["SL3D_FLAG_ONLY_HORIZONTAL"] == 2048
    assert re.search(r"SL3D_FLAG_ONLY_VERTICAL\s*=\s*1024u\b", _header()) and re.search(r"SL3D_FLAG_ONLY_HORIZONTAL\s*=\s*2048u\b", _header())
    assert scanner_mod.SL3D_FLAG_ONLY_VERTICAL == 1024 and scanner_mod.SL3D_FLAG_ONLY_HORIZONTAL == 2048
    names = list(flags)
    assert names.index("SL3D_FLAG_ONLY_VERTICAL") == names.index("SL3D_FLAG_ANCHOR_PERIODS") + 1
    assert names.index("SL3D_FLAG_ONLY_HORIZONTAL") == names.index("SL3D_FLAG_ONLY_VERTICAL") + 1
    assert re.search(r'#define\s+SL3D_VERSION_STRING\s+"0\.(19|[2-9]\d)\.', _header())


def test_the_bits_collide_with_no_other_flag(scanner_mod):
    flags = _flags_enum()
    assert len(flags) >= 11
    seen = 0
    for name, value in flags.items():
        assert value and value & (value - 1) == 0, (name, "a flag is one bit")
        assert not seen & value, (name, "two flags share a bit")
        seen |= value
    for name, value in flags.items():                       # the binding's copies are the header's
        assert getattr(scanner_mod, name) == value, name


def test_the_flags_comment_states_the_contract():
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*SL3D_FLAG_ONLY_VERTICAL\s*=", _header(), flags=re.S)
    assert m
    text = " ".join(m.group(1).replace("*", " ").split())
    for phrase in ("SL3D_FLAG_SUBPIXEL", "SL3D_FLAG_REPAIR_PERIODS", "both flags together", "sl3d_set_calibration", "distortion coefficient", "not plain",
                   "a curve and not a line", "no frame of the other axis is read", "-1", "sl3d_get_residuals", "SL3D_E_UNSUPPORTED", "sl3d_triangulate_subpixel",
                   "sl3d_get_correspondences_subpixel", "NaN", "sl3d_run_clouds", "sl3d_triangulate (", "sl3d_set_masks_modulated", "sl3d_group_create",
                   "t = fma(f, (s - c)", "(1.0 / f), c)", "det == 0", "k_one_axis", "bit for bit"):
        assert phrase in text, phrase


def test_scanner_accepts_only_axis(scanner_mod):
    p = inspect.signature(scanner_mod.Scanner.__init__).parameters
    assert "only_axis" in p and p["only_axis"].default is None
    doc = scanner_mod.Scanner.__init__.__doc__ or ""
    assert "SL3D_FLAG_ONLY_VERTICAL" in doc and "SL3D_FLAG_ONLY_HORIZONTAL" in doc
    with pytest.raises(ValueError):
        scanner_mod.Scanner(64, 32, 64, 64, 3, 3, 8, 8, subpixel=True, only_axis=2)


def test_create_refuses_before_a_device_is_touched(scanner_mod):
    """SL3D_E_UNSUPPORTED whether or not a device is present: the decision is made before one is touched."""
    unsupported = scanner_mod.load_library().sl3d_strerror(-5).decode()
    assert unsupported == "unsupported configuration"
    for flags, words in _refusals(scanner_mod):
        rc, h, text = _create(scanner_mod, flags)
        assert rc == -5 and h is None, flags
        assert all(w in text for w in words), (flags, text)
    for axis, name in ((0, "SL3D_FLAG_ONLY_VERTICAL"), (1, "SL3D_FLAG_ONLY_HORIZONTAL")):
        with pytest.raises(scanner_mod.Sl3dError) as e:
            scanner_mod.Scanner(64, 32, 64, 64, 3, 3, 8, 8, only_axis=axis)
        assert unsupported in str(e.value) and name in str(e.value) and "add SL3D_FLAG_SUBPIXEL" in str(e.value)
        with pytest.raises(scanner_mod.Sl3dError) as e:
            scanner_mod.Scanner(64, 32, 64, 64, 3, 3, 8, 8, subpixel=True, repaired=True, only_axis=axis)
        assert name in str(e.value) and "SL3D_FLAG_REPAIR_PERIODS" in str(e.value)


def test_supported_combinations_reach_the_device(scanner_mod):
    """A flag with SUBPIXEL, with or without KEEP_STAGES and ANCHOR_PERIODS: no device -> SL3D_E_NO_DEVICE as for any other create."""
    m = scanner_mod
    device = False
    for one in (m.SL3D_FLAG_ONLY_VERTICAL, m.SL3D_FLAG_ONLY_HORIZONTAL):
        for extra in (0, m.SL3D_FLAG_KEEP_STAGES, m.SL3D_FLAG_ANCHOR_PERIODS, m.SL3D_FLAG_KEEP_STAGES | m.SL3D_FLAG_ANCHOR_PERIODS):
            rc, h, _ = _create(m, one | m.SL3D_FLAG_SUBPIXEL | extra)
            if rc == 0:                                      # a GPU is present: tests/test_gpu_one_axis.py takes it from here
                device = True
                assert h
            else:
                assert not device and rc == -2 and h is None
    if device:
        with m.Scanner(64, 32, 64, 64, 3, 3, 8, 8, subpixel=True, only_axis=1) as sc:
            assert sc.cfg.flags & m.SL3D_FLAG_ONLY_HORIZONTAL and not sc.cfg.flags & m.SL3D_FLAG_ONLY_VERTICAL
    else:
        with pytest.raises(m.Sl3dError):
            m.Scanner(64, 32, 64, 64, 3, 3, 8, 8, subpixel=True, only_axis=0)


def test_a_group_refuses_what_create_refuses(scanner_mod):
    for flags, words in _refusals(scanner_mod):
        with pytest.raises(scanner_mod.Sl3dError) as e:
            scanner_mod.Group(64, 32, 64, 64, 3, 3, 8, 8, devices=[0, 0], flags=flags)
        text = str(e.value)
        assert scanner_mod.load_library().sl3d_strerror(-5).decode() in text
        assert "group_create" in text and all(w in text for w in words), (flags, text)
