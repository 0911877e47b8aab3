"""CPU tests of SL3D_FLAG_ANCHOR_PERIODS: the value in the header and in the binding, that the bit collides with no other flag,
what the header's comment promises, the Scanner argument, and the refusals sl3d_create and sl3d_group_create make before a device is
touched -- the flag without SL3D_FLAG_SUBPIXEL, and together with SL3D_FLAG_REPAIR_PERIODS."""
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


def test_the_header_and_the_binding_define_the_flag(scanner_mod):
    flags = _flags_enum()
    assert flags["SL3D_FLAG_ANCHOR_PERIODS"] == 512
    assert re.search(r"SL3D_FLAG_ANCHOR_PERIODS\s*=\s*512u\b", _header())
    assert scanner_mod.SL3D_FLAG_ANCHOR_PERIODS == 512
    names = list(flags)
    assert names.index("SL3D_FLAG_ANCHOR_PERIODS") == names.index("SL3D_FLAG_REPAIR_PERIODS") + 1


def test_the_bit_collides_with_no_other_flag(scanner_mod):
    flags = _flags_enum()
    assert len(flags) >= 9
    seen = 0
    for name, value in flags.items():
        assert value and value & (value - 1) == 0, (name, "a flag is one bit")
        assert not seen & value, (name, "two flags share a bit")
        seen |= value
    for name, value in flags.items():                       # the binding's copies are the header's
        assert getattr(scanner_mod, name) == value, name


def test_the_flags_comment_states_the_contract():
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*SL3D_FLAG_ANCHOR_PERIODS\s*=", _header(), flags=re.S)
    assert m
    text = " ".join(m.group(1).replace("*", " ").split())
    for phrase in ("SL3D_FLAG_SUBPIXEL", "sl3d_repair_periods", "validity", "bit for bit", "SL3D_FLAG_REPAIR_PERIODS", "0.15915494309189535", "n_gray > 0",
                   "sl3d_get_correspondences_subpixel", "c_p_map"):
        assert phrase in text, phrase


def test_scanner_accepts_anchored(scanner_mod):
    p = inspect.signature(scanner_mod.Scanner.__init__).parameters
    assert "anchored" in p and p["anchored"].default is False
    assert "SL3D_FLAG_ANCHOR_PERIODS" in (scanner_mod.Scanner.__init__.__doc__ or "")


def test_create_refuses_the_flag_alone_and_with_the_repair(scanner_mod):
    """SL3D_E_UNSUPPORTED whether or not a device is present: the decision is made before one is touched."""
    A, S, R, K = scanner_mod.SL3D_FLAG_ANCHOR_PERIODS, scanner_mod.SL3D_FLAG_SUBPIXEL, scanner_mod.SL3D_FLAG_REPAIR_PERIODS, scanner_mod.SL3D_FLAG_KEEP_STAGES
    unsupported = scanner_mod.load_library().sl3d_strerror(-5).decode()
    assert unsupported == "unsupported configuration"
    for flags in (A, A | K):
        rc, h, text = _create(scanner_mod, flags)
        assert rc == -5 and h is None, flags
        assert "SL3D_FLAG_ANCHOR_PERIODS" in text and "SL3D_FLAG_SUBPIXEL" in text and "add SL3D_FLAG_SUBPIXEL" in text, text
    for flags in (A | R | S, A | R | S | K):
        rc, h, text = _create(scanner_mod, flags)
        assert rc == -5 and h is None, flags
        assert "SL3D_FLAG_ANCHOR_PERIODS" in text and "SL3D_FLAG_REPAIR_PERIODS" in text and "choose one" in text, text
    rc, _, text = _create(scanner_mod, A | R)                 # (both wrong: the first refusal)
    assert rc == -5 and "add SL3D_FLAG_SUBPIXEL" in text
    try:
        scanner_mod.Scanner(64, 32, 64, 64, 3, 3, 8, 8, anchored=True)
    except scanner_mod.Sl3dError as e:
        assert unsupported in str(e) and "SL3D_FLAG_SUBPIXEL" in str(e)
    else:
        raise AssertionError("Scanner(anchored=True) without subpixel=True must raise")


def test_supported_combinations_reach_the_device(scanner_mod):
    """512 | 128 and 512 | 128 | 1: no device -> SL3D_E_NO_DEVICE as for any other create; a device -> a context."""
    A, S, K = scanner_mod.SL3D_FLAG_ANCHOR_PERIODS, scanner_mod.SL3D_FLAG_SUBPIXEL, scanner_mod.SL3D_FLAG_KEEP_STAGES
    device = False
    for flags in (A | S, A | S | K):
        rc, h, _ = _create(scanner_mod, flags)
        if rc == 0:                                          # a GPU is present: tests/test_gpu_anchor.py takes it from here
            device = True
            assert h
        else:
            assert not device and rc == -2 and h is None
    if device:
        with scanner_mod.Scanner(64, 32, 64, 64, 3, 3, 8, 8, subpixel=True, anchored=True) as sc:
            assert sc.cfg.flags & A and sc.cfg.flags & S
    else:
        try:
            scanner_mod.Scanner(64, 32, 64, 64, 3, 3, 8, 8, subpixel=True, anchored=True)
        except scanner_mod.Sl3dError:
            pass
        else:
            raise AssertionError("a flagged Scanner without a device must raise")


def test_a_group_refuses_what_create_refuses(scanner_mod):
    A, S, R = scanner_mod.SL3D_FLAG_ANCHOR_PERIODS, scanner_mod.SL3D_FLAG_SUBPIXEL, scanner_mod.SL3D_FLAG_REPAIR_PERIODS
    for flags, words in ((A, ("SL3D_FLAG_ANCHOR_PERIODS", "add SL3D_FLAG_SUBPIXEL")), (A | S | R, ("SL3D_FLAG_ANCHOR_PERIODS", "SL3D_FLAG_REPAIR_PERIODS", "choose one"))):
        try:
            scanner_mod.Group(64, 32, 64, 64, 3, 3, 8, 8, devices=[0, 0], flags=flags)
        except scanner_mod.Sl3dError as e:
            text = str(e)
        else:
            raise AssertionError("sl3d_group_create accepted the flags")
        assert scanner_mod.load_library().sl3d_strerror(-5).decode() in text
        assert "group_create" in text and all(w in text for w in words), text
