"""CPU tests of SL3D_FLAG_DIRECT_GRAY: the value in the header and in the binding, that the bit collides with no other flag,
what the header's comment promises, the Scanner argument, and every refusal sl3d_create and sl3d_group_create make before a device is
touched -- the flag without SL3D_FLAG_SUBPIXEL, the flag with SL3D_FLAG_REPAIR_PERIODS."""
import ctypes
import inspect
import os
import re

import numpy as np
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
    D, S, R, A, K, V, H, E = (m.SL3D_FLAG_DIRECT_GRAY, m.SL3D_FLAG_SUBPIXEL, m.SL3D_FLAG_REPAIR_PERIODS, m.SL3D_FLAG_ANCHOR_PERIODS, m.SL3D_FLAG_KEEP_STAGES,
                              m.SL3D_FLAG_ONLY_VERTICAL, m.SL3D_FLAG_ONLY_HORIZONTAL, m.SL3D_FLAG_EAGER_MASK)
    alone = ("SL3D_FLAG_DIRECT_GRAY", "add SL3D_FLAG_SUBPIXEL")
    repair = ("SL3D_FLAG_DIRECT_GRAY", "SL3D_FLAG_REPAIR_PERIODS", "no direct form")
    return [(D, alone), (D | K, alone), (D | E, alone), (D | R, alone), (D | R | K, alone),
            (D | S | R, repair), (D | S | R | K, repair)]


def _supported(m):
    D, S, A, K, V, H, E, L = (m.SL3D_FLAG_DIRECT_GRAY, m.SL3D_FLAG_SUBPIXEL, m.SL3D_FLAG_ANCHOR_PERIODS, m.SL3D_FLAG_KEEP_STAGES, m.SL3D_FLAG_ONLY_VERTICAL,
                              m.SL3D_FLAG_ONLY_HORIZONTAL, m.SL3D_FLAG_EAGER_MASK, m.SL3D_FLAG_SERIAL_LAUNCHES)
    return [D | S | extra | axis for extra in (0, K, A, K | A, E, L, K | A | E | L) for axis in (0, V, H)]


def test_the_header_and_the_binding_define_the_flag(scanner_mod):
    flags = _flags_enum()
    assert flags["SL3D_FLAG_DIRECT_GRAY"] == 4096
    assert re.search(r"SL3D_FLAG_DIRECT_GRAY\s*=\s*4096u\b", _header())
    assert scanner_mod.SL3D_FLAG_DIRECT_GRAY == 4096
    names = list(flags)
    assert names.index("SL3D_FLAG_DIRECT_GRAY") == names.index("SL3D_FLAG_ONLY_HORIZONTAL") + 1 == len(names) - 1, "the last member, after ONLY_HORIZONTAL"
    m = re.search(r'#define\s+SL3D_VERSION_STRING\s+"0\.(\d+)\.', _header())
    assert m and int(m.group(1)) >= 20
    pkg = __import__("importlib").import_module("3dscan_amd")
    assert int(pkg.__version__.split(".")[1]) >= 20
    assert int(scanner_mod.load_library().sl3d_version().decode().split(".")[1]) >= 20


def test_the_bit_collides_with_no_other_flag(scanner_mod):
    flags = _flags_enum()
    assert len(flags) >= 12
    seen = 0
    for name, value in flags.items():
        assert value and value & (value - 1) == 0, (name, "a flag is one bit")
        assert not seen & value, (name, "two flags share a bit")
        seen |= value
    for name, value in flags.items():                       # the binding's copies are the header's
        assert getattr(scanner_mod, name) == value, name


def test_the_flags_comment_states_the_contract():
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*SL3D_FLAG_DIRECT_GRAY\s*=", _header(), flags=re.S)
    assert m
    text = " ".join(m.group(1).replace("*", " ").split())
    for phrase in ("G_i = (2 (int)gray_i - ((int)I0 + (int)I2) >= 0)", "ties -> 1", "4/phase_unwrap.cpp:183", "fringe bytes 0 and 2 of the same axis",
                   "the same rule for n_fringe 3 and 4", "with 5 nothing is valid", "planes_per_view", "nothing reads them", "sl3d_set_frames still takes F + 2 N planes",
                   "sl3d_set_frames_range(view, axis, 0, planes, F + N, stride)", "sl3d_process_views", "sl3d_group_process_views", "may be NULL",
                   "contiguity test", "sl3d_synth_view", "sl3d_get_frames", "sl3d_copy_view", "sl3d_set_masks_modulated", "sl3d_get_modulation",
                   "k_direct_gray", '"sl3d::k_direct_gray<0, false>"', '"sl3d::k_direct_gray<2, true>"', "sl3d_camera_table_bytes_per_pixel is 0",
                   "no launch lanes", "F + N frame bytes", "bit for bit", "sl3d_unwrap_phase", "stage getters", "not the parity kernel", "sl3d_repair_periods",
                   "SL3D_E_UNSUPPORTED", "add SL3D_FLAG_SUBPIXEL", "SL3D_FLAG_REPAIR_PERIODS", "no direct form", "SL3D_FLAG_KEEP_STAGES", "SL3D_FLAG_ANCHOR_PERIODS",
                   "SL3D_FLAG_ONLY_VERTICAL", "SL3D_FLAG_EAGER_MASK", "SL3D_FLAG_SERIAL_LAUNCHES", "sl3d_run_clouds", "sl3d_group_create hands the flag",
                   "The rule is pointwise", "13 instead of 23", "26 instead of 46", "the reference has no such mode"):
        assert phrase in text, phrase
    whole = " ".join(_header().replace("*", " ").split())
    for fn in ("sl3d_run", "sl3d_unwrap_phase", "sl3d_set_frames_range", "sl3d_process_views"):   # a mention where each is declared
        at = whole.index("int %s(sl3d_ctx" % fn)
        assert "SL3D_FLAG_DIRECT_GRAY" in whole[max(0, at - 1500):at], fn


def test_scanner_accepts_direct_gray(scanner_mod):
    p = inspect.signature(scanner_mod.Scanner.__init__).parameters
    assert "direct_gray" in p and p["direct_gray"].default is False
    doc = scanner_mod.Scanner.__init__.__doc__ or ""
    assert "SL3D_FLAG_DIRECT_GRAY" in doc and "2 * gray" in doc


def test_create_refuses_before_a_device_is_touched(scanner_mod):
    """SL3D_E_UNSUPPORTED whether or not a device is present: the decision is made before one is touched."""
    unsupported = scanner_mod.load_library().sl3d_strerror(-5).decode()
    assert unsupported == "unsupported configuration"
    for flags, words in _refusals(scanner_mod):
        rc, h, text = _create(scanner_mod, flags)
        assert rc == -5 and h is None, flags
        assert all(w in text for w in words), (flags, text)
    with pytest.raises(scanner_mod.Sl3dError) as e:
        scanner_mod.Scanner(64, 32, 64, 64, 3, 3, 8, 8, direct_gray=True)
    assert unsupported in str(e.value) and "SL3D_FLAG_DIRECT_GRAY" in str(e.value) and "add SL3D_FLAG_SUBPIXEL" in str(e.value)
    with pytest.raises(scanner_mod.Sl3dError) as e:
        scanner_mod.Scanner(64, 32, 64, 64, 3, 3, 8, 8, subpixel=True, repaired=True, direct_gray=True)
    assert "SL3D_FLAG_DIRECT_GRAY" in str(e.value) and "SL3D_FLAG_REPAIR_PERIODS" in str(e.value) and "no direct form" in str(e.value)
    # the refusals of the flags it is combined with are still made
    rc, h, text = _create(scanner_mod, scanner_mod.SL3D_FLAG_DIRECT_GRAY | scanner_mod.SL3D_FLAG_SUBPIXEL | scanner_mod.SL3D_FLAG_ONLY_VERTICAL | scanner_mod.SL3D_FLAG_ONLY_HORIZONTAL)
    assert rc == -5 and h is None and "choose one" in text


def test_supported_combinations_reach_the_device(scanner_mod):
    """The flag with SUBPIXEL and any of KEEP_STAGES, ANCHOR_PERIODS, a one-axis flag, EAGER_MASK, SERIAL_LAUNCHES: no device ->
    SL3D_E_NO_DEVICE as for any other create."""
    m = scanner_mod
    device = False
    for flags in _supported(m):
        rc, h, _ = _create(m, flags)
        if rc == 0:                                      # a GPU is present: tests/test_gpu_direct_gray.py takes it from here
            device = True
            assert h
        else:
            assert not device and rc == -2 and h is None, flags
    if device:
        with m.Scanner(64, 32, 64, 64, 3, 3, 8, 8, subpixel=True, only_axis=1, direct_gray=True) as sc:
            assert sc.cfg.flags & m.SL3D_FLAG_DIRECT_GRAY and sc.cfg.flags & m.SL3D_FLAG_ONLY_HORIZONTAL
    else:
        with pytest.raises(m.Sl3dError):
            m.Scanner(64, 32, 64, 64, 3, 3, 8, 8, subpixel=True, direct_gray=True)


def test_a_group_refuses_what_create_refuses(scanner_mod):
    for flags, words in _refusals(scanner_mod):
        with pytest.raises(scanner_mod.Sl3dError) as e:
            scanner_mod.Group(64, 32, 64, 64, 3, 3, 8, 8, devices=[0, 0], flags=flags)
        text = str(e.value)
        assert scanner_mod.load_library().sl3d_strerror(-5).decode() in text
        assert "group_create" in text and all(w in text for w in words), (flags, text)


def test_process_views_takes_missing_planes_as_null_pointers(scanner_mod):
    """The binding's part of "the pointers of the inverse planes may be NULL": a per-view list with None goes down as NULL pointers, a 4-D
    array as it always did (no device needed: the call is intercepted)."""
    class Probe(scanner_mod._Handle):
        W, H = 8, 4

        def _call(self, name, n, ptrs, stride, xyz, valid):
            self.seen = (name, n, [p for p in ptrs], stride)

    planes = [np.full((4, 8), i, np.uint8) for i in range(3)]
    p = Probe.__new__(Probe)
    xyz, valid = p._process_views([[planes[0], None, planes[2]], [None, planes[1], None]], None, None)
    name, n, ptrs, stride = p.seen
    assert (name, n, stride) == ("process_views", 2, 8) and xyz.shape == (2, 4, 8, 3) and valid.shape == (2, 4, 8)
    assert [q is None for q in ptrs] == [False, True, False, True, False, True]
    stack = np.zeros((2, 3, 4, 8), np.uint8)
    p._process_views(stack, None, None)
    name, n, ptrs, stride = p.seen
    assert n == 2 and stride == 8 and ptrs == [stack[v, q].ctypes.data for v in range(2) for q in range(3)]
