"""What the GPU tests of sl3d_repair_periods do around one call (shared by tests/test_gpu_period_repair.py, tests/test_gpu_repair_edges.py and
tests/test_gpu_direct_gray.py): the stage planes of an axis, and one call against the NumPy restatement (tests/period_repair_reference.py)
applied to the very planes downloaded before it."""
import numpy as np

import period_repair_reference as PR


def bits(a):
    return a.view(np.uint32)


def stages34(sc, view=0):
    for a in (0, 1):
        sc.compute_wrapped_phase(a, view)
    for a in (0, 1):
        sc.unwrap_phase(a, view)


def planes(sc, axis, view=0):
    return sc.code(axis, view), sc.wrapped_phase(axis, view), sc.unwrapped_phase(axis, view), sc.valid_map(axis, view)


def assert_same_planes(got, want, what):
    for g, w, n in zip(got, want, ("code", "wrapped", "unwrapped", "valid")):
        assert np.array_equal(g.view(np.uint32) if g.dtype == np.float32 else g, w.view(np.uint32) if w.dtype == np.float32 else w), (what, n)


def check_pass(sc, n_gray, axis, radius, view=0, what=""):
    """One repair_periods call against the restatement applied to the planes downloaded before it: code and absolute phase bit for bit
    (floats as uint32), the counts equal, the wrapped phase, the valid map and the other axis untouched.  n_gray: the Gray planes of the
    axis.  Returns the counts."""
    before = planes(sc, axis, view)
    other = planes(sc, 1 - axis, view)
    want_code, want_unw, rep, unrep = PR.repair_periods(*before, axis, radius, n_gray)
    counts = sc.repair_periods(axis, radius, view)
    code, wrapped, unw, valid = planes(sc, axis, view)
    bad = np.argwhere(code != want_code)
    assert bad.size == 0, (what, axis, radius, "code", bad[:5].tolist())
    assert np.array_equal(bits(unw), bits(want_unw)), (what, axis, radius, "unwrapped")
    assert counts == (rep, unrep), (what, axis, radius, counts, (rep, unrep))
    assert np.array_equal(bits(wrapped), bits(before[1])) and np.array_equal(valid, before[3]), (what, axis, radius, "wrapped / valid touched")
    assert_same_planes(planes(sc, 1 - axis, view), other, (what, "the other axis"))
    return rep, unrep
