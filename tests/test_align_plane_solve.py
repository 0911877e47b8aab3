"""CPU tests of the point-to-plane solve through the library's own entry point (sl3d_align_plane_solve: host only, no context, no GPU)
against the restatement (tests/align_plane_reference.solve) and against the truth.

Pairs that are exactly rigid -- sources on integer points, targets their rotation about an axis point by a Pythagorean angle or a
quarter turn, normals on a grid of 2^-6 -- give integer features whose residual c A + s B + u nx + w nz + D vanishes for the true
motion: the quadratic form has its minimum 0 there, and the solve must find it from a start 3 degrees and 180 units off.  The bar is the one
tests/test_align_solve.py uses, 1e-9 relative, and is derived the same way: both sides round each moment once, the same eight Gauss-Newton
steps of some hundred double operations follow, and Gauss-Newton converges quadratically on a zero-residual problem -- after eight steps from
that start the iteration error is far below the rounding (2^-53 a step, conditioning of (I - R) t = d at most 3 for the angles used).  Then
pair words that add past 2^63, every degenerate condition from crafted small-integer words, and the refusals."""
import ctypes as C
import math

import numpy as np
import pytest

import align_plane_reference as PR

REL = 1e-9
ANGLES = {"3-4-5": (3, 4, 5), "minus 3-4-5": (3, -4, 5), "5-12-13": (5, 12, 13), "obtuse 8-15-17": (-8, 15, 17), "quarter": (0, 1, 1),
          "minus quarter": (0, -1, 1)}
RNG = 65536.0                                                               # Qp = 1: a length is its own fixed-point value


def _rigid_features(cn, sn, den, t, n, seed, span=1 << 9):
    """n exact feature rows (A, B, nx, nz, D) * 64 as integers, nx and nz in units of 2^-6: sources a = t + den * d, targets R (a - t) + t"""
    rng = np.random.default_rng(seed)
    d = rng.integers(-span, span, (n, 2)) * den
    a = d + np.array(t)
    b = np.stack([(cn * d[:, 0] - sn * d[:, 1]) // den, (sn * d[:, 0] + cn * d[:, 1]) // den], axis=1) + np.array(t)
    nrm = rng.integers(-64, 65, (n, 2))                                      # (nx, nz) * 64; ny plays no part: p.y = q.y
    A = nrm[:, 0] * a[:, 0] + nrm[:, 1] * a[:, 1]
    B = nrm[:, 1] * a[:, 0] - nrm[:, 0] * a[:, 1]
    D = -(nrm[:, 0] * b[:, 0] + nrm[:, 1] * b[:, 1])
    return np.stack([A, B, nrm[:, 0], nrm[:, 1], D], axis=1)


def _words(f, scale_lengths=1, sources=None, lost=0):
    """the 18 words of integer feature rows f (n, 5): lengths as given * scale_lengths, the normals' columns (units of 2^-6) times 2^10"""
    cols = [[int(v) * scale_lengths for v in f[:, 0]], [int(v) * scale_lengths for v in f[:, 1]], [int(v) << 10 for v in f[:, 2]],
            [int(v) << 10 for v in f[:, 3]], [int(v) * scale_lengths for v in f[:, 4]]]
    n = len(f)
    return [n] + [sum(x * y for x, y in zip(cols[i], cols[j])) for i in range(5) for j in range(i, 5)] + [n + lost if sources is None else sources, lost]


def _close(got, want, rel=REL):
    return abs(got - want) <= rel * max(abs(want), 1e-300)


def _same(got, want):
    (ge, gs), (we, ws) = got, want
    assert gs["degenerate"] == ws["degenerate"] and gs["n"] == ws["n"]
    for k in range(4):
        assert _close(ge[k], we[k]) or abs(ge[k] - we[k]) <= REL, (k, ge[k], we[k])
    assert (math.isnan(gs["rms_xz"]) and math.isnan(ws["rms_xz"])) or abs(gs["rms_xz"] - ws["rms_xz"]) <= REL * max(ws["rms_xz"], 1e-6)
    assert math.isnan(gs["rms_y"]) and math.isnan(ws["rms_y"])


def _start(cn, sn, den, t, off_deg=3.0):
    a = math.atan2(sn, cn) + math.radians(off_deg)
    return np.array([math.cos(a), math.sin(a), 64.0 * t[0] + 150.0, 64.0 * t[1] - 100.0])


@pytest.mark.parametrize("name", list(ANGLES))
def test_exactly_rigid_pairs(scanner_mod, name):
    """the lengths A, B, D carry the factor 64 of the normals' grid: the solve sees the scene 64 times as large, its axis point at 64 t"""
    cn, sn, den = ANGLES[name]
    t = (1234, -777)
    f = _rigid_features(cn, sn, den, t, 500, 7)
    w = np.array([_words(f)], dtype=np.int64)
    est0 = _start(cn, sn, den, t)
    got, want = scanner_mod.align_plane_solve(w, RNG, 0.0, 0.0, est0), PR.solve(w, RNG, 0.0, 0.0, est0)
    _same(got, want)
    est, stats = got
    assert not stats["degenerate"] and stats["n"] == 500
    assert abs(est[0] - cn / den) <= REL and abs(est[1] - sn / den) <= REL
    assert _close(est[2], 64.0 * t[0]) and _close(est[3], 64.0 * t[1])
    assert stats["rms_xz"] <= 1e-6 * np.abs(f).max()                          # a rigid motion leaves no residual: sqrt of the moments' rounding


def test_words_added_past_2_63(scanner_mod):
    cn, sn, den, t = 5, 12, 13, (-40, 90)
    f = _rigid_features(cn, sn, den, t, 300, 11)
    f[:, 4] += np.random.default_rng(12).integers(-3, 4, 300)                # not rigid any more: a residual
    one = np.array([_words(f, sources=400, lost=7)], dtype=np.int64)
    three = np.array([_words(f[:100], sources=150, lost=3), _words(f[100:101], sources=50, lost=0), _words(f[101:], sources=200, lost=4)], dtype=np.int64)
    assert np.array_equal(three.sum(axis=0), one[0])
    est0 = _start(cn, sn, den, t)
    e1, s1 = scanner_mod.align_plane_solve(one, RNG, 0.0, 0.0, est0)
    e3, s3 = scanner_mod.align_plane_solve(three, RNG, 0.0, 0.0, est0)
    assert np.array_equal(e1, e3) and s1["n"] == s3["n"] == 300 and s1["rms_xz"] == s3["rms_xz"] > 0.0 and not s1["degenerate"]
    huge = (1 << 62) + 12345                                                 # rows whose int64 sum would wrap: the words are added in 128 bits
    wrap = np.array([one[0] + huge, one[0] * 0 - huge, one[0] * 0 + huge, one[0] * 0 - huge], dtype=np.int64)
    e4, s4 = scanner_mod.align_plane_solve(wrap, RNG, 0.0, 0.0, est0)
    assert np.array_equal(e1, e4) and s1["rms_xz"] == s4["rms_xz"]
    _same((e3, s3), PR.solve(three, RNG, 0.0, 0.0, est0))
    _same((e4, s4), PR.solve(wrap, RNG, 0.0, 0.0, est0))
    # words next to the 2^61 bound: 2^25 - 4 pairs with features next to 2^18
    m = ((1 << 25) - 4) // 4
    lim = (1 << 18) - 1
    big = np.array([[lim, -lim + 2, 64, 0, lim - 5], [-lim, lim, 0, 64, -lim], [lim - 7, lim, -64, 64, lim], [-lim + 1, -lim, 45, -45, 9]], dtype=np.int64)
    words = [m * v for v in _words(big)]
    words[0], words[16], words[17] = 4 * m, 4 * m, 0
    assert (1 << 60) < words[1] < (1 << 61)
    w = np.array([words], dtype=np.int64)
    est0 = np.array([0.6, 0.8, 1.0, 2.0])
    _same(scanner_mod.align_plane_solve(w, RNG, 0.0, 0.0, est0), PR.solve(w, RNG, 0.0, 0.0, est0))


def test_every_degenerate_condition(scanner_mod):
    est0 = np.array([0.6, 0.8, 2.5, -1.5])
    f = _rigid_features(3, 4, 5, (10, 20), 50, 3)
    one_plane = f.copy()
    one_plane[:, 2], one_plane[:, 3] = 48, -20                               # all normals equal: the nx / nz block is exactly singular
    only_x = f.copy()
    only_x[:, 3] = 0                                                         # no normal has a z component: w is unobservable
    no_normal = f.copy()
    no_normal[:, 2:4] = 0                                                    # Huu == 0: the first pivot
    revolution = f.copy()                                                    # every source on one spot p' = (7, -3), as seen from a surface of revolution
    revolution[:, 0], revolution[:, 1] = 7 * f[:, 2] - 3 * f[:, 3], 7 * f[:, 3] + 3 * f[:, 2]      # about it: theta's column lies in the span of u's and w's
    pure = f.copy()                                                          # the minimum is at theta == 0: c' == 1.0
    rng = np.random.default_rng(4)
    a = rng.integers(-500, 500, (50, 2))
    pure[:, 0], pure[:, 1] = f[:, 2] * a[:, 0] + f[:, 3] * a[:, 1], f[:, 3] * a[:, 0] - f[:, 2] * a[:, 1]
    pure[:, 4] = -pure[:, 0]
    cases = {
        "no pair": [0] * 16 + [9, 2],
        "two pairs": _words(f[:2]),
        "a single plane": _words(one_plane),
        "normals along x only": _words(only_x),
        "no normal in the plane of rotation": _words(no_normal),
        "a surface of revolution": _words(revolution),
        "a pure translation": _words(pure),
    }
    for name, words in cases.items():
        w = np.array([words], dtype=np.int64)
        start = np.array([1.0, 0.0, 2.5, -1.5]) if name == "a pure translation" else est0
        est, stats = scanner_mod.align_plane_solve(w, RNG, 3.0, 4.0, start)
        assert stats["degenerate"] and np.array_equal(est, start), name       # the estimate it was given, bit for bit
        assert stats["n"] == words[0] and math.isnan(stats["rms_xz"]) and math.isnan(stats["rms_y"]), name
        _same((est, stats), PR.solve(w, RNG, 3.0, 4.0, start))
    # ... and three pairs in general position are enough
    est, stats = scanner_mod.align_plane_solve(np.array([_words(f[:3])], dtype=np.int64), RNG, 0.0, 0.0, _start(3, 4, 5, (10, 20)))
    assert not stats["degenerate"] and stats["n"] == 3


def test_the_refusals(scanner_mod):
    L = scanner_mod.load_library()
    w = np.array([_words(_rigid_features(3, 4, 5, (0, 0), 10, 1))], dtype=np.int64)
    est = np.array([0.6, 0.8, 0.0, 0.0])
    nan, inf = float("nan"), float("inf")

    def call(sums=w, n=1, rng=256.0, ox=0.0, oz=0.0, est_in=est, null_out=False, null_stats=False):
        out, stats = np.full(4, -7.0), np.full(4, -7.0)
        rc = L.sl3d_align_plane_solve(None if sums is None else sums.ctypes.data, n, rng, ox, oz, None if est_in is None else est_in.ctypes.data,
                                      None if null_out else out.ctypes.data, None if null_stats else stats.ctypes.data)
        assert rc == 0 or ((out == -7.0).all() and (stats == -7.0).all())     # a refused call writes nothing
        return rc
    assert call() == 0
    for kw in (dict(sums=None), dict(est_in=None), dict(null_out=True), dict(null_stats=True), dict(n=0), dict(n=-1), dict(rng=0.0), dict(rng=-1.0),
               dict(rng=nan), dict(rng=inf), dict(ox=nan), dict(oz=inf), dict(est_in=np.array([1.0, nan, 0.0, 0.0])),
               dict(est_in=np.array([1.0, 0.0, -inf, 0.0]))):
        assert call(**kw) == -1, kw
    with pytest.raises(scanner_mod.Sl3dError):
        scanner_mod.align_plane_solve(w, 0.0, 0.0, 0.0, est)
    assert L.sl3d_align_plane_solve.argtypes[0] is C.c_void_p
