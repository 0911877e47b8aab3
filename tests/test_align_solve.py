"""CPU tests of the turntable refinement's solve through the library's own entry point (sl3d_align_solve: host only, no context, no GPU)
against the restatement (tests/align_reference.solve) and against the truth.

Exactly rigid integer pairs -- rotations by the Pythagorean angles, whose cosine and sine are fractions of 5, 13 and 17, applied to multiples
of the denominator, and by the quarter turns -- give moments that describe a rigid motion without any rounding: the solve recovers the
angle and the axis point, and agrees with the restatement, to 1e-9 relative.  The bound is derived, not measured: both sides form the
centred moments as exact integers, so only the roundings of some twenty double operations (2^-53 each) and the libm calls (below an ulp
each) separate them from each other, and the conditioning of (I - R) t = d -- 1 / |1 - e^(i theta)| <= 3 for the angles used -- from the
truth.  Then every degenerate condition, sums near the 2^62 bound, several pairs that add like one, and the refusals."""
import ctypes as C
import math

import numpy as np
import pytest

import align_reference as AR

REL = 1e-9
ANGLES = {"3-4-5": (3, 4, 5), "minus 3-4-5": (3, -4, 5), "5-12-13": (5, 12, 13), "obtuse 8-15-17": (-8, 15, 17), "quarter": (0, 1, 1),
          "minus quarter": (0, -1, 1), "half": (-1, 0, 1)}


def _rigid_pairs(cn, sn, den, t, n, seed, span=1 << 12):
    """n integer points a and b = R (a - t) + t, exact: a - t is a multiple of den"""
    rng = np.random.default_rng(seed)
    d = rng.integers(-span, span, (n, 2)) * den
    a = d + np.array(t)
    b = np.stack([(cn * d[:, 0] - sn * d[:, 1]) // den, (sn * d[:, 0] + cn * d[:, 1]) // den], axis=1) + np.array(t)
    assert np.array_equal((b - np.array(t)) * den, np.stack([cn * d[:, 0] - sn * d[:, 1], sn * d[:, 0] + cn * d[:, 1]], axis=1))
    return a, b


def _words(a, b, dy=None, sources=None):
    """the 12 words of integer pairs, as exact Python integers"""
    ax, az, bx, bz = ([int(v) for v in col] for col in (a[:, 0], a[:, 1], b[:, 0], b[:, 1]))
    dy = [0] * len(ax) if dy is None else [int(v) for v in dy]
    return [len(ax), sum(ax), sum(az), sum(bx), sum(bz), sum(p * q + r * s for p, q, r, s in zip(ax, bx, az, bz)),
            sum(p * s - r * q for p, q, r, s in zip(ax, bx, az, bz)), sum(p * p + r * r for p, r in zip(ax, az)),
            sum(q * q + s * s for q, s in zip(bx, bz)), sum(dy), sum(v * v for v in dy), len(ax) if sources is None else sources]


def _close(got, want, rel=REL):
    return abs(got - want) <= rel * max(abs(want), 1e-300)


def _same(got, want):
    (ge, gs), (we, ws) = got, want
    assert gs["degenerate"] == ws["degenerate"] and gs["n"] == ws["n"]
    for k in range(4):
        assert _close(ge[k], we[k]) or abs(ge[k] - we[k]) <= REL, (k, ge[k], we[k])    # (a cosine of exactly 0 comes out as 6e-17)
    for key in ("rms_xz", "rms_y"):
        assert (math.isnan(gs[key]) and math.isnan(ws[key])) or abs(gs[key] - ws[key]) <= REL * max(ws[key], 1e-6), key


@pytest.mark.parametrize("name", list(ANGLES))
def test_rigid_integer_pairs(scanner_mod, name):
    cn, sn, den = ANGLES[name]
    rng, ox, oz, t = 256.0, 31.5, -12.25, (1234, -777)
    a, b = _rigid_pairs(cn, sn, den, t, 500, 7)
    dy = np.random.default_rng(8).integers(-300, 300, 500)
    w = np.array([_words(a, b, dy)], dtype=np.int64)
    est0 = np.array([1.0, 0.0, ox, oz])
    got, want = scanner_mod.align_solve(w, rng, ox, oz, est0), AR.solve(w, rng, ox, oz, est0)
    _same(got, want)
    est, stats = got
    assert not stats["degenerate"] and stats["n"] == 500
    Q = 262144.0 / 256.0
    assert abs(est[0] - cn / den) <= REL and abs(est[1] - sn / den) <= REL
    assert _close(math.atan2(est[1], est[0]), math.atan2(sn, cn))
    assert _close(est[2], ox + t[0] / Q) and _close(est[3], oz + t[1] / Q)
    assert stats["rms_xz"] <= 1e-6 / Q * np.abs(a).max()                     # a rigid motion leaves no residual: sqrt of the moments' rounding
    assert _close(stats["rms_y"], float(np.std(dy)) / Q, 1e-12)


def test_every_degenerate_condition(scanner_mod):
    rng, ox, oz, est0 = 100.0, 3.0, 4.0, np.array([0.6, 0.8, 2.5, -1.5])
    a, b = _rigid_pairs(3, 4, 5, (10, 20), 50, 3)
    cases = {
        "no pair": [0] * 11 + [9],
        "one pair": _words(a[:1], b[:1]),
        "every pair the same": _words(np.repeat(a[:1], 7, 0), np.repeat(b[:1], 7, 0)),       # X == 0 and C == 0
        "sources on one spot": _words(np.repeat(a[:1], 7, 0), b[:7]),
        "a pure translation": _words(a, a + np.array([17, -5])),                              # theta == 0: c' == 1.0
    }
    for name, words in cases.items():
        w = np.array([words], dtype=np.int64)
        est, stats = scanner_mod.align_solve(w, rng, ox, oz, est0)
        assert stats["degenerate"] and np.array_equal(est, est0), name       # the estimate it was given, bit for bit
        assert stats["n"] == words[0] and math.isnan(stats["rms_xz"]) and math.isnan(stats["rms_y"]), name
        _same((est, stats), AR.solve(w, rng, ox, oz, est0))
    # ... and two different pairs are enough
    est, stats = scanner_mod.align_solve(np.array([_words(a[:2], b[:2])], dtype=np.int64), rng, ox, oz, est0)
    assert not stats["degenerate"] and abs(est[0] - 0.6) <= REL and abs(est[1] - 0.8) <= REL


def test_sums_near_the_bound(scanner_mod):
    """2^25 - 4 pairs with coordinates next to +-2^18: words 7 and 8 are next to 2^62"""
    m, lim = ((1 << 25) - 4) // 4, (1 << 18) - 1
    a = np.array([[lim, lim], [-lim, lim - 2], [lim - 4, -lim], [-lim + 1, -lim + 3]], dtype=np.int64)
    t = np.array([3, -2])
    d = a - t
    b = np.stack([-d[:, 1], d[:, 0]], axis=1) + t                            # a quarter turn about t
    assert np.abs(b).max() <= lim + 5
    b = np.clip(b, -lim, lim)                                               # (the clip leaves the motion a little short of rigid)
    words = [m * v for v in _words(a, b, dy=[lim, -lim, lim - 1, 7])]
    assert (1 << 61) < words[7] < (1 << 62) and (1 << 61) < words[8] < (1 << 62) and words[0] == (1 << 25) - 4
    w = np.array([words], dtype=np.int64)
    est0 = np.array([1.0, 0.0, 0.0, 0.0])
    got, want = scanner_mod.align_solve(w, 256.0, 0.0, 0.0, est0), AR.solve(w, 256.0, 0.0, 0.0, est0)
    _same(got, want)
    est, stats = got
    assert not stats["degenerate"] and abs(est[0]) < 1e-4 and abs(est[1] - 1.0) < 1e-8
    assert math.hypot(est[2] - 3 / 1024.0, est[3] + 2 / 1024.0) < 0.01 and stats["rms_xz"] < 0.01 and stats["rms_y"] > 100.0


def test_several_pairs_add_like_one(scanner_mod):
    a, b = _rigid_pairs(5, 12, 13, (-40, 90), 300, 11)
    b = b + np.random.default_rng(12).integers(-3, 4, b.shape)                # not rigid any more: a residual
    dy = np.random.default_rng(13).integers(-50, 50, 300)
    one = np.array([_words(a, b, dy, sources=400)], dtype=np.int64)
    three = np.array([_words(a[:100], b[:100], dy[:100], 150), _words(a[100:101], b[100:101], dy[100:101], 50), _words(a[101:], b[101:], dy[101:], 200)],
                     dtype=np.int64)
    assert np.array_equal(three.sum(axis=0), one[0])
    est0 = np.array([1.0, 0.0, 5.0, 6.0])
    e1, s1 = scanner_mod.align_solve(one, 256.0, 5.0, 6.0, est0)
    e3, s3 = scanner_mod.align_solve(three, 256.0, 5.0, 6.0, est0)
    assert np.array_equal(e1, e3) and s1 == s3 and not s1["degenerate"] and s1["rms_xz"] > 0.0
    # rows whose int64 sum would wrap: the words are added in 128 bits
    huge = (1 << 62) + 12345
    wrap = np.array([one[0] + huge, one[0] * 0 - huge, one[0] * 0 + huge, one[0] * 0 - huge], dtype=np.int64)
    e4, s4 = scanner_mod.align_solve(wrap, 256.0, 5.0, 6.0, est0)
    assert np.array_equal(e1, e4) and s1 == s4
    _same((e3, s3), AR.solve(three, 256.0, 5.0, 6.0, est0))


def test_the_refusals(scanner_mod):
    L = scanner_mod.load_library()
    w = np.array([_words(*_rigid_pairs(3, 4, 5, (0, 0), 10, 1))], dtype=np.int64)
    est = np.array([1.0, 0.0, 0.0, 0.0])
    nan, inf = float("nan"), float("inf")

    def call(sums=w, n=1, rng=256.0, ox=0.0, oz=0.0, est_in=est, null_out=False, null_stats=False):
        out, stats = np.full(4, -7.0), np.full(4, -7.0)
        rc = L.sl3d_align_solve(None if sums is None else sums.ctypes.data, n, rng, ox, oz, None if est_in is None else est_in.ctypes.data,
                                None if null_out else out.ctypes.data, None if null_stats else stats.ctypes.data)
        assert rc == 0 or ((out == -7.0).all() and (stats == -7.0).all())     # a refused call writes nothing
        return rc
    assert call() == 0
    for kw in (dict(sums=None), dict(est_in=None), dict(null_out=True), dict(null_stats=True), dict(n=0), dict(n=-1), dict(rng=0.0), dict(rng=-1.0),
               dict(rng=nan), dict(rng=inf), dict(ox=nan), dict(oz=inf), dict(est_in=np.array([1.0, nan, 0.0, 0.0])),
               dict(est_in=np.array([1.0, 0.0, -inf, 0.0]))):
        assert call(**kw) == -1, kw
    with pytest.raises(scanner_mod.Sl3dError):
        scanner_mod.align_solve(w, 0.0, 0.0, 0.0, est)
    assert L.sl3d_align_solve.argtypes[0] is C.c_void_p
