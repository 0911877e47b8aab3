"""CPU test of the crafted segmented clouds (tests/segment_cases.py): the cases contain what they are built for -- every seam kind on every
shape where it exists, the lone points, the non-finite payloads, the two registration cases -- every case satisfies the bounds the helper
asserts before it writes (tests/cloud_segments.py), and the restatement agrees with a literal per-segment loop.  The same cases run on the
device in tests/test_gpu_cloud_segments_crafted.py."""
import numpy as np
import pytest

import segment_cases as SC

ALL_SHAPES = SC.SMALL_SHAPES + SC.LONG_SHAPES


def test_geometry_of_the_shapes():
    """n_segs and the k_seg_scan layout of every shape, as the code computes them (sl3d_capi_clouds.cpp: n_segs = 4 * tiles; sl3d_clouds.hip:
    part_len = ceil(ceil(n / 8) / 4096) * 4096)"""
    want = {(64, 3): (4, 1), (1021, 64): (256, 256), (1024, 260): (1040, 1040), (1024, 1100): (4400, 4400),
            (4096, 1800): (28800, 28800), (4096, 2325): (37200, 37200), (4096, 3900): (62400, 62400), (4096, 4100): (65600, 65600)}
    for shape in ALL_SHAPES:
        _, px, n_segs, n_real = SC.geometry(*shape)
        assert (n_segs, n_real) == want[shape], shape
        assert SC.room(*shape).sum() == px
    assert SC.room(64, 3).tolist() == [192, 0, 0, 0]
    # (parts that own counts, chunks per part, counts in the very last chunk)
    assert SC.scan_layout(4400) == (2, 1, 304)              # two parts, the second a partial chunk
    assert SC.scan_layout(28800) == (8, 1, 128)             # part 7 non-empty
    assert SC.scan_layout(37200) == (5, 2, 336)             # two chunks per part, the last one 336 counts
    assert SC.scan_layout(62400) == (8, 2, 960)             # part 7 non-empty AND two chunks long: the total is a carry across chunks
    assert SC.scan_layout(65600) == (6, 3, 64)              # three chunks per part
    # what the suite's decodes reach: 1080p, the 8192 x 768 stripes, the 1 Mpx views of the 4 GiB test -- one chunk per part, part 7 empty
    for shape, parts in (((1920, 1080), 2), ((8192, 768), 6), ((1024, 1024), 1)):
        n = SC.geometry(*shape)[2]
        assert SC.scan_layout(n)[:2] == (parts, 1), shape


def test_bounds_refuse_what_would_read_out_of_the_allocation():
    """the three asserts put_segments makes before it writes a count"""
    ok = np.array([192, 0, 0, 0], np.uint32)
    SC.check_bounds(64, 3, ok)
    for bad in ([193, 0, 0, 0], [257, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0, 1]):
        with pytest.raises(AssertionError):
            SC.check_bounds(64, 3, np.array(bad, np.uint32))
    with pytest.raises(AssertionError):
        SC.check_bounds(64, 3, ok.astype(np.int32))
    with pytest.raises(AssertionError):
        SC.check_bounds(64, 3, ok[:3])
    full = SC.room(1021, 64).astype(np.uint32)
    SC.check_bounds(1021, 64, full)
    full[17] = 257
    with pytest.raises(AssertionError):
        SC.check_bounds(1021, 64, full)


@pytest.mark.parametrize("shape", ALL_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_patterns_hold_every_seam_and_stay_in_bounds(shape):
    W, H = shape
    _, px, n_segs, n_real = SC.geometry(W, H)
    pats = SC.count_patterns(W, H)
    rm = SC.room(W, H)
    for name, c in pats.items():
        SC.check_bounds(W, H, c)
    assert not pats["zeros"].any()
    assert np.array_equal(pats["full"], rm) and pats["full"][n_real - 1] == px - 256 * (n_real - 1) and pats["full"].sum() == px
    assert pats["first_only"].sum() == 1 and pats["first_only"][0] == 1
    assert pats["last_only"].sum() == 1 and pats["last_only"][n_real - 1] == 1
    alt = pats["alternating"]
    assert not alt[0::2].any() and (alt[1:n_real - 1:2] == 256).all()
    assert set(np.unique(pats["sparse"])) <= {0, 1, 2, 3} and 0 < np.count_nonzero(pats["sparse"]) <= max(1, n_segs // 10)
    if n_real > 8:
        assert pats["random"].min() == 0 or n_real < 300
        assert len(np.unique(pats["random"])) > min(n_real, 256) // 2
    # non-zero exactly at the block-of-4 seam indices / at the seam indices of every kind that exists in the shape
    b4 = SC.block4_indices(W, H)
    assert np.array_equal(np.flatnonzero(pats["block4"]), b4)
    assert (len(b4) > 0) == (n_real > 4) and all(i % 4 in (0, 3) for i in b4)
    seams = SC.seam_indices(W, H)
    union = np.unique(np.concatenate(list(seams.values()))).astype(np.int64)
    assert np.array_equal(np.flatnonzero(pats["seams"]), union)
    for kind, m in zip(SC.SEAM_KINDS, (256, 1024, 4096, SC.part_len(n_segs))):
        exists = [i for k in range(1, n_real // m + 2) for i in (m * k - 1, m * k + 1) if i < n_real]
        assert seams[kind].tolist() == sorted(exists), kind
        assert all(pats["seams"][i] > 0 for i in exists), kind
    # which kinds exist where
    have = {k: len(v) > 0 for k, v in seams.items()}
    assert have["lane_run_256"] == (n_real >= 256) and have["front_stride_1024"] == (n_real >= 1024)
    assert have["chunk_4096"] == (n_real >= 4096) and have["part"] == (n_real >= SC.part_len(n_segs))
    if shape in SC.LONG_SHAPES:
        assert all(have.values())
        assert SC.part_len(n_segs) * 7 - 1 in seams["part"] or SC.scan_layout(n_segs)[0] < 8


def test_every_seam_kind_occurs_on_a_small_shape():
    seen = {k: [s for s in SC.SMALL_SHAPES if len(SC.seam_indices(*s)[k])] for k in SC.SEAM_KINDS}
    assert seen["lane_run_256"] == [(1021, 64), (1024, 260), (1024, 1100)]
    assert seen["front_stride_1024"] == [(1024, 260), (1024, 1100)]
    assert seen["chunk_4096"] == [(1024, 1100)] and seen["part"] == [(1024, 1100)]


def test_payloads_are_what_they_claim():
    n = 4096
    nan = SC.payload("nan", n).view(np.uint32).ravel()
    assert np.isnan(nan.view(np.float32)).all() and len(np.unique(nan)) == 3 * n
    assert (nan >> 31).min() == 0 and (nan >> 31).max() == 1
    assert ((nan & 0x00400000) == 0).any() and ((nan & 0x00400000) != 0).any()                  # signalling and quiet
    sp = SC.payload("special", n)
    b = sp.view(np.uint32)
    assert np.isposinf(sp).any() and np.isneginf(sp).any() and (b == 0x80000000).any()
    den = (b & 0x7F800000 == 0) & (b & 0x007FFFFF != 0)
    assert den.any() and (den & (b >> 31 == 1)).any()
    fin = SC.payload("finite", n)
    assert np.isfinite(fin).all() and not SC.holds_sentinel(fin) and np.abs(fin).max() <= 1000
    ny = SC.payload("reg_nan_y", n)
    assert np.isfinite(ny[:, [0, 2]]).all() and np.isnan(ny[:, 1]).any() and np.isinf(ny[:, 1]).any()
    fm = SC.payload("reg_flt_max", n)
    assert np.isfinite(fm).all() and (np.abs(fm) > 2.8e38).any()
    for k in SC.PAYLOADS:
        assert not SC.holds_sentinel(SC.payload(k, n)), k


def test_cases_cover_patterns_payloads_and_registration_positions():
    names = [f"{p}-{q}" for p, q in SC.CASE_LIST]
    assert len(set(names)) == len(names) == 15
    assert {p for p, _ in SC.CASE_LIST} == set(SC.count_patterns(64, 3)) and {q for _, q in SC.CASE_LIST} == set(SC.PAYLOADS)
    for q in ("reg_nan_y", "reg_flt_max"):                                     # in views 1 / 2 of their triple: a rotation angle that is not 0
        assert all(i % 3 != 0 for i, (_, qq) in enumerate(SC.CASE_LIST) if qq == q)
    for shape in SC.SMALL_SHAPES:
        for name, counts, xyz in SC.cases_of(shape):
            SC.check_bounds(*shape, counts)
            assert xyz.shape == (len(counts) * 256, 3) and xyz.dtype == np.float32


def test_registration_cases_produce_nan_and_infinity():
    """the oracle over the restated clouds: an infinite or NaN y with finite x, z gives NaN X and Z (y times an exact 0.0); coordinates near
    FLT_MAX give an infinite float out of finite ones"""
    shape = (1021, 64)
    triple = SC.triples_of(shape)[3]
    assert [n for n, _, _ in triple] == ["random2-nan", "random-reg_nan_y", "random2-reg_flt_max"]
    clouds = [SC.restate(c, SC.with_fill(*shape, c, x, SC.SENTINEL))[2] for _, c, x in triple]
    for t, step in SC.REG_SETTINGS:
        reg = SC.registered(clouds, t, step)
        assert reg.shape == (sum(len(c) for c in clouds), 3) and not SC.holds_sentinel(reg)
        a, b = len(clouds[0]), len(clouds[0]) + len(clouds[1])
        src, out = clouds[1], reg[a:b]
        bad_y = ~np.isfinite(src[:, 1])
        assert bad_y.sum() > 100 and np.isnan(out[bad_y][:, [0, 2]]).all() and np.isfinite(out[~bad_y]).all()
        src, out = clouds[2], reg[b:]
        assert np.isfinite(src).all() and np.isinf(out).sum() > 100


@pytest.mark.parametrize("shape", [(64, 3), (1021, 64)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_restatement_agrees_with_the_literal_loop(shape):
    for name, counts, xyz in SC.cases_of(shape):
        filled = SC.with_fill(*shape, counts, xyz, SC.SENTINEL)
        o1, t1, c1 = SC.restate(counts, filled)
        o2, t2, c2 = SC.restate_loop(counts, filled)
        assert t1 == t2 == int(counts.sum()) and np.array_equal(o1, o2) and o1.dtype == np.uint64, name
        assert c1.shape == c2.shape and np.array_equal(c1.view(np.uint32), c2.view(np.uint32)), name
        assert not SC.holds_sentinel(c1), name
        # the sentinel is behind every count, and only there
        s = filled.reshape(-1, 256, 3)
        behind = np.arange(256)[None, :] >= counts[:, None].astype(np.int64)
        assert (s[behind].view(np.uint32) == SC.SENTINEL_BITS).all() and not SC.holds_sentinel(s[~behind]), name
        for cap in SC.capacities(counts, o1, t1, SC.seam_segments(*shape, counts)):
            assert len(SC.clamped(c1, cap)) == min(cap, t1)


def test_clamped_capacities_hit_a_segment_seam():
    shape = (1024, 1100)
    pats = SC.count_patterns(*shape)
    for name in ("random", "seams", "block4", "full"):
        c = pats[name]
        o, t, _ = SC.restate(c, np.zeros((len(c) * 256, 3), np.float32))
        seams = SC.seam_segments(*shape, c)
        caps = SC.capacities(c, o, t, seams)
        assert {1, t - 1, t} <= set(caps) and len(seams) >= 2
        assert any(int(o[s]) in caps for s in seams if o[s] > 0), name           # a capacity that ends exactly on a segment seam
    assert SC.capacities(pats["zeros"], *SC.restate(pats["zeros"], np.zeros((0, 3), np.float32))[:2], []) == [1]
