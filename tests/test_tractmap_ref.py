"""The NumPy restatement of the tract maps (tests/tractmap_ref.py) against answers counted by hand from the definitions in
include/fibers_hip.h ("Tract maps").  tests/test_gpu_tractmap.py holds the HIP kernels to this restatement bit for bit, so what is
pinned here is what the kernels are held to.  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tractmap_ref as tm  # noqa: E402

SHAPE = (6, 5, 4)


def lin(x, y, z, shape=SHAPE):
    return (x - 1) + shape[0] * ((y - 1) + shape[1] * (z - 1))


def witnesses():
    """the tie / outside witnesses (also run on the device): points, and for each the voxel (x, y, z) it belongs to or None"""
    big = np.float32(1e30)
    pts = [((2.5, 1, 1), (2, 1, 1)), ((3.5, 1, 1), (4, 1, 1)), ((4.5, 2, 2), (4, 2, 2)), ((5.5, 2, 2), (6, 2, 2)),     # ties to even
           ((1, 0.5, 1), None), ((1, 1.5, 1), (1, 2, 1)), ((1, 1, 2.5), (1, 1, 2)), ((1, 1, 3.5), (1, 1, 4)),
           ((0.49, 1, 1), None), ((0.51, 1, 1), (1, 1, 1)), ((6.5, 1, 1), (6, 1, 1)), ((6.51, 1, 1), None),               # nx + 0.5 -> nx (even)
           ((1, 5.5, 1), None), ((1, 5.49, 1), (1, 5, 1)), ((1, 1, 4.5), (1, 1, 4)), ((1, 1, 4.51), None),               # ny + 0.5 = 5.5 -> 6: out
           ((np.nan, 1, 1), None), ((1, np.nan, 1), None), ((1, 1, np.nan), None), ((np.inf, 1, 1), None), ((1, -np.inf, 1), None),
           ((big, 1, 1), None), ((1, -big, 1), None), ((1, 1, big), None), ((-3, 2, 2), None), ((3, 2, 2), (3, 2, 2))]
    xyz = np.array([p for p, _ in pts], np.float32)
    want = np.array([-1 if v is None else lin(*v) for _, v in pts], np.int64)
    return xyz, want


def test_voxel_rounds_ties_to_even_and_tests_the_float_value():
    xyz, want = witnesses()
    assert np.array_equal(tm.voxel(xyz, SHAPE), want)
    # a rule that rounds half away from zero gives ANOTHER map on these points: a kernel that uses floor(x + .5) cannot pass
    with np.errstate(invalid="ignore"):
        away = np.floor(xyz + np.float32(0.5))
    assert away[0, 0] == 3 and away[1, 0] == 4 and away[2, 0] == 5 and away[3, 0] == 6      # 2.5 -> 3 (even rule: 2), 4.5 -> 5 (4)
    d, nout = tm.density(xyz, [len(xyz)], SHAPE, tm.POINTS)
    assert d[lin(2, 1, 1)] == 1 and d[lin(3, 1, 1)] == 0 and d[lin(4, 1, 1)] == 1 and d[lin(4, 2, 2)] == 1 and d[lin(5, 2, 2)] == 0
    assert nout == int((want < 0).sum()) == 14 and int(d.sum()) + nout == len(xyz)


def test_straight_line_along_x():
    # x = 1.0, 1.5, ..., 6.0 at y = 2, z = 3, step 0.5: rint -> 1 2 2 2 3 4 4 4 5 6 6  (1.5 -> 2, 2.5 -> 2, 3.5 -> 4, 4.5 -> 4, 5.5 -> 6)
    x = np.arange(1.0, 6.01, 0.5, dtype=np.float32)
    xyz = np.stack([x, np.full_like(x, 2), np.full_like(x, 3)], 1)
    want_pts = {1: 1, 2: 3, 3: 1, 4: 3, 5: 1, 6: 2}
    dp, op = tm.density(xyz, [len(x)], SHAPE, tm.POINTS)
    dl, ol = tm.density(xyz, [len(x)], SHAPE, tm.LINES)
    de, oe = tm.density(xyz, [len(x)], SHAPE, tm.ENDPOINTS)
    for vx, c in want_pts.items():
        assert dp[lin(vx, 2, 3)] == c and dl[lin(vx, 2, 3)] == 1
    assert dp.sum() == 11 and dl.sum() == 6 and op == ol == oe == 0
    assert de[lin(1, 2, 3)] == 1 and de[lin(6, 2, 3)] == 1 and de.sum() == 2


def test_a_line_that_comes_back_counts_once_per_voxel():
    # (2,2,2) (2,2,2) (3,2,2) (3,3,2) (2,3,2) (2,2,2) (2,2,2) (1,2,2): voxel (2,2,2) is left and entered again
    xyz = np.array([[2, 2, 2], [2.2, 2, 2], [3, 2, 2], [3, 3, 2], [2, 3, 2], [2, 2.4, 2], [2, 2, 2], [1, 2, 2]], np.float32)
    dp, _ = tm.density(xyz, [8], SHAPE, tm.POINTS)
    dl, _ = tm.density(xyz, [8], SHAPE, tm.LINES)
    assert dp[lin(2, 2, 2)] == 4 and dl[lin(2, 2, 2)] == 1
    assert dp.sum() == 8 and dl.sum() == 5 and int((dp - dl).sum()) == 3                  # modes differ by 3, all of it in (2,2,2)
    assert (dl <= dp).all()
    # the same points as two lines: the second line visits (2,2,2) on its own
    dl2, _ = tm.density(xyz, [4, 4], SHAPE, tm.LINES)
    assert dl2[lin(2, 2, 2)] == 2 and dl2.sum() == 6


def test_endpoints_one_point_lines_and_empty_lines():
    xyz = np.array([[1, 1, 1],                       # a one-point line: +2 in one voxel
                    [2, 1, 1], [3, 1, 1], [9, 1, 1],   # ends (2,1,1) and outside
                    [0, 0, 0], [4, 4, 4]],             # starts outside
                   np.float32)
    npts = [0, 1, 0, 0, 3, 2, 0]
    d, nout = tm.density(xyz, npts, SHAPE, tm.ENDPOINTS)
    assert d[lin(1, 1, 1)] == 2 and d[lin(2, 1, 1)] == 1 and d[lin(4, 4, 4)] == 1 and d.sum() == 4 and nout == 2
    assert int(d.sum()) + nout == 2 * 3                                                   # 2 * #{npts >= 1}
    dp, op = tm.density(xyz, npts, SHAPE, tm.POINTS)
    dl, ol = tm.density(xyz, npts, SHAPE, tm.LINES)
    assert int(dp.sum()) + op == 6 and op == ol == 2 and (dl <= dp).all() and dl.sum() == 4
    e, eo = tm.density(np.zeros((0, 3), np.float32), [0, 0], SHAPE, tm.ENDPOINTS)
    assert e.sum() == 0 and eo == 0


def test_accumulate_and_refusals():
    rng = np.random.default_rng(5)
    xyz = rng.uniform(0, 7, (300, 3)).astype(np.float32)
    npts = [100, 0, 150, 50]
    for mode in (tm.POINTS, tm.LINES, tm.ENDPOINTS):
        whole, nw = tm.density(xyz, npts, SHAPE, mode)
        a, na = tm.density(xyz[:100], [100, 0], SHAPE, mode)
        b, nb = tm.density(xyz[100:], [150, 50], SHAPE, mode, into=a)
        assert np.array_equal(b, whole) and na + nb == nw
    assert tm.density(np.ones((1, 3), np.float32), [1], SHAPE, tm.POINTS, into=np.full(120, 0xFFFFFFFF, np.uint32))[0][0] == 0   # wraps at 2^32
    with pytest.raises(ValueError):
        tm.density(xyz, [100, 150, 49], SHAPE, tm.POINTS)
    with pytest.raises(ValueError):
        tm.density(xyz, [301, -1], SHAPE, tm.LINES)


def test_sample_is_a_gather_of_the_nearest_voxel():
    xyz, want = witnesses()
    nvox = SHAPE[0] * SHAPE[1] * SHAPE[2]
    vol = np.arange(3 * nvox, dtype=np.float32).reshape(3, nvox) + 0.25
    s = tm.sample(xyz, vol, SHAPE, outside=-7.0)
    assert s.shape == (len(xyz), 3) and s.dtype == np.float32
    for i, v in enumerate(want):
        assert list(s[i]) == ([-7.0] * 3 if v < 0 else [v + 0.25, nvox + v + 0.25, 2 * nvox + v + 0.25])
    n = tm.sample(xyz, vol[:1], SHAPE, outside=np.nan)
    assert np.isnan(n[want < 0, 0]).all() and not np.isnan(n[want >= 0]).any()


def test_length_and_means():
    # a 3-4-5 segment in mm with anisotropic voxels: dx = 1.5 voxels of 2 mm, dy = 8 voxels of 0.5 mm -> (3, 4, 0) mm; then 12 mm along z
    xyz = np.array([[1, 1, 1], [2.5, 9, 1], [2.5, 9, 5],          # line 0: 5 + 12 = 17 mm
                    [3, 3, 3],                                       # line 1: one point
                    [1, 1, 1], [1, 1, 2]], np.float32)               # line 3 (line 2 is empty): 3 mm
    npts = [3, 1, 0, 2]
    sc = np.array([[1, 10], [2, 20], [6, np.nan], [5, 5], [0.5, -1], [0.25, 1]], np.float32)
    P, B = tm.stats(xyz, npts, (2.0, 0.5, 3.0), sc)
    assert P.shape == (4, 3) and P.dtype == np.float32
    assert list(P[:, 0]) == [17.0, 0.0, 0.0, 3.0]
    assert P[0, 1] == 3.0 and np.isnan(P[0, 2]) and P[1, 1] == 5.0 and P[1, 2] == 5.0
    assert np.isnan(P[2, 1]) and np.isnan(P[2, 2])                                         # 0 / 0
    assert P[3, 1] == 0.375 and P[3, 2] == 0.0
    assert B[0, 0] == 2 * 2.0 ** -52 * 17 and B[3, 1] == 2 * 2.0 ** -52 * 0.75 / 2
    assert tm.stats(xyz, npts, (1, 1, 1))[0].shape == (4, 1)
    # float64 accumulation, rounded once: (2^24 + 1 + 1 + 1) / 4 = 4194304.75 -> 4194305 (float32 accumulation would give 2^22)
    big = np.array([2 ** 24, 1, 1, 1], np.float32)
    assert tm.stats(np.ones((4, 3), np.float32), [4], (1, 1, 1), big)[0][0, 1] == np.float32(4194305.0)
    assert tm.stats_close(P, P, B).all()
    assert tm.ulp32(np.float32(1.0)) == 2.0 ** -23 and tm.ulp32(np.float32(17.0)) == 2.0 ** -19
    assert not tm.stats_close(np.float32(17.0) + np.float32(2.0 ** -18), np.float32(17.0), 0.0)
