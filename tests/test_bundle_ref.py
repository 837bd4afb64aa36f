"""Known answers that pin tests/bundle_ref.py, the NumPy restatement of the "Bundle tools" section of include/fibers_hip.h that the
GPU tests hold the kernels to.  No GPU and no library: answers worked out by hand."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bundle_ref as bd  # noqa: E402

RES = (1.25, 0.5, 2.0)


def _one(p, K, flip=None, res=RES):
    p = np.asarray(p, np.float32).reshape(-1, 3)
    return bd.resample(p, [p.shape[0]], res, K, None if flip is None else [flip])[0]


def test_uneven_points_on_a_straight_line_come_out_equidistant():
    # along (4, 10, 2.5) voxels = (5, 5, 5) mm: |.| = sqrt(75) per unit of s; every value below is exact in float32
    s = np.array([0, 0.125, 0.25, 1.0, 1.5, 4.0, 8.0])
    p = np.array([2.0, 3.0, 1.0]) + s[:, None] * np.array([4.0, 10.0, 2.5])
    out = _one(p, 9)
    want = np.array([2.0, 3.0, 1.0]) + np.arange(9)[:, None] * np.array([4.0, 10.0, 2.5])
    assert out.dtype == np.float32 and np.allclose(out, want, rtol=0, atol=4e-6)
    mm = np.linalg.norm(np.diff(out.astype(np.float64), axis=0) * np.array(RES), axis=1)
    assert np.allclose(mm, np.sqrt(75.0), rtol=1e-6)
    assert np.array_equal(out[0], p[0].astype(np.float32)) and np.array_equal(out[8], p[-1].astype(np.float32))
    # the spacing is equal in mm, not in voxels: a line with one step along x and one along z of the same voxel length
    q = _one([[1, 1, 1], [5, 1, 1], [5, 1, 5]], 3)                           # 5 mm, then 8 mm: the middle row lies 1.5 mm into the second segment
    assert np.array_equal(q, np.array([[1, 1, 1], [5, 1, 1.75], [5, 1, 5]], np.float32))


def test_the_corner_of_an_l_shaped_line_at_the_right_row():
    p = [[1, 1, 1], [5, 1, 1], [5, 11, 1]]                                    # 5 mm along x, then 5 mm along y
    out = _one(p, 5)
    assert np.array_equal(out, np.array([[1, 1, 1], [3, 1, 1], [5, 1, 1], [5, 6, 1], [5, 11, 1]], np.float32))
    out = _one(p, 4)                                                          # rows at 10/3 and 20/3 mm
    assert np.allclose(out[1], [1 + 4 * (10 / 3) / 5, 1, 1], atol=1e-6) and np.allclose(out[2], [5, 1 + 10 * (20 / 3 - 5) / 5, 1], atol=1e-6)


def test_duplicated_points_and_an_all_equal_line_give_copies_and_no_nan():
    p = [[1, 1, 1], [1, 1, 1], [5, 1, 1], [5, 1, 1], [5, 1, 1], [5, 11, 1], [5, 11, 1]]
    assert np.array_equal(_one(p, 5), np.array([[1, 1, 1], [3, 1, 1], [5, 1, 1], [5, 6, 1], [5, 11, 1]], np.float32))
    same = _one([[2.5, -3, 7]] * 6, 7)
    assert np.array_equal(same, np.tile(np.array([2.5, -3, 7], np.float32), (7, 1)))
    assert np.array_equal(_one([[2.5, -3, 7]], 4), np.tile(np.array([2.5, -3, 7], np.float32), (4, 1)))   # n = 1


def test_two_points_are_the_two_ends_and_huge_coordinates_are_legal():
    p = np.array([[1, 2, 3], [4, 4, 4], [9, 8, 7.5]], np.float32)
    assert np.array_equal(_one(p, 2), p[[0, 2]])
    big = _one([[0, 0, 0], [1e30, 0, 0], [1e30, 0, 4]], 3)
    assert np.isfinite(big).all() and np.array_equal(big[[0, 2]], np.array([[0, 0, 0], [1e30, 0, 4]], np.float32))
    assert abs(float(big[1, 0]) - 5e29) <= 1e23 and big[1, 1] == 0 and big[1, 2] == 0


def test_no_points_and_non_finite_points_give_nan_rows():
    for p in (np.zeros((0, 3)), [[1, 1, 1], [np.nan, 1, 1], [2, 2, 2]], [[1, 1, 1], [2, 2, 2], [2, np.inf, 2]], [[-np.inf, 0, 0], [1, 1, 1]]):
        out = _one(p, 6)
        assert (out.view(np.uint32) == 0x7FC00000).all()
    one = _one([[np.nan, 2, np.inf]], 3)                                      # n = 1 is a copy whatever the point holds
    assert np.isnan(one[:, 0]).all() and (one[:, 1] == 2).all() and np.isinf(one[:, 2]).all()


def test_flip_reverses_the_rows_and_lines_do_not_depend_on_their_neighbours():
    rng = np.random.default_rng(1)
    n = np.array([5, 0, 1, 9, 2])
    xyz = rng.uniform(1, 9, (int(n.sum()), 3)).astype(np.float32)
    a = bd.resample(xyz, n, RES, 7)
    b = bd.resample(xyz, n, RES, 7, flip=[1, 1, 0, 1, 0])
    for i, f in enumerate([1, 1, 0, 1, 0]):
        assert np.array_equal(b[i].view(np.uint32), (a[i][::-1] if f else a[i]).view(np.uint32))
    off = np.concatenate([[0], np.cumsum(n)])
    assert np.array_equal(bd.resample(xyz[off[3]:off[4]], [9], RES, 7)[0], a[3])


def _mdf_lines():
    a = np.array([[1, 1, 1], [2, 1.5, 1], [3, 2.5, 2], [5, 2.5, 4]], np.float32)
    return a, a[::-1].copy()


def test_mdf_of_a_line_with_itself_its_reverse_and_a_shifted_copy():
    a, rev = _mdf_lines()
    shifted = a + np.array([1, 0, 0], np.float32)
    d, f = bd.mdf(a[None], np.stack([a, rev, shifted]), RES)
    assert d[0, 0] == 0 and f[0, 0] == 0                                      # itself: direct, and the tie d_flip == d_dir is impossible here
    assert d[0, 1] == 0 and f[0, 1] == 1                                      # its reverse: the flipped sum is 0
    assert d[0, 2] == 1.25 and f[0, 2] == 0                                   # one voxel in x: exactly r_x
    sym = np.array([[1, 1, 1], [2, 1, 1], [3, 1, 1]], np.float32)             # a palindrome in distances: d_flip == d_dir, so f = 0
    d, f = bd.mdf(sym[None], (sym + np.array([0, 2, 0], np.float32))[None], RES)
    assert d[0, 0] == 1.0 and f[0, 0] == 0


def test_first_minimum_nan_and_the_threshold_at_equality():
    a, rev = _mdf_lines()
    far = a + np.array([0, 0, 3], np.float32)                                 # 6 mm away
    nanm = a.copy(); nanm[2, 1] = np.nan
    models = np.stack([far, nanm, a + np.array([1, 0, 0], np.float32), rev + np.array([1, 0, 0], np.float32), far])
    label, dist, flip, dall = bd.assign(a[None], models, RES, 10.0)
    assert label[0] == 2 and dist[0] == np.float32(1.25) and flip[0] == 0     # models 2 and 3 tie at 1.25: the first wins
    assert np.isnan(dall[0, 1]) and dall[0, 0] == 6 and dall[0, 4] == 6 and dall[0, 3] == np.float32(1.25)
    label, dist, flip, _ = bd.assign(a[None], models[[3, 2]], RES, 1.25)      # the flipped one first; the threshold at equality keeps it
    assert label[0] == 0 and flip[0] == 1 and dist[0] == np.float32(1.25)
    label, dist, flip, _ = bd.assign(a[None], models, RES, 1.2499999)
    assert label[0] == -1 and dist[0] == np.float32(1.25)                     # dist is written whatever the threshold says
    label, dist, flip, _ = bd.assign(np.stack([a, nanm]), models[[1, 1]], RES, np.inf)
    assert list(label) == [-1, -1] and np.isnan(dist).all() and not flip.any()           # every d is NaN
    label, dist, flip, _ = bd.assign(a[None], models[:1], RES, np.nan)             # a NaN threshold keeps nothing
    assert label[0] == -1 and dist[0] == 6


def test_centroids_of_two_lines_one_flipped():
    a = np.array([[1, 1, 1], [2, 2, 2], [4, 4, 4]], np.float32)
    b = np.array([[6, 4, 2], [3, 2, 1], [1, 1, 3]], np.float32)               # stored against the model's direction
    c = np.array([[9, 9, 9]] * 3, np.float32)
    lines = np.stack([a, b, c, c, c])
    S, N, bound = bd.centroids(lines, [1, 1, -1, 3, 4], [0, 1, 0, 0, 1], 3)
    assert list(N) == [0, 2, 0] and N.dtype == np.uint32
    assert np.array_equal(S[1], np.array([[2, 2, 4], [5, 4, 3], [10, 8, 6]], np.float64)) and not S[0].any() and not S[2].any()
    assert np.array_equal(bound[1], 2.0 ** -52 * S[1]) and not bound[0].any()
