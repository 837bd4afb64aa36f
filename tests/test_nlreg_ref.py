"""CPU tests (no GPU) of tests/nlreg_ref.py, the NumPy restatement of the "Non-linear registration" contract that the GPU tests hold
csrc/nlreg.hip to: what the restated algorithm must do on its own (zero on identical volumes, the sign and size of a shift, the quality
condition on a phantom, a positive Jacobian), that each named mutant is visible, and the library's host code (the matrices of a level)
against the restatement."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nlreg_ref as N  # noqa: E402
import warp_ref as W  # noqa: E402

F = np.float32


def _axis_aligned(res=2.0, origin=(-16.0, -8.0, 4.0)):
    """a vox2ras whose every product in the chain is exact in float32: a power-of-two voxel size and a dyadic origin"""
    V = np.eye(4, dtype=F)
    V[0, 0] = V[1, 1] = V[2, 2] = res
    V[:3, 3] = origin
    return V


def _box(V, shape):
    r = W.node_ras(V, shape).reshape(-1, 3)
    return r.min(axis=0), r.max(axis=0)


@functools.lru_cache(maxsize=None)
def _main():
    fx, Vf, mv, Vm = N.pair()
    return (fx, Vf, mv, Vm) + N.run(fx, Vf, mv, Vm, None, 2, (3, 2), 1.0)


def test_identical_volumes_give_a_zero_field_and_a_zero_cost():
    shape = (20, 17, 13)
    V = _axis_aligned()
    vol = N.scene(W.node_ras(V, shape), _box(V, shape))
    field, cost, count, _ = N.run(vol, V, vol, V, None, 2, (3, 2), 1.0)
    assert np.array_equal(field.view(np.uint32), np.zeros(field.shape, np.uint32))        # +0 everywhere, not merely small
    assert np.array_equal(cost, [[0, 0, 0], [0, 0, np.nan]], equal_nan=True)
    assert count[0, 0] == 10 * 9 * 7 and count[1, 0] == 20 * 17 * 13 and count[1, 2] == 0


def test_a_shift_is_recovered_with_the_right_sign():
    """moving(y) = scene(y - s): moving(x + s) = fixed(x), so d = +s, one voxel along x"""
    shape, V = (24, 20, 16), _axis_aligned()
    r, box = W.node_ras(V, shape), _box(V, shape)
    s = np.array([2.0, 0.0, 0.0])                                                       # one voxel
    field, cost, _, _ = N.run(N.scene(r, box), V, N.scene(r - s, box), V, None, 2, (20, 20), 1.0)
    dx = float(field[0][4:-4, 4:-4, 4:-4].mean())
    print("interior mean d_x = %.3f mm for a shift of %.1f mm; cost %.3g -> %.3g" % (dx, s[0], cost[0, 0], cost[1, 19]))
    assert dx > 0 and abs(dx - s[0]) < 0.5 * 2.0
    assert abs(float(field[1][4:-4, 4:-4, 4:-4].mean())) < 0.5 and abs(float(field[2][4:-4, 4:-4, 4:-4].mean())) < 0.5
    assert cost[1, 19] < cost[0, 0]


def phantom(n=24, seed=3):
    """a smooth n^3 volume in [0, 1]: an ellipsoid with an inner shell and a hole, plus low-pass noise"""
    k, j, i = np.meshgrid(*(np.arange(n, dtype=np.float64),) * 3, indexing="ij")
    c = (n - 1) / 2.0
    e = np.sqrt(((i - c) / (0.42 * n)) ** 2 + ((j - c) / (0.36 * n)) ** 2 + ((k - c) / (0.30 * n)) ** 2)
    soft = lambda x, w=0.15: 1.0 / (1.0 + np.exp(x / w))                                 # noqa: E731  (a smooth edge)
    v = 0.6 * soft(e - 1.0) + 0.3 * soft(e - 0.55) * (1 - soft(e - 0.35))
    hole = np.sqrt((i - c - 0.15 * n) ** 2 + (j - c + 0.1 * n) ** 2 + (k - c) ** 2) / (0.09 * n)
    v = v * (1 - 0.9 * soft(hole - 1.0, 0.3))
    noise = N.smooth(np.random.default_rng(seed).normal(size=(1, n, n, n)).astype(F), 2.0)[0].astype(np.float64)
    v = v + 0.1 * noise / np.abs(noise).max()
    return ((v - v.min()) / (v.max() - v.min())).astype(F)


@functools.lru_cache(maxsize=None)
def _quality(n=24, amp_vox=1.5):
    V = W.oblique_vox2ras((2.0, 2.0, 2.0))
    shape = (n, n, n)
    fixed = phantom(n)
    true = W.smooth_field(V, shape, amp_vox * 2.0)
    A, Q, B = W.volume_matrices(V, V, V)
    moving = W.warp_volume(true, A, Q, B, fixed[None], shape, shape, "trilinear", F(0))[0]
    field, cost, count, _ = N.run(fixed, V, moving, V, None, 2, (30, 30), 1.0)
    zero = np.zeros_like(field)
    before = N.moving_sample(zero, A, B, moving)
    after = N.moving_sample(field, A, B, moving)
    both = np.isfinite(before) & np.isfinite(after)
    mse0 = float(((fixed - before)[both].astype(np.float64) ** 2).mean())
    mse1 = float(((fixed - after)[both].astype(np.float64) ** 2).mean())
    return mse0, mse1, float(N.jacobian(field, V).min()), int(both.sum())


def test_quality_condition_on_the_phantom():
    """The condition of the issue, not a tolerance: on a smooth 24^3 phantom moved through warp_ref.smooth_field of 1.5 voxels, with
    sigma = 1, two levels and niter = (30, 30), the mean squared difference over the voxels present before and after falls at least
    10 x and the smallest Jacobian determinant stays > 0.  Measured: DESIGN.md §5."""
    mse0, mse1, jmin, nboth = _quality()
    print("MSE %.4g -> %.4g (%.1f x) over %d voxels; min det J = %.3f" % (mse0, mse1, mse0 / mse1, nboth, jmin))
    assert mse0 / mse1 >= 10.0
    assert jmin > 0.0


@pytest.mark.parametrize("mutant", N.MUTANTS)
def test_every_mutant_changes_an_output_bit(mutant):
    fx, Vf, mv, Vm, field, cost, count, _ = _main()
    fm, cm, nm, _ = N.run(fx, Vf, mv, Vm, None, 2, (3, 2), 1.0, mutant=mutant)
    assert not np.array_equal(fm.view(np.uint32), field.view(np.uint32))


def test_the_main_case_uses_every_branch():
    """absent samples at both levels, costs that fall, every face and the interior of the difference rule"""
    fx, Vf, mv, Vm, field, cost, count, _ = _main()
    assert 0 < count[0, 0] < 10 * 9 * 7 and 0 < count[1, 0] < 20 * 17 * 13
    assert cost[0, 2] < cost[0, 0] and cost[1, 1] < cost[1, 0] and np.isnan(cost[1, 2])
    assert np.isfinite(field).all() and np.abs(field).max() > 0.1


def test_dif_on_faces_interior_and_a_size_one_axis():
    a = np.array([[[1.0, 4.0, 9.0, 16.0]]], F)
    assert np.array_equal(N.dif(a, 2), [[[3.0, 4.0, 6.0, 7.0]]])
    assert np.array_equal(N.dif(a, 0), np.zeros_like(a)) and np.array_equal(N.dif(a, 1), np.zeros_like(a))
    assert np.array_equal(N.dif(np.array([2.0, 5.0], F), 0), [3.0, 3.0])
    assert np.array_equal(N.dif(np.full((1, 1, 3), np.nan, F), 0), np.zeros((1, 1, 3), F))    # 0, not NaN


def test_taps_sum_to_one_and_smoothing_keeps_a_constant():
    for sigma, r in ((0.5, 2), (1.0, 3), (4.0, 12)):
        rr, w = N.taps(sigma)
        assert rr == r and w.size == 2 * r + 1 and abs(float(w.astype(np.float64).sum()) - 1) < (2 * r + 1) * 2.0 ** -24
        assert np.array_equal(w, w[::-1])
    f = np.full((3, 5, 6, 7), 1.25, F)
    assert np.abs(N.smooth(f, 1.0) - f).max() <= 3 * 7 * 1.25 * 2.0 ** -23
    assert N.smooth(f, 0.0) is not f and np.array_equal(N.smooth(f, 0.0), f)


def test_upsampling_a_constant_and_a_ramp():
    """q = 0.5 y - 0.25: a constant stays, a ramp along x is sampled at those positions and the clamp holds the ends"""
    coarse = np.zeros((3, 4, 5, 7), F)
    coarse[0] = 2.5
    coarse[1] = np.arange(7, dtype=F)[None, None, :]
    up = N.upsample(coarse, (13, 9, 8))
    assert np.array_equal(up[0], np.full((8, 9, 13), 2.5, F)) and np.array_equal(up[2], np.zeros((8, 9, 13), F))
    want = np.clip(0.5 * np.arange(13) - 0.25, 0, 6).astype(F)
    assert np.array_equal(up[1][3, 4], want)


def test_jacobian_of_an_affine_field():
    """d = (L - I) x + t has I + dd/dx = L everywhere, faces included (the one-sided differences of a linear function are exact up to
    rounding).  The bound, from the operation count: a field value carries |d| u (u = 2^-24); a difference of two of them 2 |d| u (the
    0.5 is exact); G sums three products with |Linv| <= a, each operand and operation rounded: 3 a (2 |d| u) + 3 a |D| 4 u; the
    determinant has 9 entries with cofactors below 2 M^2 (M = max |J|) and 14 operations on terms below M^3."""
    V = W.oblique_vox2ras((2.0, 2.0, 2.0), origin=(-20.0, -16.0, -12.0))
    shape = (20, 17, 13)
    L = np.eye(3) + np.array([[0.05, -0.03, 0.02], [0.04, -0.06, 0.01], [-0.02, 0.03, 0.07]])
    d32, d64 = W.affine_field(V, shape, L, (0.5, -0.25, 0.125))
    det = N.jacobian(d32, V)
    u = 2.0 ** -24
    dmax, a = float(np.abs(d64).max()), float(np.abs(N.jacobian_matrix(V)).max())
    Dmax = float(np.abs(L - np.eye(3)).max()) * 2.0 * np.sqrt(3.0)                       # |dd_c / dvox_k| <= |L - I| |voxel edge|
    errG = 3 * a * 2 * dmax * u + 3 * a * Dmax * 4 * u
    M = 1.0 + float(np.abs(L - np.eye(3)).max()) + errG
    bound = 9 * 2 * M * M * errG + 14 * u * M ** 3
    err = float(np.abs(det.astype(np.float64) - np.linalg.det(L)).max())
    print("det(L) = %.6f, max error %.3g, bound %.3g (%.0f ulp of 1)" % (np.linalg.det(L), err, bound, bound / 2.0 ** -23))
    assert err <= bound
    assert bound < 1e-4


def test_jacobian_marks_a_fold():
    """d_x = -1.5 x inside a slab folds space there (det = 1 - 1.5 < 0) and nowhere else"""
    V = _axis_aligned(1.0, (0.0, 0.0, 0.0))
    shape = (12, 5, 4)
    x = W.node_ras(V, shape)[..., 0]
    d = np.zeros((3,) + x.shape, F)
    d[0] = (-1.5 * np.clip(x - 4.0, 0.0, 3.0)).astype(F)
    det = N.jacobian(d, V)
    assert (det[:, :, 5:7] < 0).all() and (det[:, :, :4] == 1).all() and (det[:, :, 8:] == 1).all()


# ---- the library's host code against the restatement (needs the built library, no GPU) -----------------------------------------------
def test_level_matrices_of_the_library_match(fj):
    fx, Vf, mv, Vm = N.pair()
    for post in (None, N.rigid()):
        for level in (0, 1, 2):
            got = fj.nlreg.nlreg_level(Vf, Vm, post, level, 1.7)
            want = N.level_matrices(Vf, Vm, post, level, 1.7)
            for g, w in zip(got, want):
                assert np.array_equal(np.asarray(g, F).view(np.uint32), np.asarray(w, F).view(np.uint32))
    with pytest.raises(fj.FibersError):
        fj.nlreg.nlreg_level(Vf, Vm, None, 0, 0.0)
    with pytest.raises(fj.FibersError):
        fj.nlreg.nlreg_level(np.zeros((4, 4), F), Vm, None, 0, 1.0)


def test_python_layer_refusals_need_no_gpu(fj):
    vol = np.ones((8, 8, 8, 4), F)
    vol[0, 0, 0] = 0
    with pytest.raises(ValueError, match="frame"):
        fj.mri_nlreg(fj.MRI(vol), fj.MRI(vol[..., 0]))
    with pytest.raises(ValueError, match="niter"):
        fj.mri_nlreg(fj.MRI(vol[..., 0]), fj.MRI(vol[..., 0]), levels=2, niter=(3, 2, 1))
    with pytest.raises(ValueError, match="niter"):
        fj.mri_nlreg(fj.MRI(vol[..., 0]), fj.MRI(vol[..., 0]), levels=2, niter=(3, -1))
    with pytest.raises(ValueError):
        fj.Warp(fj.MRI(vol))
