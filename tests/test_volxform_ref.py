"""CPU tests (no GPU): the NumPy restatement of the volume resampling contract (tests/volxform_ref.py), which the GPU tests compare
against bit for bit, is itself pinned on cases known by hand; so are the two pure-NumPy helpers of the package, xfm_header and
vol_xform_matrix."""
import numpy as np
import pytest

import volxform_ref as R

F = np.float32


def _shift(dx, dy=0.0, dz=0.0):
    A = np.eye(4, dtype=F)
    A[:3, 3] = (dx, dy, dz)
    return A


def _values(shape, seed=0):
    nx, ny, nz = shape
    return (np.random.default_rng(seed).standard_normal((nz, ny, nx)) * 100).astype(F)


def test_nearest_pure_shift_moves_the_volume_in_the_transforms_direction():
    """vox2vox = shift by (+2, 0, 0): input voxel i lands on output voxel i + 2.  A transform applied in the wrong direction (which
    a restatement shared with the kernel could not show) would move the volume the other way."""
    shape = (7, 5, 3)
    v = _values(shape)
    out = R.vol_xform_ref(R.out2in(_shift(2.0)), v, shape, shape, "nearest", F(-1))[0]
    assert np.array_equal(out[:, :, 2:].view(np.uint32), v[:, :, :-2].view(np.uint32))
    assert np.all(out[:, :, :2] == F(-1))


def test_nearest_ties_go_to_even_also_at_the_far_border():
    """shift by half a voxel: every coordinate is a tie.  p = o - 0.5 -> o = 7: p = 6.5, voxel 6 (n = 7); o = 6 with n = 6: p = 5.5
    rounds to 6, outside; o = 0: p = -0.5 rounds to -0.0, voxel 0."""
    for n in (7, 6):
        shape, oshape = (n, 1, 1), (n + 2, 1, 1)
        v = np.arange(10, 10 + n, dtype=np.int32).reshape(1, 1, n)
        out = R.vol_xform_ref(R.out2in(_shift(0.5)), v, shape, oshape, "nearest", np.int32(-7))[0, 0, 0]
        # p = o - 0.5 for o = 0 .. n + 1: rint (ties to even) = -0, 0, 2, 2, 4, 4, 6, 6, 8
        want_vox = [0, 0, 2, 2, 4, 4, 6, 6, 8][: n + 2]
        want = [10 + q if q <= n - 1 else -7 for q in want_vox]
        assert out.tolist() == want, (n, out.tolist(), want)
    # the three cases the contract names
    v7 = np.arange(10, 17, dtype=np.int32).reshape(1, 1, 7)
    o7 = R.vol_xform_ref(R.out2in(_shift(0.5)), v7, (7, 1, 1), (9, 1, 1), "nearest", np.int32(-7))[0, 0, 0]
    assert o7[7] == 16 and o7[0] == 10                      # p = 6.5 -> voxel 6; p = -0.5 -> voxel 0
    v6 = np.arange(10, 16, dtype=np.int32).reshape(1, 1, 6)
    o6 = R.vol_xform_ref(R.out2in(_shift(0.5)), v6, (6, 1, 1), (8, 1, 1), "nearest", np.int32(-7))[0, 0, 0]
    assert o6[6] == -7                                       # p = 5.5 -> 6: outside for n = 6


def test_nearest_identity_is_the_input_bit_for_bit():
    shape = (7, 5, 3)
    v = _values(shape)
    bits = v.view(np.uint32).copy()
    bits[0, 0, 0], bits[1, 2, 3], bits[2, 4, 6] = 0x7FC00001, 0xFFC12345, 0x7F800001      # quiet and signalling NaNs with payloads
    v = bits.view(F)
    out = R.vol_xform_ref(np.eye(4, dtype=F), v, shape, shape, "nearest", F(0))[0]
    assert np.array_equal(out.view(np.uint32), bits)
    lab = np.random.default_rng(1).integers(-2 ** 31, 2 ** 31 - 1, (2, 3, 5, 7)).astype(np.int32)
    out = R.vol_xform_ref(np.eye(4, dtype=F), lab, shape, shape, "nearest", np.int32(0))
    assert out.dtype == np.int32 and np.array_equal(out, lab)


def test_trilinear_identity_is_the_input_bit_for_bit():
    shape = (7, 5, 3)
    v = _values(shape, 3)
    out = R.vol_xform_ref(np.eye(4, dtype=F), v, shape, shape, "trilinear", F(0))[0]
    assert np.array_equal(out.view(np.uint32), v.view(np.uint32))


def _ramp_check(M, inshape, outshape, coef):
    """max of |out - ramp64(M o)| / (2^-23 S) over the output voxels whose p lies in [0, n - 1]^3, and the three classes"""
    a, b, c, d = coef
    nx, ny, nz = inshape
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    vol = (a * i + b * j + c * k + d).astype(F)
    out = R.vol_xform_ref(M, vol, inshape, outshape, "trilinear", F(np.nan))[0]
    ox, oy, oz = outshape
    K, J, I = np.meshgrid(np.arange(oz), np.arange(oy), np.arange(ox), indexing="ij")
    m = np.asarray(M, F).astype(np.float64)
    o = np.stack([I, J, K, np.ones_like(I)]).reshape(4, -1).astype(np.float64)
    q = m @ o
    p = (q[:3] / q[3]).reshape(3, oz, oy, ox)
    interior = np.ones(p[0].shape, bool)
    for comp, n in zip(p, inshape):
        interior &= (comp >= 0) & (comp <= n - 1)
    inside = R.inside_mask(R.pull_back(M, outshape), inshape)
    assert not np.any(interior & ~inside)
    assert np.all(np.isnan(out[~inside])) and not np.any(np.isnan(out[inside]))
    S = abs(a) * nx + abs(b) * ny + abs(c) * nz + abs(d)
    want = a * p[0] + b * p[1] + c * p[2] + d
    err = np.abs(out.astype(np.float64) - want)[interior].max() / (2.0 ** -23 * S)
    return err, int(inside.sum()), int((inside & ~interior).sum()), int((~inside).sum())


def test_trilinear_reproduces_a_linear_ramp_under_an_oblique_transform():
    """|out - ramp64(M o)| <= 16 * 2^-23 * S with S = |a| nx + |b| ny + |c| nz + |d|: about 6 roundings in the coordinates and 7 in
    the lerps, doubled.  Inside, clamped-shell and outside voxels must all occur, so that none is silently skipped."""
    err, n_inside, n_shell, n_outside = _ramp_check(R.out2in(R.oblique()), (7, 5, 3), (9, 6, 4), (1.5, -2.25, 3.0, 10.0))
    print("ramp 7x5x3 -> 9x6x4: max error %.3f x 2^-23 S; inside %d (clamped shell %d), outside %d" % (err, n_inside, n_shell, n_outside))
    assert n_inside > n_shell > 0 and n_outside > 0 and n_inside + n_outside == 9 * 6 * 4
    assert (n_inside, n_shell, n_outside) == (158, 63, 58)
    assert err <= 16.0


def test_trilinear_ramp_bound_over_random_rotations():
    """the same bound over 20 random rotations of 40 x 33 x 21 grids (the restatement itself stays below 2 * 2^-23 * S on them; the figure is printed)"""
    rng = np.random.default_rng(7)
    worst = 0.0
    for _ in range(20):
        Q, _r = np.linalg.qr(rng.standard_normal((3, 3)))
        A = np.eye(4)
        A[:3, :3] = Q * rng.uniform(0.8, 1.25)
        c_in = (np.array([40, 33, 21]) - 1) / 2
        A[:3, 3] = c_in - A[:3, :3] @ c_in + rng.uniform(-2, 2, 3)          # about the grid's centre, plus a shift
        err, n_inside, _s, _o = _ramp_check(A.astype(F), (40, 33, 21), (40, 33, 21), tuple(rng.uniform(-3, 3, 4)))
        assert n_inside > 1000
        worst = max(worst, err)
    print("worst ramp error over 20 rotations: %.3f x 2^-23 S" % worst)
    assert worst <= 16.0


def _hdr(shape, res, fj):
    """an oblique header with the same field of view for every (shape, res) of equal extent: the corner of voxel (-1/2, -1/2, -1/2)
    is fixed"""
    az = np.deg2rad(12.0)
    Rm = np.array([[np.cos(az), -np.sin(az), 0], [np.sin(az), np.cos(az), 0], [0, 0, 1]])
    M = np.eye(4)
    M[:3, :3] = Rm * res
    M[:3, 3] = np.array([-20.0, 13.0, 5.5]) + M[:3, :3] @ np.full(3, 0.5)
    return fj.MRI(np.zeros(shape, F), volres=(res,) * 3, vox2ras=M.astype(F))


def test_xfm_header_between_two_grids_of_one_field_of_view(fj):
    lo, hi = _hdr((4, 3, 2), 2.0, fj), _hdr((8, 6, 4), 1.0, fj)
    x = fj.xfm_header(lo, hi)
    assert tuple(x.insize) == (4, 3, 2) and tuple(x.outsize) == (8, 6, 4)
    assert np.array_equal(x.inres, np.full(3, 2, F)) and np.array_equal(x.outres, np.ones(3, F))
    assert np.array_equal(x.invox2ras, lo.vox2ras) and np.array_equal(x.outvox2ras, hi.vox2ras) and np.array_equal(x.ras2ras, np.eye(4, dtype=F))
    # a 2 mm voxel i covers the 1 mm voxels 2 i and 2 i + 1: its centre lies at 2 i + 1/2
    want = np.diag([2.0, 2.0, 2.0, 1.0])
    want[:3, 3] = 0.5
    assert x.vox2vox.dtype == F and np.allclose(x.vox2vox, want, atol=1e-5)
    assert np.allclose(x.voxrot, np.eye(3), atol=1e-6)
    # float32(inv(outref) @ inref) in float64, rounded once
    assert np.array_equal(x.vox2vox, (np.linalg.inv(hi.vox2ras.astype(np.float64)) @ lo.vox2ras.astype(np.float64)).astype(F))


def test_xfm_header_of_a_volume_with_itself_is_the_identity(fj):
    ref = _hdr((7, 5, 3), 2.0, fj)
    x = fj.xfm_header(ref, ref)
    M = fj.vol_xform_matrix(x)
    assert M.dtype == F and M.shape == (4, 4)
    assert np.allclose(x.vox2vox, np.eye(4), atol=1e-6)
    # whatever rounding inv(A) @ A leaves is far below half a voxel: both interpolations of the restatement return the volume
    v = _values((7, 5, 3), 5)
    out = R.vol_xform_ref(M, v, (7, 5, 3), (7, 5, 3), "nearest", F(0))[0]
    assert np.array_equal(out.view(np.uint32), v.view(np.uint32))
    if np.array_equal(M, np.eye(4, dtype=F)):
        out = R.vol_xform_ref(M, v, (7, 5, 3), (7, 5, 3), "trilinear", F(0))[0]
        assert np.array_equal(out.view(np.uint32), v.view(np.uint32))


def test_vol_xform_matrix_is_the_rounded_float64_inverse_and_refuses_a_singular_matrix(fj):
    x = fj.Xform(insize=(7, 5, 3), outsize=(9, 6, 4), vox2vox=R.oblique())
    assert np.array_equal(fj.vol_xform_matrix(x), R.out2in(R.oblique()))
    x.vox2vox = np.diag([1, 1, 0, 1]).astype(F)
    with pytest.raises(ValueError, match="singular"):
        fj.vol_xform_matrix(x)
