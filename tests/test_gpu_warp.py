"""Non-linear warps on the GPU (fibd_warp_pack / _points / _volume / _invert, their host forms, str_warp / mri_warp / warp_invert), bit
for bit against the NumPy restatement (tests/warp_ref.py, pinned on the CPU by tests/test_warp_ref.py) over every point and every voxel:
the pack and its views, point counts around the workgroup size, in place, 4-byte-aligned views on a side stream, points beyond every
face, NaN and Inf points, projective matrices, fields of one voxel and of one plane, volumes both ways under both interpolations, the
inverse and its tie to the points kernel, the host forms under every chunking, the road from `stream` to a connectome in template space,
the refused arguments and the device tier's argument contract.  Shapes are a few hundred voxels and a few thousand points: the file
runs in seconds.  In-process only.

"Bit for bit" leaves one thing open: which NaN.  Where the restatement gives a NaN the kernel must give a NaN, of any payload (NumPy's
Inf - Inf and the GPU's differ in the sign bit); every other value is compared as a 32-bit pattern."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import volxform_ref as V  # noqa: E402
import warp_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

F = np.float32
FIB_ERR_INVALID, FIB_ERR_UNSUPPORTED = -1, -7
FSHAPE, FRES = (9, 8, 7), (2.0, 2.0, 2.5)
FV2R = R.oblique_vox2ras(FRES)
SMALL, LARGE = (7, 5, 3), (9, 6, 4)
GRID = {SMALL: R.oblique_vox2ras((2.6, 3.2, 5.0), angles_deg=(12.0, 4.0), origin=(-8.0, 5.0, -3.0)),
        LARGE: R.oblique_vox2ras((2.0, 2.6, 3.6), angles_deg=(27.0, 14.0), origin=(-6.0, 4.0, -5.0))}
OSHAPE = (10, 9, 8)
OV2R = R.oblique_vox2ras((1.8, 1.8, 1.8), angles_deg=(-12.0, 7.0), origin=(-9.0, 3.0, -5.0))
IN_V2R = R.oblique_vox2ras((1.5, 1.5, 2.0), angles_deg=(-25.0, 8.0), origin=(-4.0, 9.0, -6.0))      # the tract volume of the point tests
OUT_V2R = R.oblique_vox2ras((1.25, 1.25, 1.25), angles_deg=(15.0, -6.0), origin=(-10.0, 2.0, -8.0))
EYE = np.eye(4, dtype=F)


def _same_bits(got, want):
    """equal 32-bit patterns, except that any NaN answers a NaN"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    if got.dtype != F:
        return np.array_equal(got, want)
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])


def _rigid(seed):
    rng = np.random.default_rng(seed)
    a = np.deg2rad(rng.uniform(-15, 15))
    M = np.eye(4)
    M[:3, :3] = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    M[:3, 3] = rng.uniform(-3, 3, 3)
    return M.astype(F)


PRE, POST = _rigid(1), _rigid(2)


def _projective(M):
    """a matrix whose last row is not 0 0 0 1 (the last row of the volxform tests' _projective())"""
    M = np.array(M, F)
    M[3] = (0.002, -0.001, 0.0015, 1.0)
    return M


def _points(n, seed, lo=-0.3, hi=1.3, shape=FSHAPE, origin=1):
    """n caller points (float32) whose field-voxel coordinates spread over [lo, hi] x the grid: inside it and beyond every face"""
    rng = np.random.default_rng(seed)
    q = rng.uniform(lo, hi, (n, 3)) * (np.array(shape) - 1)
    to_ras = R.point_matrices(FV2R, IN_V2R, OUT_V2R, PRE, POST, origin, ft=np.float64)[0]
    x = q @ FV2R.astype(np.float64)[:3, :3].T + FV2R.astype(np.float64)[:3, 3]
    return ((x - to_ras[:3, 3]) @ np.linalg.inv(to_ras[:3, :3]).T).astype(F)


@pytest.fixture(scope="module")
def torch_():
    import torch
    return torch


@pytest.fixture(scope="module")
def W(fj):
    from fibers_jl_amd import warp
    return warp


@pytest.fixture(scope="module")
def world(W, torch_):
    """the smooth field (amp 2) on the 9 x 8 x 7 grid, packed on the device once, and the matrices of the point tests"""
    field = R.smooth_field(FV2R, FSHAPE, 2.0)
    w = dict(field=field, mats=R.point_matrices(FV2R, IN_V2R, OUT_V2R, PRE, POST, 1))
    w["packed"] = _pack(W, torch_, field)
    torch_.cuda.synchronize()
    return w


def _shape(field):
    return field.shape[:0:-1]                                          # [3, nz, ny, nx] -> (nx, ny, nz)


def _pack(W, torch, field):
    return W.warp_pack_device(torch.from_numpy(np.ascontiguousarray(field).reshape(3, -1)).cuda(), _shape(field))


def _dev_points(W, torch, packed, shape, mats, p, **kw):
    out = W.warp_points_device(packed, shape, *mats, torch.from_numpy(np.ascontiguousarray(p)).cuda(), **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy()


# ---- pack ---------------------------------------------------------------------------------------------------------------------------
def test_pack_and_its_views(W, torch_, world):
    torch = torch_
    field = world["field"]
    nvox = field[0].size
    want = np.concatenate([field.reshape(3, -1).T, np.zeros((nvox, 1), F)], axis=1)
    assert tuple(world["packed"].shape) == (nvox, 4) and _same_bits(world["packed"].cpu().numpy(), want)
    # the planar field one element into a buffer (4 bytes off), the packed field 16 bytes into one, on a side stream
    src = torch.zeros(3 * nvox + 1, dtype=torch.float32, device="cuda")
    src[1:] = torch.from_numpy(field.reshape(-1)).cuda()
    dst = torch.full((4 * nvox + 8,), 123.0, dtype=torch.float32, device="cuda")
    vin, vout = src[1:].view(3, nvox), dst[4:4 + 4 * nvox].view(nvox, 4)
    assert vin.data_ptr() % 16 == 4 and vout.data_ptr() % 16 == 0
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    got = W.warp_pack_device(vin, FSHAPE, out=vout, stream=side)
    side.synchronize()
    assert got.data_ptr() == vout.data_ptr() and _same_bits(got.cpu().numpy(), want)
    assert torch.all(dst[:4] == 123.0).item() and torch.all(dst[-4:] == 123.0).item()     # nothing written outside the view
    from fibers_jl_amd._dev import ArgError
    with pytest.raises(ArgError, match="16-byte"):
        W.warp_pack_device(vin, FSHAPE, out=dst[1:1 + 4 * nvox].view(nvox, 4))


# ---- points -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 3, 4, 5, 255, 256, 257, 4099])
def test_points_at_counts_around_the_workgroup(W, torch_, world, n):
    p = _points(n, 100 + n)
    want = R.warp_points(world["field"], *world["mats"], p)
    got = _dev_points(W, torch_, world["packed"], FSHAPE, world["mats"], p)
    assert got.shape == (n, 3) and _same_bits(got, want)
    if n >= 255:
        q = R.xfm_point(world["mats"][1], p)
        for c, top in enumerate(FSHAPE):
            assert (q[:, c] < 0).any() and (q[:, c] > top - 1).any()    # beyond both faces of every axis
        assert ((q >= 0) & (q <= np.array(FSHAPE, F) - 1)).all(axis=1).any()


def test_points_in_place_and_as_a_flat_vector(W, torch_, world):
    torch = torch_
    p = _points(1000, 3)
    want = R.warp_points(world["field"], *world["mats"], p)
    d = torch.from_numpy(p.reshape(-1)).cuda()
    out = W.warp_points_device(world["packed"], FSHAPE, *world["mats"], d, out=d)
    torch.cuda.synchronize()
    assert out.data_ptr() == d.data_ptr() and tuple(out.shape) == (3000,)
    assert _same_bits(d.cpu().numpy().reshape(-1, 3), want)


def test_points_in_a_view_four_bytes_off_on_a_side_stream(W, torch_, world):
    torch = torch_
    p = _points(1000, 4)
    want = R.warp_points(world["field"], *world["mats"], p)
    src = torch.zeros(3001, dtype=torch.float32, device="cuda")
    src[1:] = torch.from_numpy(p.reshape(-1)).cuda()
    dst = torch.full((3003,), 123.0, dtype=torch.float32, device="cuda")
    vin, vout = src[1:], dst[2:3002]
    assert vin.data_ptr() % 16 == 4 and vout.data_ptr() % 16 == 8
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    got = W.warp_points_device(world["packed"], FSHAPE, *world["mats"], vin, out=vout, stream=side)
    side.synchronize()
    assert got.data_ptr() == vout.data_ptr() and _same_bits(got.cpu().numpy().reshape(-1, 3), want)
    assert torch.all(dst[:2] == 123.0).item() and dst[-1].item() == 123.0


def test_points_beyond_every_face_get_the_edge_displacement(W, torch_, world):
    """with identity matrices the points are field-voxel coordinates: far beyond a face the result is the point plus the face's node"""
    field = world["field"]
    nx, ny, nz = FSHAPE
    q = np.array([[-5.0, 3.0, 2.0], [40.0, 3.0, 2.0], [4.0, -9.5, 2.0], [4.0, 70.0, 2.0], [4.0, 3.0, -1.5], [4.0, 3.0, 33.0],
                  [-1e6, 1e6, -0.0], [nx - 1.0, ny - 1.0, nz - 1.0]], F)
    node = [(0, 3, 2), (nx - 1, 3, 2), (4, 0, 2), (4, ny - 1, 2), (4, 3, 0), (4, 3, nz - 1), (0, ny - 1, 0), (nx - 1, ny - 1, nz - 1)]
    got = _dev_points(W, torch_, world["packed"], FSHAPE, (EYE, EYE, EYE), q)
    assert _same_bits(got, R.warp_points(field, EYE, EYE, EYE, q))
    for row, (i, j, k) in zip(range(len(q)), node):
        assert np.array_equal(got[row], q[row] + field[:, k, j, i]), row


def test_nan_and_inf_points(W, torch_, world):
    p = _points(64, 5)
    p[::7, 0] = np.nan
    p[1::7, 1] = np.inf
    p[2::7, 2] = -np.inf
    p[3::7] = np.nan
    for mats in (world["mats"], (EYE, EYE, EYE)):
        want = R.warp_points(world["field"], *mats, p)
        assert np.isnan(want).any() and np.isfinite(want).any()
        assert _same_bits(_dev_points(W, torch_, world["packed"], FSHAPE, mats, p), want)
    # +-Inf field coordinates clamp: finite points through a to_field that overflows (an Inf POINT is NaN already in xfm_point: 0 * Inf)
    huge = np.diag([3e38, 3e38, 3e38, 1.0]).astype(F)
    p = np.array([[2.0, 3.0, 2.0], [-2.0, 3.0, 2.0], [2.0, -3.0, 2.0], [2.0, 2.0, -2.0], [-2.0, -2.0, -2.0]], F)
    assert np.isinf(R.xfm_point(huge, p)).all()
    want = R.warp_points(world["field"], EYE, huge, EYE, p)
    assert np.isfinite(want).all() and np.array_equal(want[0], p[0] + world["field"][:, 6, 7, 8])
    assert _same_bits(_dev_points(W, torch_, world["packed"], FSHAPE, (EYE, huge, EYE), p), want)


def test_projective_matrices(W, torch_, world):
    p = _points(2000, 6)
    mats = tuple(_projective(m) for m in world["mats"])
    want = R.warp_points(world["field"], *mats, p)
    assert not _same_bits(want, R.warp_points(world["field"], *world["mats"], p))
    assert _same_bits(_dev_points(W, torch_, world["packed"], FSHAPE, mats, p), want)


@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 8, 7), (9, 1, 7), (9, 8, 1)])
def test_fields_of_one_voxel_and_of_one_plane(W, torch_, shape):
    nx, ny, nz = shape
    field = (np.random.default_rng(7).standard_normal((3, nz, ny, nx)) * 2).astype(F)
    packed = _pack(W, torch_, field)
    q = (np.random.default_rng(8).uniform(-0.5, 1.5, (500, 3)) * np.maximum(np.array(shape) - 1, 2)).astype(F)
    want = R.warp_points(field, EYE, EYE, EYE, q)
    assert _same_bits(_dev_points(W, torch_, packed, shape, (EYE, EYE, EYE), q), want)


# ---- volume -------------------------------------------------------------------------------------------------------------------------
def _floats(nf, shape, seed):
    nx, ny, nz = shape
    return (np.random.default_rng(seed).standard_normal((nf, nz, ny, nx)) * 100).astype(F)


def _labels(nf, shape, seed):
    nx, ny, nz = shape
    return np.random.default_rng(seed).integers(-5, 2000, (nf, nz, ny, nx)).astype(np.int32)


def _vol_mats(inshape, outshape):
    """mri_warp's matrices for a volume on GRID[inshape] pulled onto GRID[outshape] through pre and post"""
    return R.volume_matrices(FV2R, GRID[outshape], GRID[inshape], PRE, POST)


def _inside(field, mats, inshape, outshape):
    nxo, nyo, nzo = outshape
    pw = R.warp_points(field, *mats, R.grid_points(outshape))
    return V.inside_mask([pw[:, c].reshape(nzo, nyo, nxo) for c in range(3)], inshape)


def _dev_volume(W, torch, packed, fshape, mats, vol, inshape, outshape, interp, outside, **kw):
    d = torch.from_numpy(np.ascontiguousarray(vol).reshape(vol.shape[0], -1)).cuda()
    out = W.warp_volume_device(packed, fshape, *mats, d, inshape, outshape, interp=interp, outside=outside, **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy().reshape((vol.shape[0],) + tuple(outshape)[::-1])


@pytest.mark.parametrize("nframes", [1, 3, 4, 5, 9])
@pytest.mark.parametrize("direction", ["up", "down"])
def test_volume_both_ways_under_both_interpolations(W, torch_, world, direction, nframes):
    """7 x 5 x 3 -> 9 x 6 x 4 and back through the 9 x 8 x 7 field: float32 under both interpolations, int32 labels under nearest;
    from 4 frames on the launch takes the kernel whose frame loop goes four at a time"""
    inshape, outshape = (SMALL, LARGE) if direction == "up" else (LARGE, SMALL)
    mats = _vol_mats(inshape, outshape)
    ok = _inside(world["field"], mats, inshape, outshape)
    assert 0 < ok.sum() < ok.size                                       # both branches of the inside test are taken
    v, lab = _floats(nframes, inshape, 2), _labels(nframes, inshape, 3)
    for interp in ("nearest", "trilinear"):
        want = R.warp_volume(world["field"], *mats, v, inshape, outshape, interp, F(np.nan))
        got = _dev_volume(W, torch_, world["packed"], FSHAPE, mats, v, inshape, outshape, interp, np.nan)
        assert _same_bits(got, want), interp
    want = R.warp_volume(world["field"], *mats, lab, inshape, outshape, "nearest", np.int32(-1))
    got = _dev_volume(W, torch_, world["packed"], FSHAPE, mats, lab, inshape, outshape, "nearest", -1)
    assert got.dtype == np.int32 and np.array_equal(got, want)


def _long_row_mats():
    """300 x 3 x 2 output voxels spanning an 11 x 4 x 3 volume that lies on the field's grid (as volxform's test, with the field between)"""
    A = np.eye(4)
    az = np.deg2rad(12.0)
    A[:3, :3] = np.array([[np.cos(az), -np.sin(az), 0], [np.sin(az), np.cos(az), 0], [0, 0, 1]]) * np.array([10.5 / 299, 1.1, 1.2])
    A[:3, 3] = (0.1, 0.4, 0.3)
    in_v2r = (FV2R.astype(np.float64) @ np.diag([0.8, 1.5, 2.0, 1.0])).astype(F)       # 11 x 4 x 3 voxels over the field's 9 x 8 x 7
    out_v2r = (in_v2r.astype(np.float64) @ A).astype(F)
    return R.volume_matrices(FV2R, out_v2r, in_v2r)


@pytest.mark.parametrize("interp", ["nearest", "trilinear"])
def test_volume_rows_longer_than_a_workgroup(W, torch_, world, interp):
    inshape, outshape = (11, 4, 3), (300, 3, 2)
    mats = _long_row_mats()
    ok = _inside(world["field"], mats, inshape, outshape)
    assert ok[:, :, 256:].any() and (~ok).any()                         # the second segment of a row holds inside voxels
    v = _floats(2, inshape, 6)
    want = R.warp_volume(world["field"], *mats, v, inshape, outshape, interp, F(-1))
    assert _same_bits(_dev_volume(W, torch_, world["packed"], FSHAPE, mats, v, inshape, outshape, interp, -1.0), want)


@pytest.mark.parametrize("interp", ["nearest", "trilinear"])
def test_volume_entirely_outside_and_nan_positions_give_the_fill(W, torch_, world, interp):
    inshape, outshape = SMALL, LARGE
    v = _floats(2, inshape, 8)
    far = np.eye(4, dtype=F)
    far[:3, 3] = (1e6, -1e30, 400.0)
    nan = np.eye(4, dtype=F)
    nan[:3, 3] = np.nan
    for to_ras, from_ras in ((EYE, far), (nan, EYE)):
        mats = (to_ras, EYE, from_ras)
        assert not _inside(world["field"], mats, inshape, outshape).any()
        got = _dev_volume(W, torch_, world["packed"], FSHAPE, mats, v, inshape, outshape, interp, 7.5)
        assert got.shape == (2, 4, 6, 9) and np.all(got == F(7.5))
        assert _same_bits(got, R.warp_volume(world["field"], *mats, v, inshape, outshape, interp, F(7.5)))


def test_zero_field_with_identity_matrices_returns_the_input(W, torch_):
    v, lab = _floats(3, SMALL, 9), _labels(1, SMALL, 10)
    zero = np.zeros((3, 2, 2, 2), F)
    packed = _pack(W, torch_, zero)
    assert _same_bits(_dev_volume(W, torch_, packed, (2, 2, 2), (EYE, EYE, EYE), v, SMALL, SMALL, "nearest", np.nan), v)
    assert np.array_equal(_dev_volume(W, torch_, packed, (2, 2, 2), (EYE, EYE, EYE), lab, SMALL, SMALL, "nearest", -1), lab)


def test_volume_views_on_a_side_stream_and_a_single_frame_vector(W, torch_, world):
    torch = torch_
    mats = _vol_mats(SMALL, LARGE)
    nvi, nvo = 7 * 5 * 3, 9 * 6 * 4
    v = _floats(3, SMALL, 11)
    want = R.warp_volume(world["field"], *mats, v, SMALL, LARGE, "trilinear", F(-1))
    src = torch.zeros(3 * nvi + 1, dtype=torch.float32, device="cuda")
    dst = torch.full((3 * nvo + 2,), 123.0, dtype=torch.float32, device="cuda")
    src[1:] = torch.from_numpy(v.reshape(-1)).cuda()
    vin, vout = src[1:].view(3, nvi), dst[1:1 + 3 * nvo].view(3, nvo)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    got = W.warp_volume_device(world["packed"], FSHAPE, *mats, vin, SMALL, LARGE, interp="trilinear", outside=-1.0, out=vout, stream=side)
    side.synchronize()
    assert got.data_ptr() == vout.data_ptr() and _same_bits(got.cpu().numpy().reshape(want.shape), want)
    assert dst[0].item() == 123.0 and dst[-1].item() == 123.0
    one = W.warp_volume_device(world["packed"], FSHAPE, *mats, torch.from_numpy(v[0].reshape(-1)).cuda(), SMALL, LARGE, outside=-1.0)
    assert tuple(one.shape) == (nvo,) and _same_bits(one.cpu().numpy().reshape(want.shape[1:]), want[0])


# ---- inverse ------------------------------------------------------------------------------------------------------------------------
def _dev_invert(W, torch, packed, fshape, Y, Q, outshape, niter, **kw):
    inv, err = W.warp_invert_device(packed, fshape, Y, Q, outshape, niter=niter, **kw)
    torch.cuda.synchronize()
    nxo, nyo, nzo = outshape
    return inv.cpu().numpy().reshape(3, nzo, nyo, nxo), None if err is None else err.cpu().numpy().reshape(nzo, nyo, nxo)


@pytest.mark.parametrize("niter", [0, 1, 20])
def test_inverse_of_the_smooth_field(W, torch_, world, niter):
    Y, Q = R.invert_matrices(FV2R, OV2R)
    want_inv, want_err = R.invert(world["field"], Y, Q, OSHAPE, niter)
    inv, err = _dev_invert(W, torch_, world["packed"], FSHAPE, Y, Q, OSHAPE, niter)
    assert _same_bits(inv, want_inv) and _same_bits(err, want_err)
    if niter == 0:
        assert not inv.any()
    if niter == 20:
        assert err.max() <= 4 * R.ulp32(np.abs(R.xfm_point(Y, R.grid_points(OSHAPE))).max())
    only, none = _dev_invert(W, torch_, world["packed"], FSHAPE, Y, Q, OSHAPE, niter, err=False)       # err NULL
    assert none is None and _same_bits(only, want_inv)


def test_inverse_of_a_folding_field(W, torch_):
    field = R.smooth_field(FV2R, FSHAPE, 12.0)
    Y, Q = R.invert_matrices(FV2R, OV2R)
    want_inv, want_err = R.invert(field, Y, Q, OSHAPE, 20)
    inv, err = _dev_invert(W, torch_, _pack(W, torch_, field), FSHAPE, Y, Q, OSHAPE, 20)
    assert _same_bits(inv, want_inv) and _same_bits(err, want_err)
    assert err.max() > 0.1


def test_the_points_kernel_undoes_the_inverse(W, torch_, world):
    """x = y + inv(y) at the output nodes through the points kernel and a pack of the original field returns y within the err the
    call reported plus one ulp of the coordinates"""
    Y, Q = R.invert_matrices(FV2R, OV2R)
    inv, err = _dev_invert(W, torch_, world["packed"], FSHAPE, Y, Q, OSHAPE, 20)
    y = R.xfm_point(Y, R.grid_points(OSHAPE))
    x = (y + inv.reshape(3, -1).T).astype(F)
    back = _dev_points(W, torch_, world["packed"], FSHAPE, (EYE, Q, EYE), x)
    dev = np.abs(back - y).max(axis=1)
    assert (dev <= err.reshape(-1) + R.ulp32(np.abs(y).max())).all(), float((dev - err.reshape(-1)).max())


# ---- host forms ---------------------------------------------------------------------------------------------------------------------
def _m16(m):
    return (C.c_float * 16)(*np.ascontiguousarray(m, F).reshape(-1).tolist())


@pytest.mark.parametrize("chunk", ["1", "7", None])
def test_host_points_under_every_chunking(fj, W, torch_, world, monkeypatch, chunk):
    if chunk is None:
        monkeypatch.delenv("FIBERS_WARP_POINTS", raising=False)
    else:
        monkeypatch.setenv("FIBERS_WARP_POINTS", chunk)
    p = _points(300, 12)
    dev = _dev_points(W, torch_, world["packed"], FSHAPE, world["mats"], p)
    assert _same_bits(dev, R.warp_points(world["field"], *world["mats"], p))
    field = np.ascontiguousarray(world["field"])
    out = np.full_like(p, 9.0)
    A, Q, B = (_m16(m) for m in world["mats"])
    assert fj.lib().fib_warp_points(0, field.ctypes.data, 9, 8, 7, A, Q, B, p.ctypes.data, out.ctypes.data, 300) == 0
    assert out.tobytes() == dev.tobytes()
    work = p.copy()                                                    # in place
    assert fj.lib().fib_warp_points(0, field.ctypes.data, 9, 8, 7, A, Q, B, work.ctypes.data, work.ctypes.data, 300) == 0
    assert work.tobytes() == dev.tobytes()
    assert fj.lib().fib_warp_points(0, field.ctypes.data, 9, 8, 7, A, Q, B, None, None, 0) == 0


@pytest.mark.parametrize("frames", ["1", "2", None])
def test_host_volume_under_every_chunking(fj, W, torch_, world, monkeypatch, frames):
    if frames is None:
        monkeypatch.delenv("FIBERS_WARP_FRAMES", raising=False)
    else:
        monkeypatch.setenv("FIBERS_WARP_FRAMES", frames)
    mats = _vol_mats(SMALL, LARGE)
    v = _floats(5, SMALL, 13)
    field = np.ascontiguousarray(world["field"])
    A, Q, B = (_m16(m) for m in mats)
    for interp, code in (("nearest", 0), ("trilinear", 1)):
        dev = _dev_volume(W, torch_, world["packed"], FSHAPE, mats, v, SMALL, LARGE, interp, -1.0)
        assert _same_bits(dev, R.warp_volume(world["field"], *mats, v, SMALL, LARGE, interp, F(-1)))
        out = np.zeros((5, 4, 6, 9), F)
        bits = int(np.array([-1.0], F).view(np.int32)[0])
        assert fj.lib().fib_warp_volume(0, field.ctypes.data, 9, 8, 7, A, Q, B, v.ctypes.data, 7, 5, 3, 5, code, bits, out.ctypes.data, 9, 6, 4) == 0
        assert out.tobytes() == dev.tobytes(), interp


def test_host_invert_equals_the_device_form(fj, W, torch_, world):
    Y, Q = R.invert_matrices(FV2R, OV2R)
    field = np.ascontiguousarray(world["field"])
    for niter in (0, 20):
        dinv, derr = _dev_invert(W, torch_, world["packed"], FSHAPE, Y, Q, OSHAPE, niter)
        inv, err = np.zeros((3, 8, 9, 10), F), np.zeros((8, 9, 10), F)
        assert fj.lib().fib_warp_invert(0, field.ctypes.data, 9, 8, 7, _m16(Y), _m16(Q), niter, inv.ctypes.data, err.ctypes.data, 10, 9, 8) == 0
        assert inv.tobytes() == dinv.tobytes() and err.tobytes() == derr.tobytes()
        inv2 = np.zeros_like(inv)
        assert fj.lib().fib_warp_invert(0, field.ctypes.data, 9, 8, 7, _m16(Y), _m16(Q), niter, inv2.ctypes.data, None, 10, 9, 8) == 0
        assert inv2.tobytes() == dinv.tobytes()


# ---- end to end ---------------------------------------------------------------------------------------------------------------------
def _as_mri(fj, vol, v2r, res):
    """[nf, nz, ny, nx] -> MRI ([nx, ny, nz, nf], Fortran-ordered)"""
    return fj.MRI(np.asfortranarray(vol.transpose(3, 2, 1, 0)), volres=res, vox2ras=v2r)


def _from_mri(mri):
    return np.ascontiguousarray(mri.vol.transpose(3, 2, 1, 0))


@pytest.fixture(scope="module")
def traced(fj):
    """lines from `stream` on a 12^3 field whose volume lies over the warp's grid"""
    from fibers_jl_amd import phantom
    ov = fj.MRI(np.asfortranarray(phantom.fibre_field(12, 12, 12).astype(F)), volres=(1.5, 1.5, 2.0), vox2ras=IN_V2R)
    mask = fj.MRI(np.ones((12, 12, 12), np.uint8), volres=(1.5, 1.5, 2.0), vox2ras=IN_V2R)      # (a Tract takes its geometry from the mask)
    tr = fj.stream(ov, mask=mask, sublist=np.array([[0.1, -0.2, 0.3]], F))
    assert tr.nstr > 10 and np.array_equal(tr.vox2ras, IN_V2R)
    tr.scalars = np.arange(tr.xyz.shape[0], dtype=F)
    tr.properties = np.arange(2 * tr.nstr, dtype=F).reshape(-1, 2)
    return tr


def test_str_warp_end_to_end(fj, W, world, traced, tmp_path):
    tr = traced
    w = fj.Warp(_as_mri(fj, world["field"], FV2R, FRES))
    nx, ny, nz = 8, 8, 8
    i, j, k = np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij")
    labels = fj.MRI(np.asfortranarray((1 + (i >= 4) + 2 * (j >= 4) + 4 * (k >= 4)).astype(np.int32)), volres=(2.5, 2.5, 2.5),
                    vox2ras=R.oblique_vox2ras((2.5, 2.5, 2.5), angles_deg=(15.0, -6.0), origin=(-10.0, 2.0, -8.0)))
    moved = fj.str_warp(w, tr, outref=labels)
    want = R.warp_points(world["field"], *R.point_matrices(FV2R, IN_V2R, labels.vox2ras, None, None, 1), tr.xyz)
    assert _same_bits(moved.xyz, want) and not np.array_equal(moved.xyz, tr.xyz)
    assert moved.volsize == (8, 8, 8) and moved.volres == (2.5, 2.5, 2.5) and np.array_equal(moved.vox2ras, labels.vox2ras)
    assert np.array_equal(moved.npts, tr.npts) and np.array_equal(moved.seed_index, tr.seed_index)
    assert np.array_equal(moved.scalars, tr.scalars) and np.array_equal(moved.properties, tr.properties)
    # pre, post and 0-based lines; the geometry from post alone
    post = fj.Xform(ras2ras=POST, outsize=(8, 8, 8), outres=(2.5, 2.5, 2.5), outvox2ras=labels.vox2ras)
    pre = fj.Xform(ras2ras=PRE)
    zero = fj.str_warp(w, tr, pre=pre, post=post, origin=0)
    want0 = R.warp_points(world["field"], *R.point_matrices(FV2R, IN_V2R, labels.vox2ras, PRE, POST, 0), tr.xyz)
    assert _same_bits(zero.xyz, want0)
    assert zero.volsize == (8, 8, 8) and zero.volres == (2.5, 2.5, 2.5) and np.array_equal(zero.vox2ras, labels.vox2ras)
    with pytest.raises(ValueError, match="output geometry"):
        fj.str_warp(w, tr, pre=pre)
    # through a file: the same bytes
    path = str(tmp_path / "1Warp.nii.gz")
    assert fj.warp_write(w, path) is False
    again = fj.str_warp(fj.warp_read(path), tr, outref=labels)
    assert again.xyz.tobytes() == moved.xyz.tobytes()
    # and on to a connectome in the template's space
    con = fj.str_connectome(moved, labels)
    assert con.counts.sum() >= 1


def test_mri_warp_end_to_end(fj, W, world):
    w = fj.Warp(_as_mri(fj, world["field"], FV2R, FRES))
    v = _floats(3, SMALL, 14)
    mri = _as_mri(fj, v, GRID[SMALL], (2.6, 3.2, 5.0))
    mri.tr = 2.5
    mri.bval, mri.bvec = np.ones(3, F), np.ones((3, 3), F)
    res = fj.mri_warp(w, mri, outside=np.nan)                          # onto the field's own grid
    mats = R.volume_matrices(FV2R, FV2R, GRID[SMALL])
    assert _same_bits(_from_mri(res), R.warp_volume(world["field"], *mats, v, SMALL, FSHAPE, "trilinear", F(np.nan)))
    assert res.volsize == FSHAPE and res.volres == FRES and np.array_equal(res.vox2ras, FV2R) and res.vol.flags.f_contiguous
    assert res.tr == 2.5 and res.bval is None and res.bvec is None
    outref = fj.MRI(np.zeros(LARGE, F), volres=(2.0, 2.6, 3.6), vox2ras=GRID[LARGE])
    pre, post = fj.Xform(ras2ras=PRE), fj.Xform(ras2ras=POST)
    res = fj.mri_warp(w, mri, outref=outref, interp="nearest", outside=-1, pre=pre, post=post)
    mats = _vol_mats(SMALL, LARGE)
    assert _same_bits(_from_mri(res), R.warp_volume(world["field"], *mats, v, SMALL, LARGE, "nearest", F(-1)))
    assert res.volsize == LARGE and res.volres == (2.0, 2.6, 3.6) and np.array_equal(res.vox2ras, GRID[LARGE])
    # a narrow integer type is widened, resampled and narrowed back
    lab = np.random.default_rng(15).integers(0, 255, (1, 3, 5, 7), endpoint=True).astype(np.uint8)
    res = fj.mri_warp(w, _as_mri(fj, lab, GRID[SMALL], (2.6, 3.2, 5.0)), outref=outref, interp="nearest", outside=-1, pre=pre, post=post)
    want = R.warp_volume(world["field"], *mats, lab.astype(np.uint32), SMALL, LARGE, "nearest", np.uint32(255))
    assert res.vol.dtype == np.uint8 and np.array_equal(_from_mri(res), want.astype(np.uint8))


def test_warp_invert_end_to_end(fj, W, world):
    w = fj.Warp(_as_mri(fj, world["field"], FV2R, FRES))
    outref = fj.MRI(np.zeros(OSHAPE, F), volres=(1.8, 1.8, 1.8), vox2ras=OV2R)
    inv, err = fj.warp_invert(w, outref)
    Y, Q = R.invert_matrices(FV2R, OV2R)
    want_inv, want_err = R.invert(world["field"], Y, Q, OSHAPE, 20)
    assert isinstance(inv, fj.Warp) and _same_bits(_from_mri(inv.field), want_inv) and _same_bits(_from_mri(err)[0], want_err)
    for m in (inv.field, err):
        assert m.volsize == OSHAPE and m.volres == (1.8, 1.8, 1.8) and np.array_equal(m.vox2ras, OV2R)
    assert err.nframes == 1
    inv1, _ = fj.warp_invert(w, outref, niter=1)
    assert _same_bits(_from_mri(inv1.field), R.invert(world["field"], Y, Q, OSHAPE, 1)[0])


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_refused_arguments_of_the_device_entries(fj, torch_):
    torch = torch_
    L = fj.lib()
    M = _m16(EYE)
    buf = torch.zeros(8192, dtype=torch.float32, device="cuda")
    p = buf.data_ptr()                                                 # the packed 4 x 4 x 4 field: 256 floats
    a, b = p + 4 * 1024, p + 4 * 2048                                  # two arrays of up to 1024 floats
    big = (1 << 24) + 1
    INV, UNS = FIB_ERR_INVALID, FIB_ERR_UNSUPPORTED
    # pack
    assert L.fibd_warp_pack(None, 4, 4, 4, a, None) == INV and L.fibd_warp_pack(p, 4, 4, 4, None, None) == INV
    for dims in ((0, 4, 4), (4, -1, 4), (4, 4, 0)):
        assert L.fibd_warp_pack(p, *dims, a, None) == INV, dims
    assert L.fibd_warp_pack(p, big, 1, 1, a, None) == UNS
    assert L.fibd_warp_pack(p, 4, 4, 4, a + 4, None) == INV and b"16-byte" in L.fib_last_error()
    assert L.fibd_warp_pack(p, 4, 4, 4, p + 16, None) == INV and b"overlap" in L.fib_last_error()
    # points
    pts = (a, b, 10)
    assert L.fibd_warp_points(None, 4, 4, 4, M, M, M, *pts, None) == INV
    for mats in ((None, M, M), (M, None, M), (M, M, None)):
        assert L.fibd_warp_points(p, 4, 4, 4, *mats, *pts, None) == INV
    assert L.fibd_warp_points(p, 4, 4, 4, M, M, M, None, b, 10, None) == INV and L.fibd_warp_points(p, 4, 4, 4, M, M, M, a, None, 10, None) == INV
    assert L.fibd_warp_points(p, 4, 4, 4, M, M, M, a, b, -1, None) == INV
    assert L.fibd_warp_points(p, 0, 4, 4, M, M, M, *pts, None) == INV and L.fibd_warp_points(p, 4, 4, -2, M, M, M, *pts, None) == INV
    assert L.fibd_warp_points(p, 1, big, 1, M, M, M, *pts, None) == UNS
    assert L.fibd_warp_points(p, 4, 4, 4, M, M, M, a, a + 12, 10, None) == INV and b"overlap" in L.fib_last_error()     # neither the same nor apart
    assert L.fibd_warp_points(p, 4, 4, 4, M, M, M, a, a, 10, None) == 0                                             # in place is fine
    # volume
    def vol(packed=p, mats=(M, M, M), src=a, ins=(4, 4, 4), nf=1, interp=0, dst=b, outs=(4, 4, 4), fdims=(4, 4, 4)):
        return L.fibd_warp_volume(packed, *fdims, *mats, src, *ins, nf, interp, 0, dst, *outs, None)
    assert vol(packed=None) == INV and vol(src=None) == INV and vol(dst=None) == INV and vol(mats=(M, None, M)) == INV
    for bad in (dict(ins=(0, 4, 4)), dict(ins=(4, -1, 4)), dict(nf=0), dict(outs=(4, 0, 4)), dict(outs=(4, 4, -3)), dict(fdims=(4, 4, 0))):
        assert vol(**bad) == INV, bad
    assert vol(interp=2) == INV and b"interpolation" in L.fib_last_error() and vol(interp=-1) == INV
    assert vol(ins=(big, 1, 1)) == UNS and vol(outs=(1, 1, big)) == UNS and vol(fdims=(big, 1, 1)) == UNS
    assert vol(dst=a) == INV and b"overlap" in L.fib_last_error()
    assert vol(dst=a + 4 * 63) == INV and vol(src=a + 4 * 8, ins=(2, 2, 2), dst=a) == INV
    assert vol(dst=a + 4 * 64) == 0                                                                                 # adjacent is fine
    # invert
    def inv(packed=p, mats=(M, M), niter=3, dst=a, err=b, outs=(4, 4, 4), fdims=(4, 4, 4)):
        return L.fibd_warp_invert(packed, *fdims, *mats, niter, dst, err, *outs, None)
    assert inv(packed=None) == INV and inv(dst=None) == INV and inv(mats=(None, M)) == INV and inv(mats=(M, None)) == INV
    assert inv(niter=-1) == INV and b"niter" in L.fib_last_error()
    assert inv(outs=(0, 4, 4)) == INV and inv(outs=(4, 4, -1)) == INV and inv(fdims=(4, 0, 4)) == INV
    assert inv(outs=(big, 1, 1)) == UNS and inv(fdims=(1, 1, big)) == UNS
    assert inv(err=None) == 0 and inv(niter=0) == 0
    torch.cuda.synchronize()
    # nothing was launched on a refusal: the zero field maps everything to itself, so only the valid calls wrote, and wrote zeros
    assert torch.all(buf == 0).item()


def test_refused_arguments_of_the_host_forms(fj):
    L = fj.lib()
    M = _m16(EYE)
    field, pts, out = np.zeros(3 * 64, F), np.zeros(30, F), np.zeros(64 * 3, F)
    fp, pp, op = field.ctypes.data, pts.ctypes.data, out.ctypes.data
    INV, UNS = FIB_ERR_INVALID, FIB_ERR_UNSUPPORTED
    assert L.fib_warp_points(-1, fp, 4, 4, 4, M, M, M, pp, op, 10) == UNS
    assert L.fib_warp_points(0, None, 4, 4, 4, M, M, M, pp, op, 10) == INV and L.fib_warp_points(0, fp, 4, 4, 4, M, None, M, pp, op, 10) == INV
    assert L.fib_warp_points(0, fp, 4, 4, 4, M, M, M, None, op, 10) == INV and L.fib_warp_points(0, fp, 4, 4, 4, M, M, M, pp, None, 10) == INV
    assert L.fib_warp_points(0, fp, 4, 0, 4, M, M, M, pp, op, 10) == INV and L.fib_warp_points(0, fp, 4, 4, 4, M, M, M, pp, op, -1) == INV
    assert L.fib_warp_points(0, fp, 4, 4, 4, M, M, M, pp, pp + 12, 5) == INV
    assert L.fib_warp_volume(-1, fp, 4, 4, 4, M, M, M, pp, 3, 3, 3, 1, 0, 0, op, 4, 4, 4) == UNS
    assert L.fib_warp_volume(0, fp, 4, 4, 4, M, M, M, pp, 3, 3, 3, 1, 5, 0, op, 4, 4, 4) == INV
    assert L.fib_warp_volume(0, fp, 4, 4, 4, M, M, M, pp, 3, 3, 0, 1, 0, 0, op, 4, 4, 4) == INV
    assert L.fib_warp_volume(0, fp, 4, 4, 4, M, M, M, pp, 3, 3, 3, 0, 0, 0, op, 4, 4, 4) == INV
    assert L.fib_warp_volume(0, fp, 4, 4, 4, M, M, M, pp, 3, 3, 3, 1, 0, 0, pp, 3, 3, 3) == INV and b"overlap" in L.fib_last_error()
    assert L.fib_warp_volume(0, fp, 4, 4, 4, M, M, M, None, 3, 3, 3, 1, 0, 0, op, 4, 4, 4) == INV
    assert L.fib_warp_invert(-1, fp, 4, 4, 4, M, M, 3, op, None, 4, 4, 4) == UNS
    assert L.fib_warp_invert(0, fp, 4, 4, 4, M, M, -1, op, None, 4, 4, 4) == INV
    assert L.fib_warp_invert(0, fp, 4, 4, 4, M, M, 3, None, None, 4, 4, 4) == INV
    assert L.fib_warp_invert(0, fp, 4, 4, 4, M, M, 3, op, None, 4, 0, 4) == INV
    assert not out.any()


def test_refused_arguments_of_the_python_layer(fj, W, torch_):
    w = fj.Warp(fj.MRI(np.zeros((4, 3, 2, 3), F)))
    with pytest.raises(ValueError, match="3 float32 frames"):
        fj.Warp(fj.MRI(np.zeros((4, 3, 2, 4), F)))
    with pytest.raises(ValueError, match="output geometry"):
        fj.str_warp(w, fj.Tract(np.zeros((2, 3), F), np.array([2], np.int32)))
    with pytest.raises(ValueError, match="int32"):
        fj.mri_warp(w, fj.MRI(np.zeros((4, 3, 2), np.int32)), interp="trilinear")
    with pytest.raises(ValueError, match="float64"):
        fj.mri_warp(w, fj.MRI(np.zeros((4, 3, 2), np.float64)), interp="nearest")
    with pytest.raises(ValueError, match="interp"):
        fj.mri_warp(w, fj.MRI(np.zeros((4, 3, 2), F)), interp="cubic")
    with pytest.raises(ValueError, match="niter"):
        fj.warp_invert(w, fj.MRI(np.zeros((4, 3, 2), F)), niter=-2)
    singular = fj.Warp(fj.MRI(np.zeros((4, 3, 2, 3), F), vox2ras=np.zeros((4, 4), F)))
    with pytest.raises(ValueError, match="singular"):
        fj.warp_invert(singular, fj.MRI(np.zeros((4, 3, 2), F)))
    packed = torch_.zeros((24, 4), dtype=torch_.float32, device="cuda")
    with pytest.raises(ValueError, match="trilinear"):
        W.warp_volume_device(packed, (4, 3, 2), EYE, EYE, EYE, torch_.zeros(24, dtype=torch_.int32, device="cuda"), (4, 3, 2), (4, 3, 2))
    with pytest.raises(ValueError, match="niter"):
        W.warp_invert_device(packed, (4, 3, 2), EYE, EYE, (4, 3, 2), niter=-1)
    assert not [n for n in dir(fj) if n.startswith("warp") and n.endswith("_device")]         # the device tier is reached through the module


# ---- the device tier's argument contract ------------------------------------------------------------------------------------------
def _calls(W, torch):
    """name -> (call(**tensors), the valid tensors): every call is an exact fit, so one element short is the smallest failing size"""
    dev = torch.device("cuda", 0)
    shape, nvox = (4, 3, 2), 24

    def z(*s):
        return torch.zeros(s, dtype=torch.float32, device=dev)
    return {
        "warp_pack_device": (lambda disp, out: W.warp_pack_device(disp, shape, out=out), dict(disp=z(3, nvox), out=z(nvox, 4))),
        "warp_points_device": (lambda packed, xyz, out: W.warp_points_device(packed, shape, EYE, EYE, EYE, xyz, out=out),
                               dict(packed=z(nvox, 4), xyz=z(5, 3), out=z(5, 3))),
        "warp_volume_device": (lambda packed, vol, out: W.warp_volume_device(packed, shape, EYE, EYE, EYE, vol, shape, shape, out=out),
                               dict(packed=z(nvox, 4), vol=z(2, nvox), out=z(2, nvox))),
        "warp_invert_device": (lambda packed, inv, err: W.warp_invert_device(packed, shape, EYE, EYE, shape, niter=2, inv=inv, err=err),
                               dict(packed=z(nvox, 4), inv=z(3, nvox), err=z(nvox))),
    }


@pytest.mark.parametrize("name", ["warp_pack_device", "warp_points_device", "warp_volume_device", "warp_invert_device"])
def test_device_tier_argument_contract(W, torch_, name):
    """a host tensor, a wrong element type, a strided view, one element short, and a tensor on another device where there are two:
    each is an ArgError in Python, before any pointer leaves it (the library's own FibersError would not pass)"""
    torch = torch_
    from fibers_jl_amd._dev import ArgError
    call, args = _calls(W, torch)[name]
    call(**args)                                                       # the valid call runs
    torch.cuda.synchronize()
    passed = []
    for arg, t in args.items():
        bad = {"a host tensor": t.cpu(), "float64": t.to(torch.float64), "one element short": t.reshape(-1)[:-1].clone(),
               "a strided view": torch.zeros(tuple(t.shape) + (2,), dtype=torch.float32, device=t.device)[..., 0]}
        if torch.cuda.device_count() >= 2:
            bad["another device"] = t.to("cuda:1")
        assert not bad["a strided view"].is_contiguous()
        for what, b in bad.items():
            try:
                call(**dict(args, **{arg: b}))
            except ArgError:
                continue
            passed.append("%s: %s" % (arg, what))
    assert not passed, "%s accepted %s" % (name, passed)
