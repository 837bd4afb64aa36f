"""Non-linear registration on the GPU (fibd_nlreg_step, fibd_warp_smooth / _upsample / _unpack / _jacobian, fibd_nlreg_run, the host
forms fib_mri_nlreg / fib_warp_jacobian, mri_nlreg / warp_jacobian), bit for bit against the NumPy restatement (tests/nlreg_ref.py,
pinned on the CPU by tests/test_nlreg_ref.py) over every voxel: one iteration at both level sizes of the main case under three fields,
non-finite voxels in either volume and in the field, a moving volume entirely outside, the smoothing at four sigmas on three shapes, on
a side stream and in a view, the step between levels, the pack's inverse, the Jacobian map of a smooth, an affine and a folding field, the
whole pyramid through all three tiers with and without an initial affine, the refused arguments and the device tier's argument
contract.  The fields and the counts are exact; a sum of squares is held to |ssd - ref| <= count 2^-53 sum diff^2, which bounds any
order of summation (ref is the exactly rounded sum).  Shapes are a few thousand voxels: the file runs in seconds.  In-process only.

As in test_gpu_warp.py, where the restatement gives a NaN the kernel must give a NaN, of any payload."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nlreg_ref as N  # noqa: E402
import register_ref as G  # noqa: E402
import warp_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

F = np.float32
FIB_ERR_INVALID, FIB_ERR_UNSUPPORTED = -1, -7
EYE = np.eye(4, dtype=F)
STEP = 2.0                                                          # min(fixed.volres) of the main case
LONG, FLAT = (70, 9, 6), (16, 12, 1)                                 # rows longer than a tile; a size-1 axis


def _same_bits(got, want):
    """equal 32-bit patterns, except that any NaN answers a NaN"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    if got.dtype != F:
        return np.array_equal(got, want)
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])


@pytest.fixture(scope="module")
def torch_():
    import torch
    return torch


@pytest.fixture(scope="module")
def NL(fj):
    from fibers_jl_amd import nlreg
    return nlreg


@functools.lru_cache(maxsize=None)
def _case():
    """the main case and everything a level of it needs, made once: volumes, norms and matrices of levels 0 and 1"""
    fx, Vf, mv, Vm = N.pair()
    fp, mp = [fx, G.halve(fx)], [mv, G.halve(mv)]
    norms = [N.norm_of(fp[l]) + N.norm_of(mp[l]) for l in range(2)]
    mats = [N.level_matrices(Vf, Vm, None, l, STEP) for l in range(2)]
    return dict(Vf=Vf, Vm=Vm, fp=fp, mp=mp, norms=norms, mats=mats)


def _shape(a):
    return a.shape[::-1][:3]                                          # [(3,) nz, ny, nx] -> (nx, ny, nz)


def _cuda(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, F).reshape(-1)).cuda()


def _pack(fj, torch, field):
    return fj.warp.warp_pack_device(torch.from_numpy(np.ascontiguousarray(field, F).reshape(3, -1)).cuda(), _shape(field))


def _unpacked(packed, shape):
    """a packed field [nvox, 4] on the device -> [3, nz, ny, nx] on the host, and its fourth words"""
    nx, ny, nz = shape
    a = packed.cpu().numpy().reshape(-1, 4)
    return np.ascontiguousarray(a[:, :3].T).reshape(3, nz, ny, nx), a[:, 3]


def _dev_step(fj, NL, torch, fixed, moving, norm, mats, field, **kw):
    out, cost = NL.nlreg_step_device(_cuda(torch, fixed), _shape(fixed), _cuda(torch, moving), _shape(moving), norm, mats[0], mats[1], mats[2],
                                     mats[3], _pack(fj, torch, field), **kw)
    torch.cuda.synchronize()
    d, w = _unpacked(out, _shape(fixed))
    assert not w.any()                                                # the fourth word is written as 0
    return (d,) + NL.cost_pair(cost)


def _fields(level):
    c = _case()
    V = c["mats"][level][0]                                          # the level grid's vox2ras
    shape = _shape(c["fp"][level])
    smooth = R.smooth_field(V, shape, 2.0)
    out = smooth.copy()
    out[0] += F(14.0)                                                 # pushes part of the grid beyond a face of the moving volume
    return dict(zero=np.zeros_like(smooth), smooth=smooth, outside=out)


# ---- one iteration ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["zero", "smooth", "outside"])
@pytest.mark.parametrize("level", [0, 1])
def test_step_on_the_main_case(fj, NL, torch_, level, which):
    c = _case()
    field = _fields(level)[which]
    want, ssd, count = N.step(c["fp"][level], c["mp"][level], c["norms"][level], c["mats"][level], field)
    d, got_ssd, got_count = _dev_step(fj, NL, torch_, c["fp"][level], c["mp"][level], c["norms"][level], c["mats"][level], field)
    nvox = field[0].size
    print("level %d, %s: count %d of %d, ssd %.17g (ref %.17g, bound %.3g)" % (level, which, got_count, nvox, got_ssd, ssd, N.ssd_bound(ssd, count)))
    assert _same_bits(d, want)
    assert got_count == count and 0 < count and (count < nvox or which != "outside")
    assert abs(got_ssd - ssd) <= N.ssd_bound(ssd, count)
    assert not _same_bits(want, field)                               # the step moved something


def test_step_with_non_finite_voxels(fj, NL, torch_):
    """NaN and +-Inf in the fixed volume, in the moving volume and in the field: u = 0 wherever one of them reaches f, m or g, and the
    restatement's bits everywhere else"""
    c = _case()
    fx, mv, field = c["fp"][0].copy(), c["mp"][0].copy(), _fields(0)["smooth"].copy()
    fx[5, 6, 7], fx[2, 3, 4], fx[9, 10, 11] = np.nan, np.inf, -np.inf
    mv[7, 9, 8], mv[3, 4, 5], mv[10, 12, 13] = np.nan, -np.inf, np.inf
    field[0, 8, 3, 15], field[1, 4, 12, 3], field[2, 11, 8, 9] = np.nan, np.inf, -np.inf
    norm = N.norm_of(fx) + N.norm_of(mv)                              # (the range is of the finite values: none of them was an extreme)
    assert norm == c["norms"][0]
    want, ssd, count = N.step(fx, mv, norm, c["mats"][0], field)
    d, got_ssd, got_count = _dev_step(fj, NL, torch_, fx, mv, norm, c["mats"][0], field)
    clean, _, clean_count = N.step(c["fp"][0], c["mp"][0], norm, c["mats"][0], _fields(0)["smooth"])
    assert _same_bits(d, want) and got_count == count and abs(got_ssd - ssd) <= N.ssd_bound(ssd, count)
    assert count < clean_count
    for k, j, i in ((5, 6, 7), (2, 3, 4), (9, 10, 11)):               # a non-finite f: the field there is d + 0
        assert _same_bits(d[:, k, j, i], (field[:, k, j, i] + F(0)).astype(F))
        assert _same_bits(d[:, k, j, i + 1], (field[:, k, j, i + 1] + F(0)).astype(F))       # and g next to it
    changed = (d.view(np.uint32) != clean.view(np.uint32)).any(axis=0)
    assert 0 < changed.sum() < 0.1 * changed.size                     # the same bits elsewhere


def test_a_moving_volume_entirely_outside(fj, NL, torch_):
    c = _case()
    far = c["Vm"].copy()
    far[:3, 3] += F(500.0)
    mats = N.level_matrices(c["Vf"], far, None, 0, STEP)
    field = _fields(0)["smooth"]
    d, ssd, count = _dev_step(fj, NL, torch_, c["fp"][0], c["mp"][0], c["norms"][0], mats, field)
    assert _same_bits(d, field) and count == 0 and ssd == 0.0
    fx, mv = c["fp"][0], c["mp"][0]
    packed, cost, cnt = NL.mri_nlreg_device(_cuda(torch_, mv), _shape(mv), far, _cuda(torch_, fx), _shape(fx), c["Vf"], levels=2, niter=(2, 1),
                                            step=STEP)
    torch_.cuda.synchronize()
    assert np.isnan(cost).all() and not cnt.any() and not packed.cpu().numpy().any()


# ---- regularisation -----------------------------------------------------------------------------------------------------------------
def _test_field(shape, seed):
    nx, ny, nz = shape
    return np.random.default_rng(seed).normal(size=(3, nz, ny, nx)).astype(F)


@pytest.mark.parametrize("shape", [(20, 17, 13), LONG, FLAT])
@pytest.mark.parametrize("sigma", [0.0, 0.5, 1.0, 4.0])
def test_smooth(fj, NL, torch_, sigma, shape):
    field = _test_field(shape, 3)
    got = NL.warp_smooth_device(_pack(fj, torch_, field), shape, sigma)
    torch_.cuda.synchronize()
    d, w = _unpacked(got, shape)
    assert _same_bits(d, N.smooth(field, sigma)) and not w.any()
    if sigma == 0.0:
        assert _same_bits(d, field)


def test_smooth_in_a_view_on_a_side_stream(fj, NL, torch_):
    torch = torch_
    shape = (20, 17, 13)
    nvox = 20 * 17 * 13
    field = _test_field(shape, 4)
    packed = _pack(fj, torch, field)
    dst = torch.full((4 * nvox + 8,), 123.0, dtype=torch.float32, device="cuda")
    view = dst[4:4 + 4 * nvox].view(nvox, 4)                          # 16 bytes into the buffer
    assert view.data_ptr() % 16 == 0 and view.data_ptr() == dst.data_ptr() + 16
    work = torch.empty(4 * nvox, dtype=torch.float32, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    got = NL.warp_smooth_device(packed, shape, 1.0, out=view, work=work, stream=side)
    side.synchronize()
    assert got.data_ptr() == view.data_ptr() and _same_bits(_unpacked(got, shape)[0], N.smooth(field, 1.0))
    assert torch.all(dst[:4] == 123.0).item() and torch.all(dst[-4:] == 123.0).item()     # nothing written outside the view
    from fibers_jl_amd._dev import ArgError
    with pytest.raises(ArgError, match="16-byte"):
        NL.warp_smooth_device(packed, shape, 1.0, out=dst[1:1 + 4 * nvox].view(nvox, 4))


# ---- between levels, the pack's inverse ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("coarse,fine", [((10, 9, 7), (20, 17, 13)), ((7, 10, 5), (14, 19, 9)), ((35, 5, 3), LONG), ((8, 6, 1), FLAT)])
def test_upsample(fj, NL, torch_, coarse, fine):
    """even and odd sizes on both sides: odd -> even (7 -> 14), even -> odd (10 -> 19), and the clamp at both ends of every axis"""
    field = _test_field(coarse, 5)
    got = NL.warp_upsample_device(_pack(fj, torch_, field), coarse, fine)
    torch_.cuda.synchronize()
    d, w = _unpacked(got, fine)
    assert _same_bits(d, N.upsample(field, fine)) and not w.any()


@pytest.mark.parametrize("shape", [(20, 17, 13), (1, 1, 1), (257, 3, 1)])
def test_unpack_undoes_pack(fj, NL, torch_, shape):
    field = _test_field(shape, 6)
    field[0].reshape(-1)[0] = np.nan
    field[1].reshape(-1)[-1] = -0.0
    got = NL.warp_unpack_device(_pack(fj, torch_, field), shape)
    torch_.cuda.synchronize()
    assert tuple(got.shape) == (3, field[0].size) and got.cpu().numpy().tobytes() == field.tobytes()


# ---- the Jacobian map ---------------------------------------------------------------------------------------------------------------
WSHAPE, WRES = (9, 8, 7), (2.0, 2.0, 2.5)                            # the warp tests' grid
WV2R = R.oblique_vox2ras(WRES)


@pytest.mark.parametrize("which", ["smooth", "affine", "folding", "flat"])
def test_jacobian(fj, NL, torch_, which):
    shape, V = WSHAPE, WV2R
    if which == "smooth":
        field = R.smooth_field(V, shape, 2.0)
    elif which == "affine":
        field = R.affine_field(V, shape, np.eye(3) + [[0.05, -0.03, 0.02], [0.04, -0.06, 0.01], [-0.02, 0.03, 0.07]], (0.5, -0.25, 0.125))[0]
    elif which == "folding":
        field = R.smooth_field(V, shape, 12.0)                        # the field of test_inverse_of_a_folding_field
    else:
        shape = FLAT
        field = R.smooth_field(V, shape, 2.0)
    want = N.jacobian(field, V)
    got = NL.warp_jacobian_device(_pack(fj, torch_, field), shape, NL.jacobian_matrix(V))
    torch_.cuda.synchronize()
    got = got.cpu().numpy().reshape(want.shape)
    assert _same_bits(got, want)
    assert np.array_equal(got <= 0, want <= 0) and (which != "folding" or (got <= 0).any()) and (which == "folding" or (got > 0).all())
    # the host form and warp_jacobian give the same bytes
    w = fj.Warp(fj.MRI(np.asfortranarray(field.transpose(3, 2, 1, 0)), volres=WRES, vox2ras=V))
    jm = fj.warp_jacobian(w)
    assert jm.nframes == 1 and jm.volsize == shape and np.array_equal(jm.vox2ras, V)
    assert np.ascontiguousarray(jm.vol[..., 0].transpose(2, 1, 0)).tobytes() == got.tobytes()


# ---- the whole pyramid --------------------------------------------------------------------------------------------------------------
def _init_xform(fj, Vf, Vm, fshape, mshape):
    """the Xform mri_register would return for a 5 degree rigid motion (in = moving, out = fixed), and the fixed RAS -> moving RAS matrix
    mri_nlreg derives from it"""
    ras2ras = np.linalg.inv(N.rigid().astype(np.float64)).astype(F)   # moving RAS -> fixed RAS
    x = fj.Xform(insize=mshape, outsize=fshape, inres=(2.1, 1.9, 2.0), outres=(2.0, 2.0, 2.0), invox2ras=Vm, outvox2ras=Vf, ras2ras=ras2ras)
    return x, np.linalg.inv(ras2ras.astype(np.float64)).astype(F)


@functools.lru_cache(maxsize=None)
def _run_ref(with_init):
    c = _case()
    post = None
    if with_init:
        post = np.linalg.inv(np.linalg.inv(N.rigid().astype(np.float64)).astype(F).astype(np.float64)).astype(F)
    field, cost, count, ssd = N.run(c["fp"][0], c["Vf"], c["mp"][0], c["Vm"], post, 2, (3, 2), 1.0, STEP)
    return field, cost, count, ssd, N.warped(field, c["Vf"], c["mp"][0], c["Vm"], post), post


def _costs_within_the_bound(cost, count, ref):
    field, rcost, rcount, rssd = ref[:4]
    assert np.array_equal(count, rcount) and np.array_equal(np.isnan(cost), np.isnan(rcost))
    ran = rcount > 0
    # the sum's bound, divided by the count, plus the rounding of that division
    tol = N.ssd_bound(rssd[ran], rcount[ran]) / rcount[ran] + 2.0 ** -52 * rcost[ran]
    assert (np.abs(cost[ran] - rcost[ran]) <= tol).all(), (cost, rcost)


@pytest.mark.parametrize("with_init", [False, True])
def test_run_on_device_volumes(fj, NL, torch_, with_init):
    c = _case()
    ref = _run_ref(with_init)
    fx, mv = c["fp"][0], c["mp"][0]
    packed, cost, count = NL.mri_nlreg_device(_cuda(torch_, mv), _shape(mv), c["Vm"], _cuda(torch_, fx), _shape(fx), c["Vf"], post=ref[5], levels=2,
                                              niter=(3, 2), sigma=1.0, step=STEP)
    torch_.cuda.synchronize()
    d, w = _unpacked(packed, _shape(fx))
    assert _same_bits(d, ref[0]) and not w.any()
    assert cost.shape == (2, 3) and np.isnan(cost[1, 2])
    _costs_within_the_bound(cost, count, ref)
    assert with_init or (cost[0, 2] < cost[0, 0] and cost[1, 1] < cost[1, 0])


@pytest.mark.parametrize("with_init", [False, True])
def test_mri_nlreg_end_to_end(fj, NL, with_init):
    c = _case()
    ref = _run_ref(with_init)
    fx, mv, Vf, Vm = c["fp"][0], c["mp"][0], c["Vf"], c["Vm"]
    fixed = fj.MRI(np.asfortranarray(fx.transpose(2, 1, 0)), volres=(2.0, 2.0, 2.0), vox2ras=Vf)
    moving = fj.MRI(np.asfortranarray(mv.transpose(2, 1, 0)), volres=(2.1, 1.9, 2.0), vox2ras=Vm)
    init = None
    if with_init:
        init, post = _init_xform(fj, Vf, Vm, _shape(fx), _shape(mv))
        assert np.array_equal(post, ref[5])
    r = fj.mri_nlreg(moving, fixed, init=init, levels=2, niter=(3, 2))                 # sigma 1, step min(volres) = 2: the defaults
    assert isinstance(r, fj.NonlinearRegistration) and isinstance(r.warp, fj.Warp)
    got = np.ascontiguousarray(r.warp.field.vol.transpose(3, 2, 1, 0))
    assert _same_bits(got, ref[0])
    assert r.warp.volsize == _shape(fx) and np.array_equal(r.warp.vox2ras, Vf) and tuple(r.warp.field.volres) == (2.0, 2.0, 2.0)
    _costs_within_the_bound(r.cost, r.count, ref)
    assert (r.post is None) == (not with_init) and (init is None or np.array_equal(r.post.ras2ras, ref[5]))
    warped = np.ascontiguousarray(r.warped.vol[..., 0].transpose(2, 1, 0))
    assert _same_bits(warped, ref[4]) and r.warped.volsize == _shape(fx) and np.array_equal(r.warped.vox2ras, Vf)
    again = fj.mri_warp(r.warp, moving, outref=fixed, post=r.post)
    assert again.vol.tobytes() == r.warped.vol.tobytes() and again.vol.dtype == r.warped.vol.dtype
    # a few points of the fixed space into the moving volume
    xyz = (np.random.default_rng(8).uniform(0.1, 0.9, (7, 3)) * (np.array(_shape(fx)) - 1) + 1).astype(F)
    tr = fj.Tract(xyz, np.array([4, 3], np.int32), volsize=_shape(fx), volres=(2.0, 2.0, 2.0), vox2ras=Vf)
    moved = fj.str_warp(r.warp, tr, outref=moving, post=r.post)
    assert _same_bits(moved.xyz, R.warp_points(ref[0], *R.point_matrices(Vf, Vf, Vm, None, ref[5], 1), xyz))
    # the Jacobian map of the estimate: no fold
    assert (fj.warp_jacobian(r.warp).vol > 0).all()


def test_mri_nlreg_defaults_and_a_named_frame(fj):
    """levels from mri_register's rule (one, for these sizes: 13 halves to 7), one niter for every level, sigma 0, a frame of a series"""
    c = _case()
    fx, mv, Vf, Vm = c["fp"][0], c["mp"][0], c["Vf"], c["Vm"]
    assert G.default_levels(_shape(fx), _shape(mv)) == 1
    fixed = fj.MRI(np.asfortranarray(fx.transpose(2, 1, 0)), volres=(2.0, 2.0, 2.0), vox2ras=Vf)
    series = np.stack([np.zeros_like(mv), mv], axis=0)
    moving = fj.MRI(np.asfortranarray(series.transpose(3, 2, 1, 0)), volres=(2.1, 1.9, 2.0), vox2ras=Vm)
    r = fj.mri_nlreg(moving, fixed, niter=2, sigma=0.0, frame=1)
    want, cost, count, ssd = N.run(fx, Vf, mv, Vm, None, None, 2, 0.0, STEP)
    assert _same_bits(np.ascontiguousarray(r.warp.field.vol.transpose(3, 2, 1, 0)), want) and np.array_equal(r.count, count)
    assert r.cost.shape == (1, 2) and _costs_within_the_bound(r.cost, r.count, (want, cost, count, ssd)) is None
    with pytest.raises(ValueError, match="frame"):
        fj.mri_nlreg(moving, fixed, niter=2)
    with pytest.raises(ValueError, match="niter"):
        fj.mri_nlreg(moving, fixed, niter=(1, 2, 3), frame=1)
    with pytest.raises(fj.FibersError, match="constant volume"):
        fj.mri_nlreg(moving, fixed, niter=2, frame=0)


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def _m16(m):
    return (C.c_float * 16)(*np.ascontiguousarray(m, F).reshape(-1).tolist())


def test_refused_arguments_of_the_device_entries(fj, torch_):
    torch = torch_
    L = fj.lib()
    M, T, NORM = _m16(EYE), (C.c_float * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1), (C.c_float * 4)(0, 1, 0, 1)
    buf = torch.zeros(16384, dtype=torch.float32, device="cuda")
    p = buf.data_ptr()
    q, w, vf, vm, co = p + 4 * 1024, p + 4 * 2048, p + 4 * 4096, p + 4 * 5120, p + 4 * 6144    # 4 x 4 x 4: a packed field is 256 floats
    big = (1 << 24) + 1
    INV, UNS = FIB_ERR_INVALID, FIB_ERR_UNSUPPORTED
    nb = C.c_uint64()

    def step(fixed=vf, fs=(4, 4, 4), moving=vm, ms=(4, 4, 4), norm=NORM, mats=(M, M), t=T, packed=p, out=q, cost=co, work=w, wb=4096):
        return L.fibd_nlreg_step(fixed, *fs, moving, *ms, norm, *mats, t, 1.0, packed, out, cost, work, wb, None)
    for bad in (dict(fixed=None), dict(moving=None), dict(norm=None), dict(mats=(None, M)), dict(mats=(M, None)), dict(t=None), dict(packed=None),
                dict(out=None), dict(cost=None), dict(work=None), dict(fs=(0, 4, 4)), dict(fs=(4, 4, -1)), dict(ms=(4, 0, 4)), dict(packed=p + 4),
                dict(out=q + 8), dict(cost=co + 4), dict(wb=8), dict(out=p + 16), dict(out=vf), dict(work=vm), dict(cost=p), dict(work=q)):
        assert step(**bad) == INV, bad
    assert step(fs=(big, 1, 1)) == UNS and step(ms=(1, 1, big)) == UNS
    assert L.fibd_nlreg_step_work_size(4, 4, 4, None) == INV and L.fibd_nlreg_step_work_size(4, 0, 4, C.byref(nb)) == INV
    assert L.fibd_nlreg_step_work_size(4, 4, 4, C.byref(nb)) == 0 and nb.value == 16 * 4

    def smooth(packed=p, dims=(4, 4, 4), sigma=1.0, out=q, work=w, wb=4096):
        return L.fibd_warp_smooth(packed, *dims, sigma, out, work, wb, None)
    for bad in (dict(packed=None), dict(out=None), dict(work=None), dict(dims=(4, 0, 4)), dict(sigma=5.0), dict(sigma=-0.5), dict(sigma=float("nan")),
                dict(packed=p + 8), dict(out=q + 4), dict(work=w + 8), dict(wb=1023), dict(out=p + 64), dict(work=q + 16), dict(work=p)):
        assert smooth(**bad) == INV, bad
    assert smooth(sigma=5.0) == INV and b"sigma" in L.fib_last_error()
    assert smooth(dims=(1, big, 1)) == UNS

    def up(coarse=p, cs=(2, 2, 2), out=q, dims=(4, 4, 4)):
        return L.fibd_warp_upsample(coarse, *cs, out, *dims, None)
    for bad in (dict(coarse=None), dict(out=None), dict(cs=(0, 2, 2)), dict(dims=(4, 4, 0)), dict(coarse=p + 4), dict(out=q + 8), dict(out=p + 64)):
        assert up(**bad) == INV, bad
    assert up(cs=(big, 1, 1)) == UNS and up(dims=(1, 1, big)) == UNS

    def unpack(packed=p, dims=(4, 4, 4), disp=q):
        return L.fibd_warp_unpack(packed, *dims, disp, None)
    for bad in (dict(packed=None), dict(disp=None), dict(dims=(4, -4, 4)), dict(packed=p + 4), dict(disp=q + 2), dict(disp=p + 4 * 255)):
        assert unpack(**bad) == INV, bad
    assert unpack(dims=(big, 1, 1)) == UNS

    def jac(packed=p, dims=(4, 4, 4), linv=T, out=q):
        return L.fibd_warp_jacobian(packed, *dims, linv, out, None)
    for bad in (dict(packed=None), dict(linv=None), dict(out=None), dict(dims=(0, 4, 4)), dict(packed=p + 8), dict(out=q + 1), dict(out=p + 4 * 255)):
        assert jac(**bad) == INV, bad
    assert jac(dims=(1, big, 1)) == UNS

    S3 = (C.c_int32 * 3)(4, 4, 4)
    n2, neg = (C.c_int32 * 2)(1, 1), (C.c_int32 * 2)(1, -1)
    wbig = torch.zeros(1 << 16, dtype=torch.float32, device="cuda")
    cost, count = (C.c_double * 2)(), (C.c_int64 * 2)()

    def run(fixed=vf, fs=S3, fv=M, moving=vm, ms=S3, mvr=M, levels=2, niter=n2, sigma=1.0, stp=1.0, field=q, work=wbig.data_ptr(), wb=4 << 16):
        return L.fibd_nlreg_run(fixed, fs, fv, moving, ms, mvr, None, levels, niter, sigma, stp, field, cost, count, work, wb, None)
    zero3 = (C.c_int32 * 3)(4, 0, 4)
    big3 = (C.c_int32 * 3)(big, 1, 1)
    for bad in (dict(fixed=None), dict(moving=None), dict(fs=None), dict(ms=None), dict(fv=None), dict(mvr=None), dict(niter=None), dict(field=None),
                dict(work=None), dict(fs=zero3), dict(ms=zero3), dict(levels=0), dict(levels=5), dict(niter=neg), dict(sigma=5.0), dict(stp=0.0),
                dict(stp=float("inf")), dict(field=q + 4), dict(work=wbig.data_ptr() + 8), dict(wb=1024), dict(field=vf), dict(work=vf, wb=1 << 30),
                dict(fv=_m16(np.zeros((4, 4), F))), dict(mvr=_m16(np.zeros((4, 4), F)))):
        assert run(**bad) == INV, bad
    assert run(niter=neg) == INV and b"niter" in L.fib_last_error()
    assert run(fs=big3) == UNS
    assert L.fibd_nlreg_work_size(S3, S3, 2, n2, None) == INV and L.fibd_nlreg_work_size(S3, S3, 2, neg, C.byref(nb)) == INV
    assert L.fibd_nlreg_work_size(S3, S3, 2, n2, C.byref(nb)) == 0 and 0 < nb.value <= 4 << 16
    torch.cuda.synchronize()
    assert torch.all(buf == 0).item()                                 # nothing was launched on a refusal
    # a constant volume is refused by the driver once the ranges are back
    assert run() == INV and b"constant volume" in L.fib_last_error()
    torch.cuda.synchronize()


def test_refused_arguments_of_the_host_forms(fj):
    L = fj.lib()
    M, T = _m16(EYE), (C.c_float * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
    INV, UNS = FIB_ERR_INVALID, FIB_ERR_UNSUPPORTED
    vol = np.arange(64, dtype=F)
    disp, out = np.zeros(3 * 64, F), np.zeros(64, F)
    S3, zero3 = (C.c_int32 * 3)(4, 4, 4), (C.c_int32 * 3)(4, 4, 0)
    n1, neg = (C.c_int32 * 1)(1), (C.c_int32 * 1)(-1)
    mats = np.concatenate([EYE.reshape(-1)] * 3).astype(F)

    def reg(device=0, moving=vol.ctypes.data, ms=S3, mvr=M, fixed=vol.ctypes.data, fs=S3, fv=M, levels=1, niter=n1, sigma=1.0, stp=1.0,
            d=disp.ctypes.data, wm=mats.ctypes.data, warped=out.ctypes.data):
        return L.fib_mri_nlreg(device, moving, ms, mvr, fixed, fs, fv, None, levels, niter, sigma, stp, d, None, None, wm, warped)
    assert reg(device=-1) == UNS and b"one device" in L.fib_last_error()
    for bad in (dict(moving=None), dict(fixed=None), dict(ms=None), dict(fs=None), dict(mvr=None), dict(fv=None), dict(niter=None), dict(d=None),
                dict(wm=None), dict(fs=zero3), dict(ms=zero3), dict(levels=0), dict(levels=5), dict(niter=neg), dict(sigma=5.0), dict(sigma=-1.0),
                dict(stp=-1.0), dict(fv=_m16(np.zeros((4, 4), F)))):
        assert reg(**bad) == INV, bad
    const = np.ones(64, F)
    assert reg(fixed=const.ctypes.data) == INV and b"constant volume" in L.fib_last_error()
    assert reg(moving=const.ctypes.data) == INV and b"constant volume" in L.fib_last_error()
    assert not disp.any() and not out.any()
    assert reg(wm=None, warped=None) == 0                             # identical volumes: the zero field
    assert not disp.any()

    def jac(device=0, d=disp.ctypes.data, dims=(4, 4, 4), linv=T, o=out.ctypes.data):
        return L.fib_warp_jacobian(device, d, *dims, linv, o)
    assert jac(device=-1) == UNS
    for bad in (dict(d=None), dict(linv=None), dict(o=None), dict(dims=(4, 0, 4)), dict(dims=(-1, 4, 4))):
        assert jac(**bad) == INV, bad
    assert jac() == 0 and np.array_equal(out, np.ones(64, F))         # the zero field: det = 1


def test_refused_arguments_of_the_python_layer(fj, NL, torch_):
    from fibers_jl_amd._dev import ArgError
    vol = np.arange(8 * 8 * 8 * 4, dtype=F).reshape(8, 8, 8, 4)
    with pytest.raises(ValueError, match="frame"):
        fj.mri_nlreg(fj.MRI(vol), fj.MRI(vol[..., 0]))                # a 4-frame moving without `frame`
    with pytest.raises(ValueError, match="frame 4"):
        fj.mri_nlreg(fj.MRI(vol), fj.MRI(vol[..., 0]), frame=4)
    with pytest.raises(ValueError, match="niter"):
        fj.mri_nlreg(fj.MRI(vol[..., 0]), fj.MRI(vol[..., 0]), levels=2, niter=(1, 2, 3))
    with pytest.raises(fj.FibersError, match="sigma"):
        fj.mri_nlreg(fj.MRI(vol[..., 0]), fj.MRI(vol[..., 0]), levels=1, niter=1, sigma=5)
    z = torch_.zeros(512, dtype=torch_.float32, device="cuda")
    with pytest.raises(ArgError, match="niter"):
        NL.mri_nlreg_device(z, (8, 8, 8), EYE, z, (8, 8, 8), EYE, levels=2, niter=(1,))
    singular = fj.Warp(fj.MRI(np.zeros((4, 3, 2, 3), F), vox2ras=np.zeros((4, 4), F)))
    with pytest.raises(ValueError, match="singular"):
        fj.warp_jacobian(singular)
    assert not [n for n in dir(fj) if n.endswith("_device") and ("nlreg" in n or n.startswith("warp"))]   # the device tier is reached through the module


# ---- the device tier's argument contract ------------------------------------------------------------------------------------------
def _calls(NL, torch):
    """name -> (call(**tensors), the valid tensors): every call is an exact fit, so one element short is the smallest failing size"""
    dev = torch.device("cuda", 0)
    shape, nvox, cshape, cvox = (4, 3, 2), 24, (2, 2, 1), 4
    T3 = np.eye(3, dtype=F)

    def z(*s, dtype=torch.float32):
        return torch.zeros(s, dtype=dtype, device=dev)

    def ramp(n):
        return torch.arange(n, dtype=torch.float32, device=dev)
    return {
        "nlreg_step_device": (lambda fixed, moving, packed, out, cost: NL.nlreg_step_device(fixed, shape, moving, shape, (0, 1, 0, 1), EYE, EYE, T3, 1.0,
                                                                                           packed, out=out, cost=cost),
                              dict(fixed=z(nvox), moving=z(nvox), packed=z(nvox, 4), out=z(nvox, 4), cost=z(2, dtype=torch.int64))),
        "warp_smooth_device": (lambda packed, out: NL.warp_smooth_device(packed, shape, 1.0, out=out), dict(packed=z(nvox, 4), out=z(nvox, 4))),
        "warp_upsample_device": (lambda coarse, out: NL.warp_upsample_device(coarse, cshape, shape, out=out), dict(coarse=z(cvox, 4), out=z(nvox, 4))),
        "warp_unpack_device": (lambda packed, out: NL.warp_unpack_device(packed, shape, out=out), dict(packed=z(nvox, 4), out=z(3, nvox))),
        "warp_jacobian_device": (lambda packed, out: NL.warp_jacobian_device(packed, shape, T3, out=out), dict(packed=z(nvox, 4), out=z(nvox))),
        "mri_nlreg_device": (lambda moving, fixed, out: NL.mri_nlreg_device(moving, shape, EYE, fixed, shape, EYE, levels=1, niter=1, out=out),
                             dict(moving=ramp(nvox), fixed=ramp(nvox), out=z(nvox, 4))),
    }


@pytest.mark.parametrize("name", ["nlreg_step_device", "warp_smooth_device", "warp_upsample_device", "warp_unpack_device", "warp_jacobian_device",
                                  "mri_nlreg_device"])
def test_device_tier_argument_contract(NL, torch_, name):
    """a host tensor, a wrong element type, a strided view, one element short, and a tensor on another device where there are two:
    each is an ArgError in Python, before any pointer leaves it (the library's own FibersError would not pass)"""
    torch = torch_
    from fibers_jl_amd._dev import ArgError
    call, args = _calls(NL, torch)[name]
    call(**args)                                                       # the valid call runs
    torch.cuda.synchronize()
    passed = []
    for arg, t in args.items():
        bad = {"a host tensor": t.cpu(), "float64": t.to(torch.float64), "one element short": t.reshape(-1)[:-1].clone(),
               "a strided view": torch.zeros(tuple(t.shape) + (2,), dtype=t.dtype, device=t.device)[..., 0]}
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
