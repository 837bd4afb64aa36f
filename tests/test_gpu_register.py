"""GPU tests of the registration ("Registration", include/fibers_hip.h) against tests/register_ref.py: the pyramid, the range and the
joint histograms bit for bit; mri_register and dwi_moco decision for decision (theta bit-equal, the trace identical)."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import register_ref as R  # noqa: E402
import volxform_ref as vref  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def gpu_hist(fj, fixed, moving, jobs, nbins):
    """(hist uint32 [njobs, nbins, nbins], fixed range, moving ranges) of the device tier for NumPy volumes [nz, ny, nx] / [nf, nz, ny, nx]"""
    reg = fj.register
    fshape, mshape = fixed.shape[::-1], moving.shape[1:][::-1]
    fx, mv = _dev(fixed.reshape(-1)), _dev(moving.reshape(moving.shape[0], -1))
    rf, rm = reg.vol_range_device(fx, fx.numel(), nbins), reg.vol_range_device(mv, mv.shape[1], nbins)
    h = reg.reg_hist_device(fx, fshape, rf, mv, mshape, rm, [f for f, _ in jobs], np.stack([M for _, M in jobs]), nbins)
    return h.cpu().numpy().view(np.uint32), rf, rm


def ref_hist(fixed, moving, jobs, nbins):
    return R.reg_hist(fixed, R.vol_range(fixed, nbins), moving, [R.vol_range(m, nbins) for m in moving], jobs, nbins)


# ---- fibd_reg_hist ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("njobs,nbins", [(1, 32), (12, 8), (12, 32), (13, 64)])
def test_reg_hist_bit_for_bit(fj, njobs, nbins):
    """fixed 13x11x9 against moving 10x12x7 through the oblique matrix: different grids, odd sizes, a partial overlap, NaN voxels in
    both, a job -> frame map that is neither monotone nor injective, a projective last row in every other job"""
    fixed, moving = R.hist_volumes((13, 11, 9), (10, 12, 7), 3, seed=4)
    jobs = R.hist_jobs(njobs, 3, vref.out2in(vref.oblique()), projective=True)
    got, _, _ = gpu_hist(fj, fixed, moving, jobs, nbins)
    want = ref_hist(fixed, moving, jobs, nbins)
    assert np.array_equal(got, want)
    # the sum of a histogram is the restated count of inside, finite samples
    for j, (f, M) in enumerate(jobs):
        ok = vref.inside_mask(vref.pull_back(M, (13, 11, 9)), (10, 12, 7)) & np.isfinite(fixed)
        v = vref.vol_xform_ref(M, moving[f], (10, 12, 7), (13, 11, 9), "trilinear", F(0))[0]
        assert got[j].sum() == (ok & ~np.isnan(v)).sum()
    assert 0 < got[0].sum() < fixed.size


def test_reg_hist_value_equal_to_hi_lands_in_the_last_bin(fj):
    fixed = np.arange(5 * 6 * 7, dtype=F).reshape(5, 6, 7)
    moving = fixed[None].copy()
    jobs = [(0, np.eye(4, dtype=F))]
    got, _, _ = gpu_hist(fj, fixed, moving, jobs, 8)
    assert np.array_equal(got, ref_hist(fixed, moving, jobs, 8))
    assert got[0, 7, 7] >= 1 and got[0].sum() == fixed.size and np.array_equal(got[0], np.diag(np.diag(got[0])))


@pytest.mark.parametrize("fshape", [(3, 2, 2), (70, 6, 10), (130, 9, 17)])
def test_reg_hist_fewer_voxels_than_a_wave_and_more_than_one_tile_along_every_axis(fj, fshape):
    fixed, moving = R.hist_volumes(fshape, (11, 9, 8), 2, seed=5)
    s = np.diag([10.0 / fshape[0], 8.0 / fshape[1], 7.0 / fshape[2], 1.0]).astype(F)
    jobs = R.hist_jobs(5, 2, s)
    got, _, _ = gpu_hist(fj, fixed, moving, jobs, 32)
    assert np.array_equal(got, ref_hist(fixed, moving, jobs, 32))
    assert got.sum() > 0


def test_reg_hist_under_the_other_lds_scheme_of_the_diagnostic_build():
    """the same cases with both LDS schemes forced (one histogram per workgroup; a copy per wave), in a child process that loads
    libfibers_hip_stamp.so (tools/register_check.py)"""
    assert os.path.exists(os.path.join(ROOT, "fibers.jl_amd", "libfibers_hip_stamp.so")), \
        "the diagnostic build is absent (make -C fibers.jl_amd/csrc stamp): the other LDS scheme cannot be checked"
    env = {k: v for k, v in os.environ.items() if not k.startswith("FIBERS_")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "register_check.py")], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "register check: ok" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]


# ---- fibd_vol_halve, fibd_vol_range -------------------------------------------------------------------------------------------------
def _same_bits(got, want):
    got, want = np.asarray(got, F), np.asarray(want, F)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])


@pytest.mark.parametrize("shape", [(8, 4, 6), (7, 5, 3), (1, 9, 2), (5, 1, 1), (33, 18, 7)])
def test_vol_halve_and_vol_range_bit_for_bit(fj, shape):
    """even, odd and size-1 axes; +-Inf and NaN entries; two frames at once"""
    rng = np.random.default_rng(sum(shape))
    vol = rng.normal(0, 50, (2,) + shape[::-1]).astype(F)
    flat = vol.reshape(-1)
    flat[[1, flat.size // 2]] = np.nan
    flat[flat.size // 3] = np.inf
    flat[flat.size - 2] = -np.inf
    d = _dev(vol.reshape(2, -1))
    got = fj.register.vol_halve_device(d, shape).cpu().numpy()
    want = np.stack([R.halve(v) for v in vol])
    assert fj.register.halved(shape) == want.shape[1:][::-1]
    assert _same_bits(got.reshape(want.shape), want)
    for nbins in (8, 32):
        tab, n = fj.register.range_table(fj.register.vol_range_device(d, d.shape[1], nbins))
        for f in range(2):
            lo, hi, scale, cnt = R.vol_range(vol[f], nbins)
            assert _same_bits(tab[f], np.array([lo, hi, scale], F)) and n[f] == cnt


def test_vol_range_without_a_finite_value_and_of_a_constant(fj):
    vol = np.full((3, 10), np.nan, F)
    vol[1] = 4.5
    vol[2, :5] = [-0.0, 0.0, np.inf, -0.0, 0.0]
    tab, n = fj.register.range_table(fj.register.vol_range_device(_dev(vol), 10, 16))
    assert list(n) == [0, 10, 4] and np.isnan(tab[0, 2]) and tab[0, 0] == 0 and np.isinf(tab[1, 2]) and tab[1, 0] == tab[1, 1] == F(4.5)
    assert np.signbit(tab[2, 0]) and not np.signbit(tab[2, 1]) and np.isinf(tab[2, 2])


# ---- mri_register -------------------------------------------------------------------------------------------------------------------
def _mri(fj, arr, V, **kw):
    """[nz, ny, nx] or [nf, nz, ny, nx] -> an MRI of 2 mm voxels"""
    return fj.MRI(np.asfortranarray(arr.T), volres=(2.0, 2.0, 2.0), vox2ras=np.array(V, F), **kw)


def _check_trace(got_rows, want_rows):
    got = np.array([[t["level"], t["ndof"], t["index"], t["moved"]] for t in got_rows], np.float64).reshape(-1, 4)
    assert np.array_equal(got, want_rows[:, :4])
    for t, w in zip(got_rows, want_rows):
        n = 2 * t["ndof"]
        assert np.allclose(np.append(t["costs"], t["cost"]), np.append(w[5:5 + n], w[4]), rtol=1e-10, atol=0)


@pytest.mark.parametrize("name", ["28", "41", "41x12"])
def test_mri_register_takes_the_restatement_s_decisions(fj, name):
    c = R.case(name)
    r = fj.mri_register(_mri(fj, c["moving"], c["V"]), _mri(fj, c["fixed"], c["V"]), dof=c["dof"], levels=c["levels"])
    assert np.array_equal(r.theta, c["theta"])
    _check_trace(r.trace, c["trace"])
    assert abs(r.cost - c["cost"]) <= 1e-10 * abs(c["cost"])
    r2r, v2v = R.xfm_matrices(c["theta"], c["V"], c["size"], c["V"])
    for got, want in ((r.xfm.ras2ras, r2r), (r.xfm.vox2vox, v2v)):
        assert np.abs(got.astype(np.float64) - want.astype(np.float64)).max() <= 2 * np.spacing(np.abs(want).max())
    assert tuple(r.xfm.outsize) == c["size"] and np.array_equal(r.xfm.voxrot, fj.xform.voxrot_of(r.xfm.vox2vox))
    if name == "28":                                           # mri_xform through the result lands on the fixed grid
        out = fj.mri_xform(r.xfm, _mri(fj, c["moving"], c["V"]))
        assert out.volsize == c["size"] and np.corrcoef(np.sqrt(np.maximum(c["fixed"].T, 0)).reshape(-1), out.vol.reshape(-1))[0, 1] > 0.9


def test_mri_register_device_on_a_side_stream_with_the_caller_s_workspace(fj):
    import torch
    c = R.case("28")
    reg = fj.register
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        mov = _dev(np.stack([c["moving"], c["moving"]]).reshape(2, -1))
        fix = _dev(c["fixed"].reshape(-1))
        work = torch.empty(reg.reg_run_work_size(c["size"], c["size"], 2, 2, 1, 32) // 8 + 2, dtype=torch.int64, device="cuda")
    st.synchronize()
    res = reg.mri_register_device(mov, c["size"], c["V"], fix, c["size"], (2.0, 2.0, 2.0), c["V"], dof=6, levels=1, work=work, stream=st)
    assert len(res) == 2
    for theta, cost, rows in res:
        assert np.array_equal(theta, c["theta"]) and np.array_equal(rows[:, :4], c["trace"][:, :4]) and abs(cost - c["cost"]) <= 1e-10 * abs(c["cost"])
    with pytest.raises(reg.ArgError):                          # a short workspace
        reg.mri_register_device(mov, c["size"], c["V"], fix, c["size"], (2.0, 2.0, 2.0), c["V"], levels=1, work=work[:16], stream=st)
    with pytest.raises(reg.ArgError):                          # mismatched sizes
        reg.mri_register_device(mov, (28, 24, 21), c["V"], fix, c["size"], (2.0, 2.0, 2.0), c["V"], levels=1)


# ---- dwi_moco -----------------------------------------------------------------------------------------------------------------------
MOCO_THETA = ((0.0, 0.0, 0.0, 0.0, 0.0, 0.0), (1.7, -1.1, 0.9, 3.0, -2.5, 4.0), (-0.8, 0.6, 0.0, -1.5, 0.5, 1.0), (0.5, 1.4, -1.2, 2.0, 2.0, -3.0),
              (-1.5, -0.4, 0.7, 0.0, -3.5, 1.5))
MOCO_BVAL = (0.0, 1000.0, 0.0, 1000.0, 1000.0)


def _moco_case():
    size = (28, 24, 20)
    frames = [R.phantom_pair(size, th, kind=int(b > 0))[1] for th, b in zip(MOCO_THETA, MOCO_BVAL)]
    rng = np.random.default_rng(6)
    bvec = rng.normal(size=(5, 3))
    bvec = (bvec / np.linalg.norm(bvec, axis=1, keepdims=True)).astype(F)
    bvec[[0, 2]] = 0
    return size, np.stack(frames), R.geometry(size), bvec


def test_dwi_moco_frame_by_frame_as_the_restatement(fj):
    """5 frames of 28x24x20, each moved by its own theta, two contrasts: theta and trace per frame as restated, the output series bit
    for bit vol_xform_ref through the same matrices, bvec within one rounding, and one frame at a time gives the batched theta"""
    size, series, V, bvec = _moco_case()
    dwi = _mri(fj, series, V, bval=np.array(MOCO_BVAL, F), bvec=bvec)
    m = fj.dwi_moco(dwi)
    # the restatement: the target is the float64 mean of the b = 0 frames, two levels by default
    target = ((series[0].astype(np.float64) + series[2].astype(np.float64)) / 2.0).astype(F)
    levels = R.default_levels(size, size)
    assert levels == 2
    pyr = R.Pyramid(target, series, levels, 32)
    for f in range(5):
        theta, cost, trace, gap, _ = R.search(pyr, f, (size, (2.0, 2.0, 2.0), V), V, dof=6, levels=levels)
        assert gap >= 2.0 ** -30
        assert np.array_equal(m.theta[f], theta), (f, m.theta[f], theta)
        _check_trace(m.trace[f], trace)
        assert abs(m.cost[f] - cost) <= 1e-10 * abs(cost)
        M = R.reg_matrix(theta, V, size, V, 0)
        want = vref.vol_xform_ref(M, series[f], size, size, "trilinear", F(0))[0]
        assert np.array_equal(np.ascontiguousarray(m.dwi.vol[..., f].T).view(np.uint32), want.view(np.uint32))
        wb = R.rotate_bvec(bvec[f], R.xfm_matrices(theta, V, size, V)[1])[0]
        assert np.abs(m.dwi.bvec[f].astype(np.float64) - wb.astype(np.float64)).max() <= 2.0 ** -24
    assert not m.dwi.bvec[0].any() and not m.dwi.bvec[2].any()
    assert np.array_equal(m.dwi.bval, np.array(MOCO_BVAL, F)) and np.array_equal(m.dwi.vox2ras, V) and m.dwi.volsize == size
    assert len(m.xfm) == 5
    # one frame at a time, against the same target: the theta and the voxels of the batched launches
    tgt = _mri(fj, target, V)
    for f in range(5):
        one = fj.dwi_moco(_mri(fj, series[f:f + 1], V, bval=np.array(MOCO_BVAL[f:f + 1], F), bvec=bvec[f:f + 1]), target=tgt)
        assert np.array_equal(one.theta[0], m.theta[f]) and np.array_equal(one.dwi.vol[..., 0], m.dwi.vol[..., f])


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals(fj):
    import torch
    reg = fj.register
    buf = torch.zeros(4096, dtype=torch.int32, device="cuda")
    fixed, moving = buf[:512].view(torch.float32), torch.ones(512, dtype=torch.float32, device="cuda")
    rf, rm = torch.zeros((1, 4), device="cuda"), torch.zeros((1, 4), device="cuda")
    eye = np.eye(4, dtype=F)[None]
    with pytest.raises(fj.FibersError) as e:                   # hist overlaps the fixed volume
        reg.reg_hist_device(fixed, (8, 8, 8), rf, moving, (8, 8, 8), rm, [0], eye, 8, out=buf[500:564])
    assert e.value.code == -1 and "overlap" in str(e.value)
    for nb in (7, 65):
        with pytest.raises(fj.FibersError):
            reg.reg_hist_device(fixed, (8, 8, 8), rf, moving, (8, 8, 8), rm, [0], eye, nb)
        with pytest.raises(fj.FibersError):
            reg.vol_range_device(moving, 512, nb)
    with pytest.raises(fj.FibersError):                        # a job names a frame the series lacks
        reg.reg_hist_device(fixed, (8, 8, 8), rf, moving, (8, 8, 8), rm, [1], eye, 8)
    with pytest.raises(reg.ArgError):                          # mismatched sizes
        reg.reg_hist_device(fixed, (8, 8, 9), rf, moving, (8, 8, 8), rm, [0], eye, 8)
    with pytest.raises(reg.ArgError):
        reg.vol_halve_device(moving, (8, 8, 9))
    with pytest.raises(fj.FibersError):                        # vol_halve in place
        reg.vol_halve_device(moving, (8, 8, 8), out=moving[:64])
    c = R.case("28")
    const = np.full_like(c["fixed"], 3.0)
    for a, b in ((const, c["fixed"]), (c["moving"], const)):
        with pytest.raises(fj.FibersError, match="constant volume"):
            fj.mri_register(_mri(fj, a, c["V"]), _mri(fj, b, c["V"]), levels=1)
    with pytest.raises(fj.FibersError) as e:
        fj.mri_register(_mri(fj, c["moving"], c["V"]), _mri(fj, c["fixed"], c["V"]), device=fj.DEVICE_ALL)
    assert e.value.code == -7
    with pytest.raises(fj.FibersError):
        fj.mri_register(_mri(fj, c["moving"], c["V"]), _mri(fj, c["fixed"], c["V"]), dof=9)
