"""dwi_denoise on the GPU against the float64 restatement (tests/denoise_ref.py): every case and estimator through the device tier and
through fib_dwi_denoise, held to |gpu - ref64| <= 4 d + 2^-23 |ref64| with equal rank in every voxel (d: the case's own difference
between the restatement's two routes; the second term is the one rounding to float32); masks, slabs, determinism, the workspace and
argument contracts, and the tensor fit of the denoised series end to end."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import denoise_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = pytest.mark.parametrize("case", ref.CASES, ids=ref.case_id)
ESTS = pytest.mark.parametrize("estimator", ref.ESTIMATORS)
MID = ref.CASES[2]                    # 7x6x5, N = 30, P = 5


def _planar(vol):
    """host [nx,ny,nz,N] -> device [N, nvox]"""
    import torch
    N = vol.shape[3]
    return torch.from_numpy(np.array(vol.reshape(-1, N, order="F").T, order="C")).cuda()     # (a copy: the shared volumes are read-only)


def _host(t, shape):
    """device [k, nvox] or [nvox] -> host [nx,ny,nz,k] or [nx,ny,nz]"""
    a = t.cpu().numpy()
    return a.reshape(shape, order="F") if a.ndim == 1 else a.T.reshape(shape + (a.shape[0],), order="F")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _device(fj, vol, P, estimator="exp2", mask=None, **kw):
    import torch
    shape = vol.shape[:3]
    m = torch.ones(int(np.prod(shape)), dtype=torch.uint8, device="cuda") if mask is None else \
        torch.from_numpy(np.ascontiguousarray(mask.reshape(-1, order="F").astype(np.uint8))).cuda()
    o = fj.denoise.dwi_denoise_device(_planar(vol), m, shape, P, estimator, **kw)
    torch.cuda.synchronize()
    return _host(o["dwi"], shape), _host(o["sigma"], shape), _host(o["rank"], shape)


def _hold(got, case, estimator):
    dwi, sigma, rank = got
    a, _, d_rows, d_sigma = ref.case_reference(case, estimator)
    assert np.array_equal(rank, a["rank"]), "rank differs in %d voxels" % np.count_nonzero(rank != a["rank"])
    err, tol = np.abs(dwi - a["dwi"]), 4 * d_rows + 2.0 ** -23 * np.abs(a["dwi"])
    es, ts = np.abs(sigma - a["sigma"]), 4 * d_sigma + 2.0 ** -23 * np.abs(a["sigma"])
    print("%s %s: rows %.3g of the tolerance (d %.3g), sigma %.3g (d %.3g)" % (ref.case_id(case), estimator, (err / tol).max(), d_rows,
                                                                              (es / ts).max(), d_sigma))
    assert np.all(err <= tol) and np.all(es <= ts)


@CASES
@ESTS
def test_device_tier_matches_restatement(fj, case, estimator):
    _hold(_device(fj, ref.case_volume(case), case[2], estimator), case, estimator)


@CASES
@ESTS
def test_host_form_matches_restatement(fj, case, estimator):
    r = fj.dwi_denoise(fj.MRI(ref.case_volume(case)), patch=case[2], estimator=estimator)
    _hold((r.dwi.vol, r.sigma.vol[..., 0], r.rank.vol[..., 0]), case, estimator)


@pytest.mark.parametrize("case", [ref.CASES[1], MID], ids=ref.case_id)
def test_partial_mask(fj, case):
    """checkerboard plus one empty z-plane: zero outside; inside, the bits of the full mask's result (the patch ignores the mask)"""
    vol = ref.case_volume(case)
    x, y, z = np.meshgrid(*[np.arange(n) for n in vol.shape[:3]], indexing="ij")
    m = ((x + y + z) % 2 == 0) & (z != 1)
    full, part = _device(fj, vol, case[2]), _device(fj, vol, case[2], mask=m)
    for f, p in zip(full, part):
        assert not p[~m].any() and np.array_equal(_bits(p[m]), _bits(f[m]))
    r = fj.dwi_denoise(fj.MRI(vol), mask=fj.MRI(m.astype(np.float32)), patch=case[2])
    for f, p in zip(full, (r.dwi.vol, r.sigma.vol[..., 0], r.rank.vol[..., 0])):
        assert not p[~m].any() and np.array_equal(_bits(p[m]), _bits(f[m]))


@pytest.mark.parametrize("case", [ref.CASES[1], MID, ref.CASES[6]], ids=ref.case_id)
def test_slabs_that_hold_just_their_halo(fj, case):
    import torch
    vol, P = ref.case_volume(case), case[2]
    nx, ny, nz, N = vol.shape
    whole = _device(fj, vol, P)
    for z0, z1 in [(0, 1), (1, 3), (nz - 2, nz), (nz // 2, nz // 2 + 1), (0, nz)]:
        zin0 = ref.patch_start(z0, nz, P)
        zin1 = ref.patch_start(z1 - 1, nz, P) + P
        slab = _planar(np.asfortranarray(vol[:, :, zin0:zin1]))
        m = torch.ones(nx * ny * (z1 - z0), dtype=torch.uint8, device="cuda")
        o = fj.denoise.dwi_denoise_device(slab, m, (nx, ny, nz), P, zin0=zin0, z0=z0, z1=z1)
        sshape = (nx, ny, z1 - z0)
        for w, k in zip(whole, ("dwi", "sigma", "rank")):
            assert np.array_equal(_bits(_host(o[k], sshape)), _bits(w[:, :, z0:z1])), (k, z0, z1)
        if zin1 - zin0 > P or zin0 > 0:                        # one plane less on either side is refused, not read past
            for lo, hi, zi in ((zin0 + 1, zin1, zin0 + 1), (zin0, zin1 - 1, zin0)):
                short = _planar(np.asfortranarray(vol[:, :, lo:hi]))
                with pytest.raises(fj.FibersError, match="need"):
                    fj.denoise.dwi_denoise_device(short, m, (nx, ny, nz), P, zin0=zi, z0=z0, z1=z1)


def test_slab_thickness_of_the_host_form(fj, monkeypatch):
    vol, P = ref.case_volume(MID), MID[2]
    outs = []
    for nzs in (None, 1, 2, vol.shape[2]):
        if nzs is None:
            monkeypatch.delenv("FIBERS_DENOISE_SLAB", raising=False)
        else:
            monkeypatch.setenv("FIBERS_DENOISE_SLAB", str(nzs))
        r = fj.dwi_denoise(fj.MRI(vol), patch=P)
        outs.append((r.dwi.vol, r.sigma.vol, r.rank.vol))
    for o in outs[1:]:
        for a, b in zip(outs[0], o):
            assert np.array_equal(_bits(a), _bits(b))
    dev = _device(fj, vol, P)
    assert np.array_equal(_bits(dev[0]), _bits(outs[0][0]))


def test_two_runs_give_identical_bits(fj):
    case = ref.CASES[3]
    a, b = _device(fj, ref.case_volume(case), case[2]), _device(fj, ref.case_volume(case), case[2])
    for u, v in zip(a, b):
        assert np.array_equal(_bits(u), _bits(v))


def test_workspace_contract(fj):
    import torch
    vol, P = ref.case_volume(MID), MID[2]
    nx, ny, nz, N = vol.shape
    need = fj.denoise.dwi_denoise_work_size(nx, ny, nz, N, P)
    assert need == 256 + min(nx * ny * nz, 512) * 24 * 29 * 15 * 8
    own = _device(fj, vol, P)
    exact = _device(fj, vol, P, work=torch.empty(need, dtype=torch.uint8, device="cuda"))
    for u, v in zip(own, exact):
        assert np.array_equal(_bits(u), _bits(v))
    with pytest.raises(fj._dev.ArgError, match="dwi_denoise_work_size"):
        _device(fj, vol, P, work=torch.empty(need - 1, dtype=torch.uint8, device="cuda"))
    with pytest.raises(fj._dev.ArgError, match="work"):
        _device(fj, vol, P, work=torch.empty(need, dtype=torch.uint8))
    # the C entry refuses a short workspace itself
    d, m, w = _planar(vol), torch.ones(nx * ny * nz, dtype=torch.uint8, device="cuda"), torch.empty(need // 8 + 1, dtype=torch.int64, device="cuda")
    o = torch.empty((N + 2) * nx * ny * nz, dtype=torch.float32, device="cuda")
    rc = fj.lib().fibd_dwi_denoise(d.data_ptr(), nx, ny, nz, 0, nz, 0, nz, N, P, 2, m.data_ptr(), o.data_ptr(), o.data_ptr(), o.data_ptr(),
                                   w.data_ptr(), need - 1, None)
    assert rc == -1 and b"fibd_dwi_denoise_work_size" in fj.lib().fib_last_error()


def test_device_arguments_are_checked_before_a_launch(fj, monkeypatch):
    import torch
    from fibers_jl_amd import _lib
    shape, N, P = (6, 5, 4), 16, 3
    nvox = 120
    good = dict(dwi=torch.zeros((N, nvox), dtype=torch.float32, device="cuda"), mask=torch.ones(nvox, dtype=torch.uint8, device="cuda"))
    bad = {"dwi": [good["dwi"].double(), good["dwi"].cpu(), torch.zeros((N, nvox - 1), dtype=torch.float32, device="cuda"),
                   torch.zeros((N, 2 * nvox), dtype=torch.float32, device="cuda")[:, ::2], good["dwi"].reshape(-1)],
           "mask": [good["mask"].to(torch.int32), good["mask"].cpu(), good["mask"][:-1].clone(),
                    torch.ones(2 * nvox, dtype=torch.uint8, device="cuda")[::2]]}
    if torch.cuda.device_count() > 1:
        bad["mask"].append(good["mask"].to("cuda:1"))
    outs = dict(dwi=torch.zeros((N, nvox), dtype=torch.float32, device="cuda"), sigma=torch.zeros(nvox, dtype=torch.float32, device="cuda"),
                rank=torch.zeros(nvox, dtype=torch.float32, device="cuda"))
    fj.denoise.dwi_denoise_device(good["dwi"], good["mask"], shape, P, out=outs)             # the valid call goes through
    monkeypatch.setattr(_lib, "lib", lambda: pytest.fail("the library was reached with a bad argument"))
    for k, ts in bad.items():
        for t in ts:
            with pytest.raises(fj._dev.ArgError):
                fj.denoise.dwi_denoise_device(shape=shape, patch=P, **dict(good, **{k: t}))
    for k in outs:
        for t in (outs[k].double(), outs[k].cpu(), outs[k].reshape(-1)[:-1].clone()):
            with pytest.raises(fj._dev.ArgError):
                fj.denoise.dwi_denoise_device(good["dwi"], good["mask"], shape, P, out=dict(outs, **{k: t}))
    with pytest.raises(fj._dev.ArgError, match="output planes"):
        fj.denoise.dwi_denoise_device(good["dwi"], good["mask"], shape, P, z0=2, z1=2)


def test_gpu_refusals(fj):
    import torch
    nvox = 8 * 7 * 7
    d, m = torch.zeros((129, nvox), dtype=torch.float32, device="cuda"), torch.ones(nvox, dtype=torch.uint8, device="cuda")
    with pytest.raises(fj.FibersError) as e:
        fj.denoise.dwi_denoise_device(d, m, (8, 7, 7), 7)
    assert e.value.code == -7 and "P = 7 with N = 129" in str(e.value) and "128" in str(e.value)
    with pytest.raises(fj.FibersError) as e:
        fj.dwi_denoise(fj.MRI(np.zeros((3, 3, 3, 4), np.float32)), device=fj.DEVICE_ALL)
    assert e.value.code == -7
    # an all-zero volume: zero rows, sigma 0, rank r
    r = fj.dwi_denoise(fj.MRI(np.zeros((4, 3, 3, 5), np.float32)), patch=3)
    assert not r.dwi.vol.any() and not r.sigma.vol.any() and np.all(r.rank.vol == 5)


# ---- above the cap: more output voxels than persistent workgroups ---------------------------------------------------------------------
DN_MAXWG = 512                        # csrc/denoise.hip: the persistent workgroups of dwi_denoise_kernel, one output voxel a ticket
L1, L2, L3 = ref.LARGE_CASES
_WHOLE = {}


def _above_the_cap(nout, what):
    """the precondition of every test below: each of the DN_MAXWG workgroups takes a second ticket, most a third"""
    print("%s: %d output voxels over DN_MAXWG = %d workgroups (csrc/denoise.hip): %.1f tickets a workgroup" % (what, nout, DN_MAXWG, nout / DN_MAXWG))
    assert nout > 2 * DN_MAXWG, "%s: %d output voxels do not send every one of DN_MAXWG = %d workgroups (csrc/denoise.hip) round its loop " \
                                "twice; resize ref.LARGE_CASES" % (what, nout, DN_MAXWG)


def _whole(fj, case, estimator="exp2"):
    """one device call over the whole volume of a large case, run once and shared; do not modify"""
    if (case, estimator) not in _WHOLE:
        _above_the_cap(int(np.prod(case[0])), ref.case_id(case))
        _WHOLE[case, estimator] = _device(fj, ref.case_volume(case), case[2], estimator)
    return _WHOLE[case, estimator]


@pytest.mark.parametrize("case,estimator", ref.LARGE_HELD, ids=lambda v: v if isinstance(v, str) else ref.case_id(v))
def test_above_the_workgroup_cap_device_tier_matches_restatement(fj, case, estimator):
    """2197 and 1100 output voxels against DN_MAXWG = 512 workgroups (csrc/denoise.hip): whatever G, y, lam, step_rot, s_cut, s_sig2
    and the rotation records keep of a workgroup's previous voxel would show here, by the pass rule of the small cases"""
    _hold(_whole(fj, case, estimator), case, estimator)


def test_above_the_workgroup_cap_host_form_matches_restatement(fj):
    _above_the_cap(int(np.prod(L1[0])), "host form, " + ref.case_id(L1))
    r = fj.dwi_denoise(fj.MRI(ref.case_volume(L1)), patch=L1[2], estimator="exp2")
    _hold((r.dwi.vol, r.sigma.vol[..., 0], r.rank.vol[..., 0]), L1, "exp2")


@pytest.mark.parametrize("case,planes", [(L1, 3), (L2, 3), (L3, 4)], ids=lambda v: ref.case_id(v) if isinstance(v, tuple) else "%dplanes" % v)
def test_whole_volume_equals_slabs_below_the_workgroup_cap(fj, case, planes):
    """one call with nout > 2 DN_MAXWG (csrc/denoise.hip) against the same volume in z-slabs of at most DN_MAXWG = 512 output voxels,
    where no workgroup takes a second ticket, each slab holding exactly its halo: dwi, sigma and rank bit for bit"""
    import torch
    vol, P = ref.case_volume(case), case[2]
    nx, ny, nz, N = vol.shape
    whole = _whole(fj, case)
    assert nx * ny * planes <= DN_MAXWG, "a slab of %d planes has %d output voxels, more than DN_MAXWG = %d" % (planes, nx * ny * planes, DN_MAXWG)
    for z0 in range(0, nz, planes):
        z1 = min(z0 + planes, nz)
        zin0 = ref.patch_start(z0, nz, P)
        zin1 = ref.patch_start(z1 - 1, nz, P) + P
        slab = _planar(np.asfortranarray(vol[:, :, zin0:zin1]))
        m = torch.ones(nx * ny * (z1 - z0), dtype=torch.uint8, device="cuda")
        o = fj.denoise.dwi_denoise_device(slab, m, (nx, ny, nz), P, zin0=zin0, z0=z0, z1=z1)
        for w, k in zip(whole, ("dwi", "sigma", "rank")):
            got = _host(o[k], (nx, ny, z1 - z0))
            assert np.array_equal(_bits(got), _bits(w[:, :, z0:z1])), "%s of planes [%d, %d): %d values differ" % (
                k, z0, z1, np.count_nonzero(_bits(got) != _bits(w[:, :, z0:z1])))


def test_a_mask_that_interleaves_the_skip_and_the_solve(fj):
    """every third voxel (by linear index) and one whole z-plane masked out, above DN_MAXWG = 512 (csrc/denoise.hip): successive tickets
    alternate between the masked `continue` and a full solve.  Zero outside; inside, the bits of the full mask's run."""
    vol, P = ref.case_volume(L2), L2[2]
    nx, ny, nz, N = vol.shape
    lin = np.arange(nx * ny * nz).reshape((nx, ny, nz), order="F")
    m = (lin % 3 != 0) & (lin // (nx * ny) != 6)
    assert not m[:, :, 6].any() and m[1, 0, 0] and not m[0, 0, 0] and m.sum() > 2 * DN_MAXWG
    full, part = _whole(fj, L2), _device(fj, vol, P, mask=m)
    for f, p, k in zip(full, part, ("dwi", "sigma", "rank")):
        assert not p[~m].any(), k + " is not zero outside the mask"
        assert np.array_equal(_bits(p[m]), _bits(f[m])), "%s: %d values differ inside the mask" % (k, np.count_nonzero(_bits(p[m]) != _bits(f[m])))


def test_two_runs_above_the_workgroup_cap_give_identical_bits(fj):
    """which workgroup draws which ticket differs from run to run; above DN_MAXWG = 512 (csrc/denoise.hip) so does what it solved before"""
    a, b = _whole(fj, L2), _device(fj, ref.case_volume(L2), L2[2])
    for u, v in zip(a, b):
        assert np.array_equal(_bits(u), _bits(v))


def test_workspace_above_the_workgroup_cap(fj):
    """the workspace is DN_MAXWG = 512 (csrc/denoise.hip) rotation records whatever the volume: exactly that size serves, a byte less
    is refused"""
    import torch
    vol, P = ref.case_volume(L2), L2[2]
    nx, ny, nz, N = vol.shape
    _above_the_cap(nx * ny * nz, "workspace, " + ref.case_id(L2))
    n = 28                                                      # r = 27 rounded up to even
    need = fj.denoise.dwi_denoise_work_size(nx, ny, nz, N, P)
    assert need == 256 + DN_MAXWG * 24 * (n - 1) * (n // 2) * 8
    exact = _device(fj, vol, P, work=torch.empty(need, dtype=torch.uint8, device="cuda"))
    for u, v in zip(_whole(fj, L2), exact):
        assert np.array_equal(_bits(u), _bits(v))
    with pytest.raises(fj._dev.ArgError, match="dwi_denoise_work_size"):
        _device(fj, vol, P, work=torch.empty(need - 1, dtype=torch.uint8, device="cuda"))


def test_tensor_fit_of_the_denoised_series(fj):
    """dti_fit(dwi_denoise(dwi).dwi, mask) against dti_fit of the restatement's float32 output: fa to DESIGN.md §5's DTI tolerance"""
    from fibers_jl_amd import phantom
    shape, N, P, k = MID
    bval, bvec = phantom.scheme_dti(N - 1, 1)
    assert len(bval) == N
    vol = ref.case_volume(MID)
    mask = fj.MRI(np.ones(shape, np.uint8))
    den = fj.dwi_denoise(fj.MRI(vol, bval, bvec), patch=P)
    assert den.dwi.bval is not None and np.array_equal(den.dwi.bval, np.asarray(bval, np.float32))
    got = fj.dti_fit(den.dwi, mask)
    want = fj.dti_fit(fj.MRI(np.asfortranarray(ref.case_reference(MID, "exp2")[0]["dwi"].astype(np.float32)), bval, bvec), mask)
    assert np.isfinite(got.fa.vol).all()
    assert np.allclose(got.fa.vol, want.fa.vol, atol=1e-4)
