"""st_recon (structens.jl:40-88) on the GPU against the float64 restatement (tests/st_recon_ref.py): the smoothed tensor, the
eigen-decomposition, the device / host / slabbed forms against each other, NaN containment, and microscopy tracking end to end."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import st_recon_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(1, 5, 4), (3, 17, 9), (33, 20, 11)]
PARAMS = [(0, 0), (1, 0), (0, 2), (1, 2), (1.5, 3)]


def _random(shape, seed=7):
    return np.asfortranarray(np.random.default_rng(seed).normal(size=shape).astype(np.float32))


def _face_trap(shape, seed=8):
    """a ramp with three unequal slopes (large gx*gy, gx*gz, gy*gz everywhere, up to the faces) plus a little noise.  A gradient
    computed past a face flips its normal component, so products formed from such gradients flip the off-diagonal terms there:
    the per-filter reflection of the reference keeps them."""
    x, y, z = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")
    v = 1.0 * x - 0.8 * y + 0.6 * z + 0.05 * np.random.default_rng(seed).normal(size=shape)
    return np.asfortranarray(v.astype(np.float32))


def _device(fj, vol, sigma, rho, **kw):
    import torch
    t = torch.from_numpy(np.asarray(vol).reshape(-1, order="F").copy()).cuda()
    return fj.st_recon_device(t, vol.shape, sigma, rho, **kw)


def _bits(a):
    """float32 -> its bit patterns (bit-identity, NaNs included)"""
    return np.ascontiguousarray(a).view(np.uint32)


def _vol5(a, shape, k):
    """device [k, nvox] -> host [nx,ny,nz,k] (column-major)"""
    return a.cpu().numpy().reshape((k,) + shape[::-1]).transpose(3, 2, 1, 0)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("sigma,rho", PARAMS)
@pytest.mark.parametrize("kind", ["random", "face_trap"])
def test_st_recon_matches_restatement(fj, orc, shape, sigma, rho, kind):
    """S_out against the restatement to 1e-5 of max |S| (this is what catches forming K2's products from gradients computed past
    a face).  Two departures from checking everything against float64 eigh, both forced by the shared 3x3 closed form:
    eigenvalues are held to st_eigen's tolerance (rtol 2e-5, atol 2e-6 max |lambda|) against the oracle's st_eigen of the GPU's
    own S, and to atol 3e-5 max |S| (the S tolerance through Weyl's inequality) against eigh where they are well separated;
    eigenvectors are checked only where no row of S vanishes -- for shape (1, 5, 4), gx = 0, that is no voxel, and that shape's
    vectors rest on test_fused_eigen_is_st_eigen_of_S (bit-identity with fibd_st_eigen)."""
    import torch
    vol = _random(shape) if kind == "random" else _face_trap(shape)
    rvec, rval, rS = ref.st_recon(vol.astype(np.float64), sigma, rho)
    dvec, dval, dS = _device(fj, vol, sigma, rho, S_out=True)
    torch.cuda.synchronize()
    S = _vol5(dS, shape, 6)
    smax = max(np.abs(s).max() for s in rS)
    for c in range(6):
        err = np.abs(S[..., c] - rS[c]).max()
        assert err <= 1e-5 * smax, "S component %d: max error %.3g of max |S| %.3g" % (c, err, smax)

    gvec, gval = fj.st_recon(vol, sigma, rho)
    assert gvec.shape == shape + (3, 3) and gval.shape == shape + (3,)
    lmax = np.abs(rval).max()
    # the eigen-solve against the oracle's StaticArrays closed form on the tensor that was decomposed, at st_eigen's tolerance.  The
    # f32 closed form is itself ~sqrt(eps)-accurate on (near-)degenerate pairs (rank-1 tensors when rho = 0), and its vectors are
    # unreliable (NaN, or a wrong axis) where a row of S vanishes -- a gradient component that is zero by symmetry: nx = 1, or a
    # face voxel when rho = 0.  Those vectors are fibd_st_eigen's (test_fused_eigen_is_st_eigen_of_S); the solver is not this
    # kernel's.  Against float64 eigh where the eigenvalues are well separated and no row vanishes, with the S tolerance above
    # carried over (Weyl: |dlambda| <= |dS|)
    ovec, oval = orc.st_eigen(*[np.asfortranarray(S[..., c]) for c in range(6)])
    np.testing.assert_allclose(gval, oval, rtol=2e-5, atol=2e-6 * lmax)
    zero_row = np.zeros(shape, bool)
    for row in ((0, 1, 2), (1, 3, 4), (2, 4, 5)):
        zero_row |= (np.abs(S[..., row]) <= 1e-6 * smax).all(-1)
    assert not (np.isnan(gvec).any((-2, -1)) & ~zero_row).any(), "NaN eigenvectors of a tensor without a vanishing row"
    gap = np.minimum(rval[..., 1] - rval[..., 0], rval[..., 2] - rval[..., 1])
    well = (gap > 1e-2 * lmax) & ~zero_row
    np.testing.assert_allclose(gval[well], rval[well], rtol=2e-5, atol=3e-5 * smax)
    for j in range(3):
        cos = np.abs((gvec[..., :, j] * rvec[..., :, j]).sum(-1))
        assert (cos[well] > 1 - 1e-4).all(), "eigenvector %d: min |cos| %.6f over %d well-separated voxels" % (
            j, cos[well].min() if well.any() else 1.0, well.sum())


@pytest.mark.parametrize("sigma,rho", [(1, 2), (1.5, 3), (0, 0)])
def test_fused_eigen_is_st_eigen_of_S(fj, sigma, rho):
    import torch
    vol = _face_trap((33, 20, 11))
    dvec, dval, dS = _device(fj, vol, sigma, rho, S_out=True)
    evec, eval_ = fj.st_eigen_device([dS[c].contiguous() for c in range(6)])
    torch.cuda.synchronize()
    assert torch.equal(dvec.view(torch.int32), evec.view(torch.int32)) and torch.equal(dval.view(torch.int32), eval_.view(torch.int32))


def test_device_form_is_host_form_and_z_ranges_compose(fj):
    import torch
    shape, sigma, rho = (33, 20, 23), 1.0, 2.0
    vol = _random(shape, 11)
    gvec, gval = fj.st_recon(vol, sigma, rho)
    dvec, dval = _device(fj, vol, sigma, rho)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(gvec.reshape(-1, order="F")), _bits(dvec.cpu().numpy().ravel()))
    assert np.array_equal(_bits(gval.reshape(-1, order="F")), _bits(dval.cpu().numpy().ravel()))
    # a z-range of outputs from a slab that holds just its halo
    H = fj.st_recon_halo(sigma, rho)
    plane = shape[0] * shape[1]
    for z0, z1 in ((0, 4), (9, 12), (20, 23)):
        zin0, zin1 = max(0, z0 - H), min(shape[2], z1 + H)
        slab = torch.from_numpy(np.ascontiguousarray(vol[:, :, zin0:zin1].reshape(-1, order="F"))).cuda()
        svec, sval = fj.st_recon_device(slab, shape, sigma, rho, zin0=zin0, z0=z0, z1=z1)
        torch.cuda.synchronize()
        assert torch.equal(svec.view(torch.int32), dvec.view(9, shape[2], plane)[:, z0:z1].reshape(9, -1).view(torch.int32))
        assert torch.equal(sval.view(torch.int32), dval.view(3, shape[2], plane)[:, z0:z1].reshape(3, -1).view(torch.int32))
    with pytest.raises(fj.FibersError):                      # one plane short of the halo
        slab = torch.from_numpy(np.ascontiguousarray(vol[:, :, 9 - H + 1:12 + H].reshape(-1, order="F"))).cuda()
        fj.st_recon_device(slab, shape, sigma, rho, zin0=9 - H + 1, z0=9, z1=12)


def test_device_form_on_a_stream_that_is_not_current(fj):
    """the gradient workspace lives across both kernels: launched on a stream other than the current one (a torch stream passed
    in, the current stream inside `with torch.cuda.stream`, a raw handle), allocations made on the default stream right after the
    call must not take it over while the kernels still run"""
    import ctypes as C
    import torch
    shape, sigma, rho = (128, 96, 48), 1.0, 2.0
    vol = _random(shape, 19)
    want_vec, want_val = _device(fj, vol, sigma, rho)
    torch.cuda.synchronize()
    nb = C.c_uint64()
    assert fj.lib().fibd_st_recon_work_size(*shape[:2], shape[2], sigma, rho, C.byref(nb)) == 0
    t = torch.from_numpy(vol.reshape(-1, order="F").copy()).cuda()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    got, junk = [], []
    for how in ("stream=s", "with stream(s)", "raw handle"):
        if how == "stream=s":
            got.append(fj.st_recon_device(t, shape, sigma, rho, stream=s))
        elif how == "with stream(s)":
            with torch.cuda.stream(s):
                got.append(fj.st_recon_device(t, shape, sigma, rho))
        else:
            got.append(fj.st_recon_device(t, shape, sigma, rho, stream=s.cuda_stream))
        junk += [torch.full((nb.value,), 255, dtype=torch.uint8, device="cuda") for _ in range(3)]   # on the default stream
    s.synchronize()
    torch.cuda.synchronize()
    for how, (vec, val) in zip(("stream=s", "with stream(s)", "raw handle"), got):
        assert torch.equal(vec.view(torch.int32), want_vec.view(torch.int32)), how
        assert torch.equal(val.view(torch.int32), want_val.view(torch.int32)), how


def test_slab_thickness_does_not_change_results(fj, monkeypatch):
    shape, sigma, rho = (64, 48, 40), 1.5, 3.0
    assert fj.st_recon_halo(sigma, rho) > 7
    vol = _random(shape, 13)
    monkeypatch.setenv("FIBERS_ST_RECON_SLAB", str(shape[2]))
    vec1, val1 = fj.st_recon(vol, sigma, rho)
    for planes in (7, 1):
        monkeypatch.setenv("FIBERS_ST_RECON_SLAB", str(planes))
        vec, val = fj.st_recon(vol, sigma, rho)
        assert np.array_equal(_bits(vec), _bits(vec1)) and np.array_equal(_bits(val), _bits(val1)), "slab of %d planes" % planes


def test_nan_voxel_stays_in_its_box(fj):
    import torch
    shape, sigma, rho = (40, 36, 32), 1.0, 2.0
    H = fj.st_recon_halo(sigma, rho)
    c = (20, 17, 15)
    assert all(H + 1 <= ci <= n - 2 - H for ci, n in zip(c, shape))
    vol = _random(shape, 17)
    bad = vol.copy(order="F")
    bad[c] = np.nan
    v0, w0, S0 = _device(fj, vol, sigma, rho, S_out=True)
    v1, w1, S1 = _device(fj, bad, sigma, rho, S_out=True)
    torch.cuda.synchronize()
    box = np.zeros(shape, bool)
    box[tuple(slice(ci - H, ci + H + 1) for ci in c)] = True
    w1h, S1h = _vol5(w1, shape, 3), _vol5(S1, shape, 6)
    assert np.array_equal(~np.isfinite(S1h).all(-1), box)
    assert (~np.isfinite(S1h)).all(-1)[box].all()             # every component of the tensor inside the box
    assert np.array_equal(~np.isfinite(w1h).all(-1), box)
    out = ~box.reshape(-1, order="F")
    for a, b in ((v0, v1), (w0, w1), (S0, S1)):
        a, b = a.cpu().numpy(), b.cpu().numpy()
        assert np.array_equal(_bits(a[:, out]), _bits(b[:, out]))


def test_microscopy_tubes_end_to_end(fj):
    """bright parallel tubes along an oblique axis d at 10 um voxels: st_recon's smallest-eigenvalue vector is d inside the
    tubes, and the microscopy-regime tracer follows it"""
    shape, sigma, rho = (64, 64, 48), 1.0, 2.0
    d = np.array([1.0, 0.6, 0.4]); d /= np.linalg.norm(d)
    u = np.cross(d, [0.0, 0.0, 1.0]); u /= np.linalg.norm(u)
    v = np.cross(d, u)
    x = np.stack(np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij"), -1)
    spacing, r = 8.0, 1.5
    a, b = x @ u, x @ v
    da = a - spacing * np.round(a / spacing)
    db = b - spacing * np.round(b / spacing)
    vol = np.asfortranarray(np.exp(-(da * da + db * db) / (2 * r * r)).astype(np.float32))
    m = fj.MRI(vol, volres=(0.01, 0.01, 0.01))
    eigvec, eigval = fj.st_recon(m, sigma, rho)
    e0 = eigvec[..., :, 0]
    H = fj.st_recon_halo(sigma, rho)
    inner = np.zeros(shape, bool)
    inner[H:-H, H:-H, H:-H] = True
    tube = (vol > 0.6) & inner
    assert tube.sum() > 1000
    cos = np.abs(e0 @ d)
    assert (cos[tube] > 0.99).all(), "min |cos(e0, d)| in the tubes: %.4f" % cos[tube].min()

    ov = fj.MRI(np.asfortranarray(e0.astype(np.float32)), volres=(0.01, 0.01, 0.01))
    mask = fj.MRI(np.ones(shape, np.uint8), volres=(0.01, 0.01, 0.01))
    idx = np.argwhere(tube)[::max(1, int(tube.sum()) // 200)]
    seed = np.zeros(shape, np.uint8)
    seed[tuple(idx.T)] = 1
    tr = fj.stream(ov, mask=mask, seed=fj.MRI(seed, volres=(0.01, 0.01, 0.01)), nsub=None, len_min=3)
    nseed = int(seed.sum())
    assert tr.nstr >= nseed // 2, "%d lines from %d seeds" % (tr.nstr, nseed)
    offs = np.concatenate([[0], np.cumsum(tr.npts)])
    coss = []
    for i in range(tr.nstr):
        p = tr.xyz[offs[i]:offs[i + 1]].astype(np.float64)
        s = np.diff(p, axis=0)
        n = np.linalg.norm(s, axis=1)
        s = s[n > 0] / n[n > 0, None]
        coss.append(np.abs(s @ d))
    coss = np.concatenate(coss)
    assert coss.mean() > 0.95, "mean |cos(step, d)| %.4f" % coss.mean()
