"""The NumPy restatement of rumba_rec (tests/rumba_ref.py) checked on the CPU: against the float32 oracle (oracle.rumba_rec), against
known answers of the TV term and of zero iterations, and the argument checks that come back before any device call."""
import numpy as np
import pytest

import rumba_ref as R

FIB_ERR_UNSUPPORTED = -7                                                   # include/fibers_hip.h

CONFIGS = [                                                                # (use_tv, ipat_factor, coil_combine, ncoils)
    (True, 1, "SMF-SENSE", 1), (False, 1, "SMF-SENSE", 1), (True, 2, "SMF-SENSE", 1),
    (True, 1, "SoS-GRAPPA", 1), (True, 1, "SoS-GRAPPA", 4), (False, 2, "SoS-GRAPPA", 4),
]


@pytest.fixture(scope="module")
def case():
    from fibers_jl_amd import phantom
    bval, bvec = phantom.scheme_gqi(3, 30, (1000.0, 2500.0), 5)
    shape = (7, 6, 5)
    dwi, _, _ = phantom.make_volume(shape, bval, bvec, 5, noise_frac=0.03, crossing=True)
    mask = (np.random.default_rng(6).random(shape) < 0.85).astype(np.uint8)
    dwi[1, 1, 1, :] = 0.0                                                  # a masked voxel without signal
    mask[1, 1, 1] = 1
    return dwi, mask, bval, bvec


@pytest.mark.parametrize("niter", [0, 1, 3, 10])
@pytest.mark.parametrize("use_tv,ipat,coil,ncoils", CONFIGS)
def test_restatement_matches_oracle(fj, orc, case, niter, use_tv, ipat, coil, ncoils):
    """float32 and float64 runs of the restatement agree with the oracle at the float32 level (measured: float32 is the oracle to
    the bit on every configuration here; float64 is within 2e-6 of each field's maximum, GFA within 2e-7)"""
    dwi, mask, bval, bvec = case
    sph = fj.sphere_724
    kw = dict(ncoils=ncoils, coil_combine=coil, ipat_factor=ipat, use_tv=use_tv)
    o = orc.rumba_rec(dwi, mask, bval, bvec, sph.vertices, niter=niter, **kw)
    for dt in (np.float32, np.float64):
        r = R.rumba_ref(dwi, mask, bval, o["kernel"], sph.vertices, niter, dtype=dt, **kw)
        for k in ("fodf", "fgm", "fcsf", "gfa", "var"):
            err = np.abs(r[k] - o[k]).max()
            scale = 1.0 if k == "gfa" else np.abs(o[k]).max()              # (GFA lies in [0, 1]; it is ~0 without iterations)
            assert err <= 1e-5 * scale, "%s %s: %g" % (dt.__name__, k, err)
        for k in ("snr_mean", "snr_std"):
            assert abs(r[k] - o[k]) <= 1e-6 * max(abs(o[k]), 1.0), "%s %s: %r vs %r" % (dt.__name__, k, r[k], o[k])
        for k in range(5):
            np.testing.assert_allclose(r["peak"][k], o["peak"][k], rtol=0, atol=1e-6)
        m = mask.reshape(-1, order="F") > 0
        assert (r["fodf"].reshape(-1, sph.nvert, order="F")[~m] == 0).all()


def test_niter_zero_known_answer(fj, case):
    """no iteration: every masked fODF is uniform (1/nvert), GFA 0, no peaks, var = (1/15)^2, SNR statistics 0"""
    dwi, mask, bval, bvec = case
    sph = fj.sphere_642
    K = np.ones((int((bval > bval.min()).sum()) + 1, sph.nvert + 2), np.float32)   # (K plays no part without iterations)
    m = mask.astype(bool)
    for dt, tol in ((np.float64, 1e-15), (np.float32, 1e-6)):
        r = R.rumba_ref(dwi, mask, bval, K, sph.vertices, 0, dtype=dt)
        np.testing.assert_allclose(r["fodf"][m], 1.0 / sph.nvert, rtol=tol)
        assert (r["fodf"][~m] == 0).all()
        assert np.abs(r["gfa"]).max() <= tol
        assert all((p == 0).all() for p in r["peak"]) and (r["peak_vertex"] == -1).all()
        np.testing.assert_allclose(r["var"][m], 1.0 / 225.0, rtol=tol)
        assert r["snr_mean"] == 0.0 and r["snr_std"] == 0.0


@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_tv_constant_volume(dt):
    """a constant volume has no gradient: div = 0 and tv = 1 / (1 + eps) everywhere, faces included"""
    vol = np.full((5, 4, 6, 3), dt(0.37), dt)
    tv = R.tv_term(vol, dt(0.01))
    assert (tv == dt(1) / (dt(1) + dt(R.EPS32))).all()


def test_tv_linear_ramp_along_x():
    """f = a x + b along x: interior divergence 0 (tv = 1 / (1 + eps)); at x = 1 div = +g, at x = nx div = -g, g = a / sqrt(a^2 + eps)"""
    nz, ny, nx = 3, 4, 9
    a, lam = 0.02, 0.3
    x = np.arange(nx, dtype=np.float64)
    vol = np.broadcast_to(a * x + 0.5, (nz, ny, nx))[..., None].copy()
    tv = R.tv_term(vol, lam)[..., 0]
    g = a / np.sqrt(a * a + R.EPS32)
    np.testing.assert_allclose(tv[:, :, 1:-1], 1 / (1 + R.EPS32), rtol=1e-15)
    np.testing.assert_allclose(tv[:, :, 0], 1 / (abs(1 - lam * g) + R.EPS32), rtol=1e-14)
    np.testing.assert_allclose(tv[:, :, -1], 1 / (abs(1 + lam * g) + R.EPS32), rtol=1e-14)


def _sd_div_literal(Gx, Gy, Gz):
    """sd_div! (rusd.jl:194-207) transcribed with 1-based indices, element by element; arrays indexed [x, y, z]"""
    nx, ny, nz = Gx.shape
    D = np.zeros_like(Gx)
    at = lambda A, i, j, k: A[i - 1, j - 1, k - 1]                                  # noqa: E731
    for i in range(1, nx + 1):
        for j in range(1, ny + 1):
            for k in range(1, nz + 1):
                d = at(Gx, i, j, k) - at(Gx, i - 1, j, k) if 2 <= i <= nx - 1 else (at(Gx, 1, j, k) if i == 1 else -at(Gx, nx - 1, j, k))
                d += at(Gy, i, j, k) - at(Gy, i, j - 1, k) if 2 <= j <= ny - 1 else (at(Gy, i, 1, k) if j == 1 else -at(Gy, i, ny - 1, k))
                d += at(Gz, i, j, k) - at(Gz, i, j, k - 1) if 2 <= k <= nz - 1 else (at(Gz, i, j, 1) if k == 1 else -at(Gz, i, j, nz - 1))
                D[i - 1, j - 1, k - 1] = d
    return D


@pytest.mark.parametrize("shape", [(2, 3, 2), (3, 2, 3), (2, 2, 2), (3, 3, 3), (4, 2, 3)])
def test_sd_div_matches_literal_transcription(shape):
    """the vectorised divergence, boundary rows included, equals a 1-based element loop of sd_div! on axes of length 2 and 3"""
    rng = np.random.default_rng(sum(shape))
    Gx, Gy, Gz = (rng.normal(size=shape) for _ in range(3))
    want = _sd_div_literal(Gx, Gy, Gz)
    t = lambda A: np.ascontiguousarray(A.transpose(2, 1, 0))                        # noqa: E731  [x,y,z] -> [z,y,x]
    got = (R.sd_div(t(Gx), 2) + R.sd_div(t(Gy), 1)) + R.sd_div(t(Gz), 0)
    np.testing.assert_array_equal(got, t(want))


def test_singleton_axis_adds_nothing():
    """length-1 axis (the reference throws BoundsError): its forward difference is 0, so the TV of a (nx, ny, 1) volume is
    the 2-D TV of its slice: equal to the TV of the slice repeated along z, where the z gradients vanish too"""
    rng = np.random.default_rng(3)
    sl = rng.random((1, 5, 6, 4))
    tv1 = R.tv_term(sl, 0.05)
    tv3 = R.tv_term(np.repeat(sl, 3, axis=0), 0.05)
    for z in range(3):
        np.testing.assert_array_equal(tv1[0], tv3[z])


def test_besseli_ratio_is_the_truncated_fraction():
    """rusd.jl:170-177 as written (four levels), in the argument's float type; n_order = 1 and ncoils"""
    z = np.array([0.0, 1e-3, 0.5, 3.0, 40.0])
    for nu in (1, 4, 8):
        a = 2 * nu
        want = z / ((a + z) - ((a + 1) * z / (2 * z + (a + 1) - ((a + 3) * z / ((a + 2) + 2 * z - ((a + 5) * z / ((a + 3) + 2 * z)))))))
        np.testing.assert_array_equal(R.besseli_ratio(nu, z), want)
        assert R.besseli_ratio(nu, z.astype(np.float32)).dtype == np.float32


def test_arguments_rejected_before_any_device_call(fj, case):
    """an unsupported tessellation (rusd.jl:476-480 defines the peak neighbourhood for three spheres), ipat_factor < 1 (:437) and an
    unknown coil combination (:433) fail before the library touches a GPU"""
    dwi, mask, bval, bvec = case
    v = fj.sphere_362.vertices
    odd = fj.ODF(np.ascontiguousarray(np.vstack([v[:100], -v[:100]])), fj.sphere_362.faces)
    with pytest.raises(fj.FibersError) as e:
        fj.rumba_rec(fj.MRI(dwi, bval, bvec), fj.MRI(mask), odd, niter=1)
    assert e.value.code == FIB_ERR_UNSUPPORTED
    with pytest.raises(fj.FibersError) as e:
        fj.RumbaPlan(bval, bvec, odd)
    assert e.value.code == FIB_ERR_UNSUPPORTED
    with pytest.raises(ValueError, match="iPAT factor"):
        fj.rumba_rec(fj.MRI(dwi, bval, bvec), fj.MRI(mask), fj.sphere_362, niter=1, ipat_factor=0)
    with pytest.raises(ValueError, match="Unknown coil combine mode foo"):
        fj.rumba_rec(fj.MRI(dwi, bval, bvec), fj.MRI(mask), fj.sphere_362, niter=1, coil_combine="foo")
    with pytest.raises(ValueError, match="Unknown coil combine mode foo"):
        R.rumba_ref(dwi, mask, bval, np.ones((2, 183), np.float32), fj.sphere_362.vertices, 1, coil_combine="foo")
    with pytest.raises(ValueError, match="iPAT factor"):
        R.rumba_ref(dwi, mask, bval, np.ones((2, 183), np.float32), fj.sphere_362.vertices, 1, ipat_factor=0)
