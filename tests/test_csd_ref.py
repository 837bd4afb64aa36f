"""CSD without a GPU: fib_csd_design against the float64 restatement (tests/csd_ref.py), the frame selection and the two refusals, and
the restatement's own known answers (what the GPU tests then hold the kernel to)."""
import numpy as np
import pytest

import csd_ref
from fibers_jl_amd import phantom  # noqa: F401

RESP = (1.7e-3, 0.3e-3, 1000.0)


_scheme = csd_ref.scheme


def _near(got, want64):
    """got equals the float32 rounding of want64 or that value's float32 neighbour -- or differs from want64 by less than the
    restatement's own float64 evaluation error, 8 eps64 max|table| absolute (lpmv and sin(m phi) are accurate in absolute terms): an
    entry that is zero in exact arithmetic (a vertex in the xz plane or on the equator) is 1e-15 in either computation, with no
    digit in common and no meaningful float32 neighbour.  For every other entry the first rule is the one that binds."""
    want64 = np.asarray(want64, np.float64)
    w = want64.astype(np.float32)
    got = np.asarray(got, np.float32)
    lo, hi = np.nextafter(w, np.float32(-np.inf)), np.nextafter(w, np.float32(np.inf))
    tiny = 8 * np.finfo(np.float64).eps * np.abs(want64).max()
    return bool(np.all((got == w) | (got == lo) | (got == hi) | (np.abs(got.astype(np.float64) - want64) <= tiny)))


@pytest.mark.parametrize("lmax", [2, 4, 6, 8])
@pytest.mark.parametrize("sphere", ["sphere_362", "sphere_642", "sphere_724"])
def test_design_tables_match_the_restatement(fj, lmax, sphere):
    sph = getattr(fj, sphere)
    bval, bvec = _scheme()
    got = fj.csd_design(bval, bvec, RESP, sph, lmax=lmax, lam=0.7)
    ref = csd_ref.design(bval, bvec, sph.vertices, RESP, lmax=lmax, lam=0.7)
    n = csd_ref.ncoef(lmax)
    assert got["rank"] == n
    assert np.array_equal(got["frames"], ref["frames"]) and len(got["frames"]) == 64
    assert got["X"].shape == (64, n) and got["B"].shape == (sph.nvert, n) and got["Y"].shape == (sph.nvert, n)
    for k in ("R", "X", "B", "Y"):
        assert _near(got[k], ref[k]), k
    # the scaling of the constraint rows: Y lambda R_0 nshell / nreg
    assert np.allclose(got["B"], got["Y"] * (0.7 * ref["R"][0] * 64 / sph.nvert), rtol=1e-6, atol=0)


def test_basis_is_orthonormal_and_has_the_stated_phase():
    # a 5810-point Gauss product rule is exact for these products: Y'WY = I
    t, w = np.polynomial.legendre.leggauss(20)
    phi = (np.arange(40) + 0.5) * (2 * np.pi / 40)
    T, P = np.meshgrid(t, phi, indexing="ij")
    st = np.sqrt(1 - T ** 2)
    d = np.stack([st * np.cos(P), st * np.sin(P), T], -1).reshape(-1, 3)
    W = np.repeat(w, 40) * (2 * np.pi / 40)
    Y = csd_ref.sh_basis(d, 8)
    assert np.allclose(Y.T @ (Y * W[:, None]), np.eye(45), atol=1e-12)
    # Y_00 = 1 / sqrt(4 pi); Y_2,1 at (theta, phi) = (pi / 4, 0) carries the Condon-Shortley sign: -sqrt(15 / (4 pi)) sin cos
    v = csd_ref.sh_basis([[np.sin(np.pi / 4), 0.0, np.cos(np.pi / 4)]], 2)[0]
    assert np.isclose(v[0], 1 / np.sqrt(4 * np.pi))
    assert np.isclose(v[2 * 3 // 2 + 1], -np.sqrt(15 / (4 * np.pi)) * 0.5)


def test_frame_selection(fj):
    g = phantom.sphere_dirs(30, 2)
    # b0s interleaved, two shells, one frame just inside and one just outside the tolerance of the outer shell
    bval = np.array([0, 1000] * 10 + [5, 3000] * 10 + [2860.0, 3140.0, 2840.0, 50.0] + [3000.0] * 6, np.float32)
    bvec = np.resize(g, (len(bval), 3)).astype(np.float32)
    bvec[bval <= 50] = 0
    got = fj.csd_design(bval, bvec, RESP, fj.sphere_362, lmax=2)
    want = np.nonzero((bval > 50) & (np.abs(bval - 3140.0) <= 0.05 * 3140.0))[0]
    assert np.array_equal(got["frames"], want)                     # the default shell is the largest b
    got = fj.csd_design(bval, bvec, RESP, fj.sphere_362, lmax=2, shell=3000.0)
    want = np.nonzero(np.abs(bval - 3000.0) <= 150.0)[0]
    assert np.array_equal(got["frames"], want) and 2860.0 in bval[want] and 2840.0 not in bval[want]
    got = fj.csd_design(bval, bvec, RESP, fj.sphere_362, lmax=2, shell=1000.0)
    assert np.array_equal(got["frames"], np.nonzero(bval == 1000)[0])
    assert np.array_equal(got["frames"], csd_ref.shell_frames(bval, shell=1000.0))
    # a shell below b0_thresh has no frames: those are b0 frames
    with pytest.raises(fj.FibersError) as e:
        fj.csd_design(bval, bvec, RESP, fj.sphere_362, lmax=2, shell=50.0, b_tol=1.0, b0_thresh=3000.0)
    assert e.value.code == -1


def test_too_few_frames_and_rank_are_refused(fj):
    for lmax in (2, 4, 6, 8):
        n = csd_ref.ncoef(lmax)
        bval, bvec = _scheme(ndir=n - 1, lmax=lmax)
        with pytest.raises(fj.FibersError) as e:
            fj.csd_design(bval, bvec, RESP, fj.sphere_362, lmax=lmax)
        assert e.value.code == -1 and "at least %d frames" % n in e.value.message
        bval, bvec = _scheme(ndir=n, lmax=lmax)
        assert fj.csd_design(bval, bvec, RESP, fj.sphere_362, lmax=lmax)["rank"] == n
    # 30 frames, but only 5 distinct directions: lmax 4 needs 15
    bval, bvec = _scheme(ndir=30)
    bvec[4:] = np.resize(bvec[4:9], (30, 3))
    with pytest.raises(fj.FibersError) as e:
        fj.csd_design(bval, bvec, RESP, fj.sphere_362, lmax=4)
    assert e.value.code == -1 and "rank" in e.value.message
    with pytest.raises(fj.FibersError):
        fj.csd_design(bval, bvec, RESP, fj.sphere_362, lmax=5)
    with pytest.raises(fj.FibersError):
        fj.csd_design(bval, bvec, (0.3e-3, 1.7e-3, 1000.0), fj.sphere_362, lmax=4)     # an oblate "response"


def test_missing_tables_are_the_reference_errors(fj):
    import ctypes as C
    from fibers_jl_amd import _lib
    p = _lib.CsdParams(8, 1.7e-3, 0.3e-3, 1000.0, 50.0, 0.0, 0.05, 1.0, 0.1, 50)
    v = np.asfortranarray(fj.sphere_362.vertices, dtype=np.float32)
    bval, bvec = _scheme()
    L = fj.lib()
    assert L.fib_csd_design(None, None, 0, v.ctypes.data, v.shape[0], C.byref(p), None, None, None, None, None, None, None) == -4
    assert L.fib_csd_design(bval.ctypes.data, None, len(bval), v.ctypes.data, v.shape[0], C.byref(p), None, None, None, None, None, None, None) == -5
    assert L.fib_csd_design(bval.ctypes.data, np.asfortranarray(bvec).ctypes.data, len(bval), v.ctypes.data, v.shape[0], None, None, None, None,
                            None, None, None, None) == -1


# ---- known answers of the restatement on the library's tables -------------------------------------------------------------------
@pytest.fixture(scope="module")
def tables(fj):
    bval, bvec = _scheme()
    return bval, bvec, fj.csd_design(bval, bvec, RESP, fj.sphere_724, lmax=8)


def test_single_fibre_along_a_vertex_peaks_there(fj, tables):
    """peak 1 of a noise-free fibre along a vertex is that vertex, and sh[0] R_0 Y_00 -- the l = 0 term of the convolution -- is the mean
    signal over the sphere, s0 int exp(-b (lperp + (lpar - lperp) t^2)) dt / 2 = R_0 / (4 pi) (64 random directions sample it to a few per
    cent only, so the integral is the yardstick).  What a fit up to lmax cannot hold of a delta's signal, the orders above lmax, is at
    most sum_{l > 8} |R_l| (2l + 1) / R_0 = 2.7 % of that mean, and that is the bound, with the constraint rows weighted down (lambda =
    0.01) so that the data decide sh[0] (the restatement is within 0.3 %).  At lambda = 1 suppressing the side lobes costs the fit a
    few per cent more of sh[0], by an amount the definition does not bound: only the peak is asserted there."""
    bval, bvec, t = tables
    t01 = fj.csd_design(bval, bvec, RESP, fj.sphere_724, lmax=8, lam=0.01)
    V = fj.sphere_724.vertices
    for vtx in (0, 17, 200, 361):
        s = csd_ref.signal(bval, bvec, t["frames"], [V[vtx]], [1.0], *RESP).astype(np.float32)[None]
        t_ = np.polynomial.legendre.leggauss(64)
        mean = 0.5 * RESP[2] * np.sum(t_[1] * np.exp(-3000.0 * (RESP[1] + (RESP[0] - RESP[1]) * t_[0] ** 2)))
        assert np.isclose(mean, t["R"][0] / (4 * np.pi), rtol=1e-6)
        Rhi = csd_ref.response_R(3000.0, *[float(np.float32(v)) for v in RESP], 20)
        rtol = sum(abs(Rhi[l // 2]) * (2 * l + 1) for l in range(10, 21, 2)) / Rhi[0]
        assert 0.02 < rtol < 0.03
        for tab in (t, t01):
            r = csd_ref.rec(s, tab["X"], tab["B"], tab["Y"])
            pk, amp, top, nval = csd_ref.peaks(r["odf"], V, fj.sphere_724.faces)
            assert top[0, 0] == vtx and nval[0] >= 1 and 1 <= r["niter"][0] < 50
            assert np.allclose(pk[0, 0], V[vtx]) and amp[0, 0] == np.float32(r["odf"][0, vtx])
            if tab is t01:
                assert np.isclose(r["sh"][0, 0] * tab["R"][0] / np.sqrt(4 * np.pi), mean, rtol=rtol)


def test_two_fibres_at_right_angles_are_both_found(fj, tables):
    bval, bvec, t = tables
    V = fj.sphere_724.vertices
    a = 40
    b = int(np.argmin(np.abs(V[:362] @ V[a])))                      # the vertex closest to perpendicular
    s = csd_ref.signal(bval, bvec, t["frames"], [V[a], V[b]], [0.5, 0.5], *RESP).astype(np.float32)[None]
    r = csd_ref.rec(s, t["X"], t["B"], t["Y"])
    pk, amp, top, nval = csd_ref.peaks(r["odf"], V, fj.sphere_724.faces)
    assert nval[0] >= 2 and set(top[0, :2]) == {a, b}
    assert amp[0, 1] > 0.5 * amp[0, 0]


def test_restatement_orders_and_types(fj, tables):
    """the two summation orders of the float64 restatement agree to rounding, and its float32 form takes the same number of solves on
    these well-separated voxels; a voxel without a positive sample is skipped"""
    bval, bvec, t = tables
    V = fj.sphere_724.vertices
    rng = np.random.default_rng(1)
    s = np.stack([csd_ref.signal(bval, bvec, t["frames"], [V[i], V[j]], [0.6, 0.4], *RESP) for i, j in ((3, 150), (90, 300))])
    s = (s + rng.normal(0, 20.0, s.shape)).astype(np.float32)
    s = np.concatenate([s, -np.abs(s[:1])])
    r = csd_ref.rec(s, t["X"], t["B"], t["Y"])
    rp = csd_ref.rec(s, t["X"], t["B"], t["Y"], perm=rng.permutation(len(t["frames"])))
    assert np.array_equal(r["niter"], rp["niter"]) and r["niter"][2] == 0 and not r["odf"][2].any() and not r["sh"][2].any()
    assert np.abs(r["odf"] - rp["odf"]).max() <= 1e-12 * np.abs(r["odf"]).max()
    assert r["margin"][:2].min() > 1e-9 and np.isinf(r["margin"][2])
    r1 = csd_ref.rec(s, t["X"], t["B"], t["Y"], niter=1)
    assert list(r1["niter"]) == [1, 1, 0]


def test_restatement_reports_the_set_sizes(fj, tables):
    """setmin / setmax of `rec`: with a threshold above every amplitude the set is all nreg directions on every pass, with one below
    every amplitude it is empty (thr = tau B[0,0] f0[0] and f0[0] > 0; the second pass repeats the set, so one solve); a skipped voxel
    reports -1; the permuted order reports the same sizes; a single fibre at tau = 0.1 leaves most directions, not all, under the
    threshold (a sparse fODF); and the sizes bracket the first pass's and the last pass's own counts"""
    bval, bvec, t = tables
    V = fj.sphere_724.vertices
    nreg = t["B"].shape[0]
    s = np.stack([csd_ref.signal(bval, bvec, t["frames"], [V[i]], [1.0], *RESP) for i in (3, 90)]).astype(np.float32)
    s = np.concatenate([s, -np.abs(s[:1])])
    r = csd_ref.rec(s, t["X"], t["B"], t["Y"], tau=1e6)
    assert list(r["setmin"]) == [nreg, nreg, -1] and list(r["setmax"]) == [nreg, nreg, -1] and list(r["niter"]) == [1, 1, 0]
    r = csd_ref.rec(s, t["X"], t["B"], t["Y"], tau=-1e6)
    assert list(r["setmin"]) == [0, 0, -1] and list(r["setmax"]) == [0, 0, -1] and list(r["niter"]) == [1, 1, 0]
    r = csd_ref.rec(s, t["X"], t["B"], t["Y"])
    rp = csd_ref.rec(s, t["X"], t["B"], t["Y"], perm=np.random.default_rng(4).permutation(len(t["frames"])))
    assert np.array_equal(r["setmin"], rp["setmin"]) and np.array_equal(r["setmax"], rp["setmax"])
    assert np.all(r["setmin"] <= r["setmax"]) and np.all(2 * r["setmax"][:2] > nreg) and np.all(r["setmax"][:2] < nreg)
    one = csd_ref.rec(s, t["X"], t["B"], t["Y"], niter=1)                 # the first pass alone
    assert np.array_equal(one["setmin"], one["setmax"]) and np.all(r["setmin"][:2] <= one["setmin"][:2]) and np.all(one["setmax"][:2] <= r["setmax"][:2])
    # the count is that of the set the odf shows: after the last pass, the directions below thr are those the constraint holds down
    a = t["B"].astype(np.float64) @ r["sh"][0]
    thr = np.float64(np.float32(0.1)) * np.float64(t["B"][0, 0]) * np.linalg.lstsq(t["X"][:, :15].astype(np.float64), s[0].astype(np.float64), rcond=None)[0][0]
    assert r["setmin"][0] <= int((a < thr).sum()) <= r["setmax"][0]


def test_response_from_a_tensor_fit(fj):
    shape = (4, 3, 2)
    mk = lambda v: fj.MRI(np.full(shape + (1,), v, np.float32))    # noqa: E731
    fa = mk(0.8)
    fa.vol[0, 0, 0, 0] = 0.5
    l1 = mk(1.7e-3)
    l1.vol[0, 0, 0, 0] = 9.0                                        # excluded by fa
    l1.vol[1, 0, 0, 0] = 9.0                                        # excluded by the mask
    mask = np.ones(shape, np.uint8)
    mask[1, 0, 0] = 0

    class D:
        pass
    d = D()
    d.fa, d.eigval1, d.eigval2, d.eigval3, d.s0 = fa, l1, mk(0.4e-3), mk(0.2e-3), mk(900.0)
    lpar, lperp, s0 = fj.csd_response(d, mask)
    assert np.isclose(lpar, np.float32(1.7e-3)) and np.isclose(lperp, 0.3e-3, rtol=1e-6) and s0 == 900.0
    with pytest.raises(ValueError):
        fj.csd_response(d, mask, fa_thresh=0.9)


def test_top_level_exports(fj):
    for name in ("CSD", "CsdPlan", "csd_design", "csd_response", "csd_rec", "csd_write"):
        assert hasattr(fj, name), name
    assert not hasattr(fj, "csd_rec_device") and hasattr(fj.csd, "csd_rec_device")
