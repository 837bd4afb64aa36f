"""The NumPy restatement of dti_fit / adc_fit (tests/dti_ref.py) pinned on the CPU: analytic known answers, the branch table by
hand, the vectorised row-subset fit against an explicit per-voxel pinv, and the two float32 restatements that already exist
(oracle.dti_fit / adc_fit and oracle_np.dti_fit_voxel), whose deviation from float64 this file measures and prints."""
import numpy as np
import pytest

import dti_ref as R

from dti_ref import CLASSES, axis_scheme, coplanar_scheme, coplanar_signal

EPS32 = R.EPS32


def _scheme(ndir, nb0, b, seed):
    from fibers_jl_amd import phantom
    return phantom.scheme_dti(ndir, nb0, b, seed)


# ------------------------------------------------------------------------------------------------------------------------------
# known answers
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", sorted(CLASSES))
@pytest.mark.parametrize("ndir,nb0,b", [(6, 1, 1000.0), (12, 2, 700.0), (30, 3, 3000.0), (64, 4, 2000.0)])
def test_noise_free_tensors_are_recovered(cls, ndir, nb0, b):
    """s = S0 exp(-b g'Dg) of a prescribed tensor under a random rotation: eigenvalues, md, fa and s0 come back to 1e-10"""
    rng = np.random.default_rng(ndir)
    bval, bvec = _scheme(ndir, nb0, b, 3)
    ev = np.array(CLASSES[cls])
    n = 40
    d6 = R.random_tensors(ev, n, rng)
    s0 = rng.uniform(0.5, 1500.0, n)
    r = R.dti_fit_ref(R.tensor_signal(bval, bvec, d6, s0), np.ones(n), bval, bvec)
    assert (r["branch"] == R.FULL).all() and r["nsubset"] == 0
    for k, want in zip(("eigval1", "eigval2", "eigval3"), ev):
        np.testing.assert_allclose(r[k], want, rtol=1e-10)
    rd, md, fa = R.dti_maps(*ev)
    np.testing.assert_allclose(r["md"], md, rtol=1e-10)
    np.testing.assert_allclose(r["rd"], rd, rtol=1e-10)
    np.testing.assert_allclose(r["fa"], fa, rtol=1e-10, atol=1e-10)
    np.testing.assert_allclose(r["s0"], s0, rtol=1e-10)
    np.testing.assert_allclose(r["d"][:, :6], d6, rtol=0, atol=1e-10 * ev[0])
    for k in (1, 2, 3):                                                     # eigenvectors: unit, and D v = l v
        v = r["eigvec%d" % k]
        np.testing.assert_allclose(np.linalg.norm(v, axis=1), 1.0, rtol=1e-12)
        res = np.einsum("nij,nj->ni", r["D"], v) - r["eigval%d" % k][:, None] * v
        assert np.abs(res).max() <= 1e-12 * ev[0]


def test_signal_written_without_the_design_matrix_is_recovered():
    """s = S0 exp(-b g'Dg) written out from b, g and D in float64, not through design_dti: a wrong design matrix (a missing factor
    2, a swapped column) would not cancel.  g is the Float32 direction; b * g_i * g_j rounded to Float32 in the design matrix
    costs eps32 / 2 per entry, hence 1e-6"""
    rng = np.random.default_rng(5)
    bval, bvec = _scheme(30, 3, 1000.0, 5)
    ev = np.array(CLASSES["generic"])
    n = 40
    d6 = R.random_tensors(ev, n, rng)
    D = np.empty((n, 3, 3))
    for (i, j), k in zip(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)), range(6)):
        D[:, i, j] = D[:, j, i] = d6[:, k]
    g = np.asarray(bvec, np.float32).astype(np.float64)
    s0 = rng.uniform(0.5, 1500.0, n)
    s = s0[:, None] * np.exp(-np.asarray(bval, np.float64)[None] * np.einsum("fi,nij,fj->nf", g, D, g))
    r = R.dti_fit_ref(s, np.ones(n), bval, bvec)
    for k, want in zip(("eigval1", "eigval2", "eigval3"), ev):
        np.testing.assert_allclose(r[k], want, rtol=0, atol=1e-6 * ev[0])
    np.testing.assert_allclose(r["d"][:, :6], d6, rtol=0, atol=1e-6 * ev[0])
    np.testing.assert_allclose(r["s0"], s0, rtol=1e-6)


def test_adc_mono_exponential_two_shells():
    rng = np.random.default_rng(2)
    bval = np.concatenate([np.zeros(2), np.full(10, 1000.0), np.full(10, 2500.0)]).astype(np.float32)
    bval = bval[rng.permutation(bval.size)]
    adc, s0 = rng.uniform(0.2e-3, 3e-3, 50), rng.uniform(1e-3, 1e6, 50)
    s = s0[:, None] * np.exp(-bval.astype(np.float64)[None] * adc[:, None])
    r = R.adc_fit_ref(s, np.ones(50), bval)
    np.testing.assert_allclose(r["adc"], adc, rtol=1e-10)
    np.testing.assert_allclose(r["s0"], s0, rtol=1e-10)
    assert (r["branch"] == R.FULL).all()


def test_adc_constant_b_is_the_minimum_norm_solution():
    """one b-value: A = [-b 1] has rank 1; pinv gives d = (-b, 1) * mean(log s) / (b^2 + 1)"""
    bval = np.full(9, 1000.0, np.float32)
    s = np.random.default_rng(3).uniform(100.0, 900.0, (5, 9))
    r = R.adc_fit_ref(s, np.ones(5), bval)
    m = np.log(s).mean(1)
    np.testing.assert_allclose(r["d"], np.stack([-1000.0 * m, m], 1) / (1000.0 ** 2 + 1), rtol=1e-12)


def test_underdetermined_six_frames_minimum_norm():
    """nvol = 6: seven unknowns, pinv(A) log(s) is the solution of A d = log(s) of least norm (orthogonal to A's null space)"""
    bval, bvec = _scheme(6, 1, 1000.0, 1)
    bval, bvec = bval[:6], bvec[:6]                                          # b0 + five directions
    A = R.design_dti(bval, bvec).astype(np.float64)
    s = np.random.default_rng(4).uniform(200.0, 900.0, (8, 6))
    r = R.dti_fit_ref(s, np.ones(8), bval, bvec)
    assert (r["branch"] == R.FULL).all()
    np.testing.assert_allclose(r["d"] @ A.T, np.log(s), rtol=1e-11)
    null = np.linalg.svd(A)[2][6]
    assert np.abs(A @ null).max() < 1e-9 and np.abs(r["d"] @ null).max() <= 1e-12 * np.abs(r["d"]).max()
    np.testing.assert_allclose(r["d"], np.linalg.lstsq(A, np.log(s).T, rcond=None)[0].T, rtol=1e-9, atol=1e-15)


def test_axis_only_scheme_has_exactly_zero_off_diagonals():
    """+-x, +-y, +-z and a b0: rank 4, columns xy, xz, yz of A are zero -> those d are exactly 0 and the eigenvalues are the
    sorted diagonal, eigenvectors the axes"""
    bval, bvec = axis_scheme()
    assert np.linalg.matrix_rank(R.design_dti(bval, bvec)) == 4
    rng = np.random.default_rng(5)
    diag = rng.uniform(0.2e-3, 2.5e-3, (30, 3))
    s = 700.0 * np.exp(-1000.0 * np.concatenate([np.zeros((30, 1)), diag, diag], 1))
    r = R.dti_fit_ref(s, np.ones(30), bval, bvec)
    assert (r["d"][:, [1, 2, 4]] == 0).all()
    np.testing.assert_allclose(r["d"][:, [0, 3, 5]], diag, rtol=1e-11)
    np.testing.assert_allclose(np.stack([r["eigval3"], r["eigval2"], r["eigval1"]], 1), np.sort(diag, 1), rtol=1e-11)
    assert set(np.unique(np.abs(r["eigvec1"]))) == {0.0, 1.0}


# ------------------------------------------------------------------------------------------------------------------------------
# branch table
# ------------------------------------------------------------------------------------------------------------------------------
def _branch_case():
    bval, bvec = _scheme(12, 3, 1000.0, 2)                                   # frames 0-2: b0
    rng = np.random.default_rng(6)
    s = rng.uniform(100.0, 900.0, (16, 15)).astype(np.float32)
    return bval, bvec, s


def test_branch_table_by_hand():
    bval, bvec, s = _branch_case()
    tiny = np.float32(np.finfo(np.float32).tiny)
    s[1, 3:11] = 0                       # npos = 7 (3 b0 + 4): solves
    s[2, 3:12] = -1                      # npos = 6: zeros
    s[3, :3] = 0                         # every b0 non-positive: zeros
    s[4, :2] = -5                        # one of three b0 positive: solves
    s[5, 7] = np.nan                     # NaN is not > 0: subset
    s[6, 7] = -np.inf                    # nor is -Inf: subset
    s[7, 7] = np.inf                     # +Inf is: the full fit, nothing finite comes out
    s[8, 7] = np.float32(1e-42)          # a denormal counts as positive: full fit
    s[9, 7] = tiny                       # FLT_MIN
    s[10, 7] = np.nextafter(tiny, np.float32(0))
    s[11, 7] = np.finfo(np.float32).max
    s[12, :] = 0                         # nothing positive
    s[13, :] = np.nan
    mask = np.ones(16)
    mask[15] = 0
    with np.errstate(all="ignore"):
        r = R.dti_fit_ref(s, mask, bval, bvec)
        a = R.adc_fit_ref(s, mask, bval)
    want = [R.FULL, R.SUBSET, R.ZEROS, R.ZEROS, R.SUBSET, R.SUBSET, R.SUBSET, R.FULL, R.FULL, R.FULL, R.FULL, R.FULL, R.ZEROS,
            R.ZEROS, R.FULL, R.OUTSIDE]
    assert r["branch"].tolist() == want and a["branch"].tolist() == want
    assert r["nsubset"] == 4 and a["nsubset"] == 4
    for k in R.FIELDS + ("d", "D"):
        assert (r[k][[2, 3, 12, 13, 15]] == 0).all(), k
    assert (a["adc"][[2, 3, 12, 13, 15]] == 0).all() and (a["s0"][[2, 3, 12, 13, 15]] == 0).all()
    ok = R.comparable(r)
    assert ok.tolist() == [b in (R.FULL, R.SUBSET) and i != 7 for i, b in enumerate(want)]
    assert np.isnan(r["eigval1"][7]) and np.isnan(r["fa"][7]) and not np.isfinite(a["adc"][7])
    for i in (1, 4, 5, 6, 8, 9, 10, 11):
        assert np.isfinite(r["eigval1"][i]) and np.isfinite(r["s0"][i]) and r["s0"][i] > 0, i


def test_b0_is_the_minimum_b_value():
    """ib0 = (bval .== minimum(bval)) with a non-zero minimum: b = 5 frames are the b0 frames"""
    bval, bvec, s = _branch_case()
    bval = bval.copy()
    bval[:3] = 5.0
    bvec = bvec.copy()
    bvec[:3] = (1.0, 0.0, 0.0)
    s[0, :3] = 0                         # no b = 5 frame positive: zeros
    s[1, 1:4] = 0                        # frame 0 (b = 5) positive: solves
    s[2, 3:6] = 0                        # b = 5 frames all positive, three others not: solves
    r = R.dti_fit_ref(s[:3], np.ones(3), bval, bvec)
    assert r["branch"].tolist() == [R.ZEROS, R.SUBSET, R.SUBSET]


# ------------------------------------------------------------------------------------------------------------------------------
# the zero-row form of the subset fit
# ------------------------------------------------------------------------------------------------------------------------------
def test_subset_fit_equals_per_voxel_pinv():
    from fibers_jl_amd import phantom
    bval, bvec = _scheme(30, 3, 1000.0, 7)
    dwi, _, _ = phantom.make_volume((6, 5, 4), bval, bvec, 7, nonpositive_frac=0.3)
    s = dwi.reshape(-1, 33)
    r = R.dti_fit_ref(s, np.ones(len(s)), bval, bvec)
    a = R.adc_fit_ref(s, np.ones(len(s)), bval)
    A7, A2 = R.design_dti(bval, bvec).astype(np.float64), R.design_adc(bval).astype(np.float64)
    assert r["nsubset"] > 100
    for i in np.flatnonzero(r["branch"] == R.SUBSET):
        p = s[i] > 0
        l = np.log(s[i][p].astype(np.float64))
        np.testing.assert_allclose(r["d"][i], np.linalg.pinv(A7[p], rcond=EPS32 * 7) @ l, rtol=1e-9, atol=1e-15)
        np.testing.assert_allclose(a["d"][i], np.linalg.pinv(A2[p], rcond=EPS32 * 2) @ l, rtol=1e-9, atol=1e-15)


def test_subset_fit_of_rank_four():
    """29 positive rows (coplanar directions plus one b0) of rank 4: the cut-off drops three singular values in both forms"""
    bval, bvec = coplanar_scheme(ndir=28, nb0=4, extra=8)
    s = coplanar_signal(bval, bvec, 12, 8)
    A = R.design_dti(bval, bvec).astype(np.float64)
    p = s[0] > 0
    assert p.sum() == 29 and np.linalg.matrix_rank(A[p], tol=EPS32 * 7 * np.linalg.norm(A[p], 2)) == 4
    r = R.dti_fit_ref(s, np.ones(12), bval, bvec)
    assert (r["branch"] == R.SUBSET).all()
    for i in range(12):
        want = np.linalg.pinv(A[p], rcond=EPS32 * 7) @ np.log(s[i][p].astype(np.float64))
        np.testing.assert_allclose(r["d"][i], want, rtol=1e-9, atol=1e-11 * np.abs(want[:6]).max())
    assert np.abs(r["d"][:, [2, 4, 5]]).max() <= 1e-11 * np.abs(r["d"][:, :6]).max()   # xz, yz, zz: outside the row space


# ------------------------------------------------------------------------------------------------------------------------------
# the two float32 restatements
# ------------------------------------------------------------------------------------------------------------------------------
def _class_volume(cls, noise, seed, n=600, ndir=30, nb0=3, b=1000.0):
    rng = np.random.default_rng(seed)
    bval, bvec = _scheme(ndir, nb0, b, seed)
    s0 = rng.uniform(800.0, 1200.0, n)
    s = R.tensor_signal(bval, bvec, R.random_tensors(CLASSES[cls], n, rng), s0)
    if noise:
        s = np.maximum(s + rng.normal(scale=noise * 1000.0, size=s.shape), 1.0)
    shape = (n // 20, 5, 4)
    return np.asfortranarray(s.astype(np.float32).reshape(shape + (len(bval),))), (rng.random(shape) < 0.9).astype(np.uint8), bval, bvec


def _report(label, cm):
    print("\n  %-28s" % label + "  ".join("%s %.1e/%.1e" % (k, cm[k][0], cm[k][1]) for k in ("eigval1", "eigval2", "eigval3", "fa", "s0", "res1", "orth")))


@pytest.mark.parametrize("cls,noise", [("generic", 0.0), ("generic", 0.02), ("prolate", 0.0), ("prolate", 0.02), ("oblate", 0.0),
                                       ("oblate", 0.02), ("isotropic", 0.0), ("isotropic", 0.02)])
def test_oracle_matches_restatement_by_class(orc, cls, noise):
    """identical zero pattern and branch; the oracle's deviation from float64 is measured, printed (pytest -s) and held to four
    times the float32 figures of DESIGN.md §5: eigenvalues 1.6e-6 |eigval1| where the closed form is well conditioned and 1.7e-4
    where it is not (sqrt(eps32) * p through the acos), FA 4e-6, S0 1.5e-6, eigenvector residual 6e-6 |eigval1|"""
    dwi, mask, bval, bvec = _class_volume(cls, noise, 11)
    ref = R.dti_fit_ref(dwi, mask, bval, bvec)
    o = orc.dti_fit(dwi, mask, bval, bvec, nthreads=2)
    assert o["_npartial"] == ref["nsubset"] == 0
    for k in R.FIELDS:
        if k in ("s0", "eigval1", "md"):                                     # (FA and a vector component may be exactly 0 in a solved voxel)
            assert np.array_equal(np.asarray(o[k]) == 0, ref[k] == 0), k
        assert (np.asarray(o[k])[mask == 0] == 0).all() and (ref[k][mask == 0] == 0).all(), k
    ill = R.ill_conditioned(ref)
    cm = R.class_max(R.dti_errors(o, ref), ill)
    _report("%s noise %g (well/ill)" % (cls, noise), cm)
    for k in ("eigval1", "eigval2", "eigval3", "rd", "md"):
        assert cm[k][0] <= 4 * 1.6e-6 and cm[k][1] <= 4 * 1.7e-4, (k, cm[k])
    assert max(cm["fa"]) <= 4 * 4e-6 and max(cm["s0"]) <= 4 * 1.5e-6, (cm["fa"], cm["s0"])
    for k in (1, 2, 3):
        assert max(cm["res%d" % k]) <= 4 * 6e-6, (k, cm["res%d" % k])
    print("  orthogonality %.1e / %.1e  norm %.1e" % (cm["orth"] + (max(max(cm["norm%d" % k]) for k in (1, 2, 3)),)))
    if not (cls == "isotropic" and noise == 0.0):           # there the closed form's eigenvectors are neither orthogonal nor unit
        assert max(cm["orth"]) <= 4 * 2e-7 and max(max(cm["norm%d" % k]) for k in (1, 2, 3)) <= 4 * 2e-7, cm


@pytest.mark.parametrize("frac", [0.05, 0.3, 0.6])
def test_oracle_matches_restatement_on_the_partial_branch(orc, frac):
    """knock-outs: same zero pattern, same subset count, and the float32 SVD against the float64 pinv of the row subset"""
    from fibers_jl_amd import phantom
    bval, bvec = _scheme(30, 3, 1000.0, 12)
    shape = (10, 8, 6)
    dwi, _, _ = phantom.make_volume(shape, bval, bvec, 12, nonpositive_frac=frac)
    mask = (np.random.default_rng(13).random(shape) < 0.9).astype(np.uint8)
    ref = R.dti_fit_ref(dwi, mask, bval, bvec)
    o = orc.dti_fit(dwi, mask, bval, bvec, nthreads=2)
    assert o["_npartial"] == ref["nsubset"] and ref["nsubset"] > (10 if frac > 0.5 else 100)
    for k in ("s0", "eigval1", "md", "fa"):
        assert np.array_equal(np.asarray(o[k]) == 0, ref[k] == 0), k
    cm = R.class_max(R.dti_errors(o, ref), R.ill_conditioned(ref))
    _report("knock-out %g (well/ill)" % frac, cm)
    for k in ("eigval1", "eigval2", "eigval3"):                              # (float32 SVD against float64 pinv, up to 1.8e-5)
        assert cm[k][0] <= 4 * 1.8e-5 and cm[k][1] <= 4 * 1.7e-4, (k, cm[k])
    assert max(cm["fa"]) <= 4 * 4e-6 and max(cm["s0"]) <= 4 * 1.5e-6
    adc, s0 = orc.adc_fit(dwi, mask, bval, nthreads=2)
    aref = R.adc_fit_ref(dwi, mask, bval)
    assert aref["nsubset"] == ref["nsubset"] and np.array_equal(adc == 0, aref["adc"] == 0)
    ae = R.adc_errors(adc, s0, aref)
    print("  adc knock-out %g: adc %.1e (of %.1e)  s0 %.1e" % (frac, ae["adc"].max(), np.abs(aref["adc"]).max(), ae["s0"].max()))
    assert ae["adc"].max() <= 1e-5 * np.abs(aref["adc"]).max() and ae["s0"].max() <= 1e-5


def test_oracle_matches_restatement_on_a_rank_deficient_subset(orc):
    bval, bvec = coplanar_scheme()
    dwi = np.asfortranarray(coplanar_signal(bval, bvec, 60, 14).reshape(6, 5, 2, 40))
    mask = np.ones((6, 5, 2), np.uint8)
    ref = R.dti_fit_ref(dwi, mask, bval, bvec)
    o = orc.dti_fit(dwi, mask, bval, bvec, nthreads=1)
    assert o["_npartial"] == ref["nsubset"] == 60
    cm = R.class_max(R.dti_errors(o, ref), R.ill_conditioned(ref))
    _report("rank-4 subset (well/ill)", cm)
    for k in ("eigval1", "eigval2", "eigval3"):
        assert cm[k][0] <= 4 * 1.8e-5 and cm[k][1] <= 4 * 1.7e-4, (k, cm[k])
    # (the tensor has an exactly singular z row in float64 and a 1e-10 one in float32: the closed form's eigenvector of the zero
    #  eigenvalue is decided by that noise -- residuals of the order of |eigval1| are the oracle's own here; printed, not asserted)
    print("  residuals %.1e %.1e %.1e" % tuple(max(cm["res%d" % k]) for k in (1, 2, 3)))


def test_second_restatement_matches_voxel_by_voxel():
    """oracle_np.dti_fit_voxel (float32 pinv through LAPACK, eigh in place of the closed form): same branch in every voxel of
    the hand-made table, values at the float32 level"""
    from oracle import oracle_np
    bval, bvec, s = _branch_case()
    s[1, 3:11] = 0
    s[2, 3:12] = -1
    s[3, :3] = 0
    s[4, :2] = -5
    s[5, 7] = np.nan
    s[6, 7] = -np.inf
    s[8, 7] = np.float32(1e-42)
    s[12, :] = 0
    with np.errstate(all="ignore"):
        ref = R.dti_fit_ref(s, np.ones(16), bval, bvec)
    W = oracle_np.dti_work(bval, bvec)
    worst = 0.0
    for i in range(16):
        v = oracle_np.dti_fit_voxel(s[i], W)
        assert (v is None) == (ref["branch"][i] == R.ZEROS), i
        if v is None:
            continue
        lam = np.array([ref["eigval1"][i], ref["eigval2"][i], ref["eigval3"][i]])
        worst = max(worst, np.abs(v["eigval"] - lam).max() / abs(lam[0]), abs(v["s0"] - ref["s0"][i]) / ref["s0"][i], abs(v["fa"] - ref["fa"][i]))
    print("  oracle_np against ref64: worst deviation %.1e" % worst)
    assert worst <= 1e-4
