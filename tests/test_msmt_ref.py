"""Multi-shell multi-tissue deconvolution without a GPU: fib_msmt_design and fib_msmt_wm_response against the float64 restatement
(tests/msmt_ref.py), the edges of the shell walk, the refusals, the tie of the restatement to csd_ref, and the restatement's own known
answers (what the GPU tests then hold the kernel to)."""
import numpy as np
import pytest

import csd_ref
import msmt_ref

TENSOR = (1.7e-3, 0.3e-3, 1000.0)
# |iso[1] - 1| and |sh[0] sqrt(4 pi)| in a noise-free pure-CSF voxel: 1.1e-14 is the largest the restatement gave here over lmax 4, 6, 8
# (at lmax 4; the float32 samples of a pure-CSF voxel are the response table's own entries, so only the float64 solves err)
# (DESIGN.md §5 records it); the bound is twice that
CSF_MEASURED, CSF_BOUND = 1.1e-14, 2.2e-14


def _near(got, want64):
    """test_csd_ref's rule: got equals the float32 rounding of want64 or that value's float32 neighbour, or differs from want64 by less
    than the restatement's own float64 evaluation error, 8 eps64 max|table| absolute (entries that are zero in exact arithmetic)"""
    want64 = np.asarray(want64, np.float64)
    w = want64.astype(np.float32)
    got = np.asarray(got, np.float32)
    lo, hi = np.nextafter(w, np.float32(-np.inf)), np.nextafter(w, np.float32(np.inf))
    tiny = 8 * np.finfo(np.float64).eps * np.abs(want64).max()
    return bool(np.all((got == w) | (got == lo) | (got == hi) | (np.abs(got.astype(np.float64) - want64) <= tiny)))


def _response(fj, bval, lmax, niso=2):
    shell, bbar = msmt_ref.shells(bval)
    wm_R, iso_r = msmt_ref.model_responses(bbar, lmax, niso=niso)
    return shell, bbar, fj.MsmtResponse(bbar, wm_R, iso_r)


@pytest.mark.parametrize("lmax,niso", [(8, 2), (8, 1), (8, 0), (6, 2), (4, 1), (2, 2)])
@pytest.mark.parametrize("sphere", ["sphere_362", "sphere_724"])
def test_design_tables_match_the_restatement(fj, lmax, niso, sphere):
    sph = getattr(fj, sphere)
    bval, bvec = msmt_ref.scheme(nb0=5, ndirs=(20, 30, 40), bs=(1000.0, 2000.0, 3000.0))
    bval[7], bval[30] = 1040.0, 1960.0                                  # shells are ranges, bbar a mean
    bvec[2] = (0.0, 0.6, 0.8)                                           # a shell-0 frame's direction is not read
    shell, bbar, resp = _response(fj, bval, lmax, niso)
    got = fj.msmt_design(bval, bvec, resp, sph, lmax=lmax, lam=0.7, lam_iso=1.3)
    ref = msmt_ref.design(bval, bvec, sph.vertices, resp.wm_R, resp.iso_r, lmax=lmax, lam=0.7, lam_iso=1.3)
    n, nreg = csd_ref.ncoef(lmax) + niso, sph.nvert
    assert got["rank"] == n
    assert np.array_equal(got["shell"], ref["shell"]) and np.array_equal(np.bincount(got["shell"]), [5, 20, 30, 40])
    assert np.allclose(got["bbar"], ref["bbar"], rtol=1e-14, atol=0) and got["bbar"][1] == (19 * 1000.0 + 1040.0) / 20
    assert got["X"].shape == (95, n) and got["B"].shape == (nreg + niso, n) and got["Y"].shape == (nreg, n)
    for k in ("X", "B", "Y"):
        assert _near(got[k], ref[k]), k
    # a shell-0 row is [Y_00 R_0(0), 0, ..] and the isotropic columns; the isotropic constraint rows are unit vectors
    nwm = n - niso
    assert np.all(got["X"][:5, 1:nwm] == 0) and np.all(got["X"][:5, 0] == np.float32(np.sqrt(1 / (4 * np.pi)) * float(resp.wm_R[0, 0])))
    assert not got["Y"][:, nwm:].any() and not got["B"][:nreg, nwm:].any() and not got["B"][nreg:, :nwm].any()
    for t in range(niso):
        row = got["B"][nreg + t]
        assert np.count_nonzero(row) == 1 and np.isclose(row[nwm + t], 1.3 * resp.iso_r[t][shell].astype(np.float64).sum(), rtol=1e-6)
    sum_r0 = resp.wm_R[shell, 0].astype(np.float64).sum()
    assert np.allclose(got["B"][:nreg, :nwm], got["Y"][:, :nwm] * (0.7 * sum_r0 / nreg), rtol=1e-6, atol=0)


@pytest.mark.parametrize("lmax", [2, 8])
def test_wm_response_matches_the_restatement_and_csd_design(fj, lmax):
    bbar = np.array([4.0, 1010.5, 2000.0, 2995.0])
    got = fj.msmt_wm_response(*TENSOR, bbar, lmax)
    want = msmt_ref.wm_response(*TENSOR, bbar, lmax)
    # (R_8 at b = 4 is 6e-10 beside R_0 = 1.25e4: the quadrature cancels there, and `_near`'s absolute allowance is what binds)
    assert got.shape == (4, lmax // 2 + 1) and _near(got, want) and np.array_equal(got[:, :2], want[:, :2].astype(np.float32))
    # the code is csd_rec's: the one-shell design reports the same R
    bval, bvec = csd_ref.scheme(64, lmax)
    R = fj.csd_design(bval, bvec, TENSOR, fj.sphere_362, lmax=lmax)["R"]
    assert np.array_equal(fj.msmt_wm_response(*TENSOR, [3000.0], lmax)[0], R)


def test_shell_walk_edges(fj):
    def walk(b, **kw):
        sh, bbar = fj.msmt_shells(np.asarray(b, np.float32), **kw)
        rs, rb = msmt_ref.shells(b, **kw)
        assert np.array_equal(sh, rs) and np.allclose(bbar, rb, rtol=1e-14, atol=0)
        return list(sh), list(bbar)
    # 1100 is exactly (1 + 2 * 0.05) * 1000: one shell; 1101 opens the next
    assert walk([0, 1000, 1100, 1000]) == ([0, 1, 1, 1], [0.0, 3100.0 / 3])
    assert walk([0, 1000, 1101, 1000]) == ([0, 1, 2, 1], [0.0, 1000.0, 1101.0])
    # the walk is in ascending b with ties in frame order, whatever the frame order; the limit is relative to the shell's smallest b
    assert walk([3000, 5, 1050, 2000, 1000, 0, 1090, 50]) == ([3, 0, 1, 2, 1, 0, 1, 0], [55.0 / 3, 3140.0 / 3, 2000.0, 3000.0])
    assert walk([1000, 1090, 1190])[0] == [1, 1, 2]
    # an empty shell 0: it still counts, with bbar 0
    assert walk([1000, 2000, 1000]) == ([1, 2, 1], [0.0, 1000.0, 2000.0])
    assert walk([40, 60, 1000], b0_thresh=30.0)[0] == [1, 2, 3] and walk([40, 60, 1000], b0_thresh=60.0)[0] == [0, 0, 1]
    assert walk([0, 1000, 1250, 1300], b_tol=0.15)[0] == [0, 1, 1, 1]
    # eight shells above b0 are the most
    assert walk([0] + [500.0 * k for k in range(1, 9)])[0] == list(range(9))
    with pytest.raises(fj.FibersError) as e:
        fj.msmt_shells(np.array([0] + [500.0 * k for k in range(1, 10)], np.float32))
    assert e.value.code == -7 and "9 shells" in str(e.value)


def test_zero_gradient_rows_and_frame_count(fj):
    bval, bvec = msmt_ref.scheme(nb0=4, ndirs=(20, 20, 20))
    _, _, resp = _response(fj, bval, 4)
    bad = bvec.copy()
    bad[30] = 0.0
    with pytest.raises(fj.FibersError) as e:
        fj.msmt_design(bval, bad, resp, fj.sphere_362, lmax=4)
    assert e.value.code == -1 and "frame 30" in str(e.value)
    ok = bvec.copy()
    ok[:4] = 0.0                                                        # zero rows in shell 0 are what b0 frames have
    assert fj.msmt_design(bval, ok, resp, fj.sphere_362, lmax=4)["rank"] == 17
    # 512 frames are accepted, 513 refused
    for nd, code in ((169, 0), (170, -7)):
        bval, bvec = msmt_ref.scheme(nb0=5, ndirs=(169, 169, nd))
        _, _, resp = _response(fj, bval, 2)
        if code:
            with pytest.raises(fj.FibersError) as e:
                fj.msmt_design(bval, bvec, resp, fj.sphere_362, lmax=2)
            assert e.value.code == code and "513" in str(e.value) and "512" in str(e.value)
        else:
            assert len(bval) == 512 and fj.msmt_design(bval, bvec, resp, fj.sphere_362, lmax=2)["rank"] == 8
    # fewer frames than unknowns, and a response table for another number of shells
    bval, bvec = msmt_ref.scheme(nb0=2, ndirs=(5, 5, 4))
    _, _, resp = _response(fj, bval, 4)
    with pytest.raises(fj.FibersError, match="at least 17 frames") as e:
        fj.msmt_design(bval, bvec, resp, fj.sphere_362, lmax=4)
    assert e.value.code == -1
    bval, bvec = msmt_ref.scheme(nb0=4, ndirs=(20, 20, 20))
    with pytest.raises(fj.FibersError, match="given for 3 shells, the series has 4") as e:
        fj.msmt_design(bval, bvec, fj.MsmtResponse(resp.shells[:3], resp.wm_R[:3], resp.iso_r[:, :3]), fj.sphere_362, lmax=4)
    assert e.value.code == -1


def test_two_isotropic_tissues_need_three_shells(fj):
    """the WM l = 0 column and the two isotropic columns are constant within a shell: three such columns need three distinct shells"""
    for nb0, ndirs, bs, ok in ((6, (50,), (1000.0,), False), (0, (30, 30), (1000.0, 2000.0), False),
                               (6, (30, 30), (1000.0, 2000.0), True), (0, (20, 20, 20), (1000.0, 2000.0, 3000.0), True)):
        bval, bvec = msmt_ref.scheme(nb0=nb0, ndirs=ndirs, bs=bs)
        _, _, resp = _response(fj, bval, 4)
        if ok:
            assert fj.msmt_design(bval, bvec, resp, fj.sphere_362, lmax=4)["rank"] == 17
        else:
            with pytest.raises(fj.FibersError, match="rank 16") as e:
                fj.msmt_design(bval, bvec, resp, fj.sphere_362, lmax=4)
            assert e.value.code == -1
            one = fj.MsmtResponse(resp.shells, resp.wm_R, resp.iso_r[:1])
            assert fj.msmt_design(bval, bvec, one, fj.sphere_362, lmax=4)["rank"] == 16      # one isotropic tissue is determined


@pytest.mark.parametrize("lmax,ndir", [(8, 64), (6, 47), (4, 16)])
def test_the_restatement_reduces_to_csd_ref(fj, lmax, ndir):
    """niso = 0, no b0 frame, one shell, tau = 0.1: csd_ref.rec's niter exactly and its sh within 1e-12 max|sh| -- on the same tables and,
    with the response evaluated at the shell, on msmt_ref's own tables too"""
    bval, bvec = csd_ref.scheme(ndir, lmax, nb0=0)
    sph = fj.sphere_362
    tc = csd_ref.rounded(csd_ref.design(bval, bvec, sph.vertices, TENSOR, lmax=lmax))
    shell, bbar = msmt_ref.shells(bval)
    assert list(bbar) == [0.0, 3000.0] and np.all(shell == 1)
    wm_R = msmt_ref.wm_response(*TENSOR, bbar, lmax)
    tm = msmt_ref.design(bval, bvec, sph.vertices, wm_R.astype(np.float32), [], lmax=lmax)
    # the float64 tables agree up to the float32 rounding of the response table
    for k in ("X", "B", "Y"):
        assert np.allclose(tm[k], csd_ref.design(bval, bvec, sph.vertices, TENSOR, lmax=lmax)[k], rtol=1e-6, atol=1e-9 * np.abs(tm[k]).max()), k
    rng = np.random.default_rng(lmax)
    s = np.stack([csd_ref.signal(bval, bvec, np.arange(ndir), rng.normal(size=(1 + i % 3, 3)), np.full(1 + i % 3, 1.0 / (1 + i % 3)), *TENSOR)
                  + rng.normal(0, 1000.0 / 30, ndir) for i in range(9)]).astype(np.float32)
    want = csd_ref.rec(s, tc["X"], tc["B"], tc["Y"], tau=0.1)
    got = msmt_ref.rec(s, tc["X"], tc["B"], tc["Y"], csd_ref.ncoef(lmax), tau=0.1)
    assert want["niter"].min() >= 1 and np.array_equal(got["niter"], want["niter"])
    assert np.abs(got["sh"] - want["sh"]).max() <= 1e-12 * np.abs(want["sh"]).max()
    assert np.array_equal(got["setmin"], want["setmin"]) and np.array_equal(got["setmax"], want["setmax"]) and got["iso"].shape == (9, 0)


@pytest.mark.parametrize("lmax", [4, 6, 8])
def test_known_answers_on_noise_free_mixtures(fj, lmax):
    """signals mixed from the model's own responses: a single fibre peaks at the vertex nearest its axis; pure CSF gives iso[1] = 1 and no
    white matter within CSF_BOUND.  GM fractions are NOT asserted tightly: the WM l = 0 column and GM are nearly collinear."""
    sph = fj.sphere_724
    bval, bvec = msmt_ref.scheme(nb0=6, ndirs=(30, 30, 30))
    shell, bbar, resp = _response(fj, bval, lmax)
    t = msmt_ref.rounded(msmt_ref.design(bval, bvec, sph.vertices, resp.wm_R, resp.iso_r, lmax=lmax))
    nwm = csd_ref.ncoef(lmax)
    V = np.asarray(sph.vertices, np.float64)[:sph.nvert]
    axes = [V[17], V[200], np.array([0.3, -0.5, 0.81])]
    s = [msmt_ref.mixture(bvec, shell, bbar, resp.wm_R, resp.iso_r, [u], [1.0]) for u in axes]
    s.append(msmt_ref.mixture(bvec, shell, bbar, resp.wm_R, resp.iso_r, [], [], iso_w=(0.0, 1.0)))
    s.append(msmt_ref.mixture(bvec, shell, bbar, resp.wm_R, resp.iso_r, [], [], iso_w=(1.0, 0.0)))
    s.append(msmt_ref.mixture(bvec, shell, bbar, resp.wm_R, resp.iso_r, [axes[0]], [0.5], iso_w=(0.3, 0.2)))
    r = msmt_ref.rec(np.asarray(s, np.float32), t["X"], t["B"], t["Y"], nwm)
    pk, amp, top, nval = csd_ref.peaks(r["odf"], np.asarray(sph.vertices, np.float32), sph.faces)
    for v, u in enumerate(axes):
        u = u / np.linalg.norm(u)
        assert nval[v] >= 1 and top[v, 0] == int(np.argmax(np.abs(V @ u))), (lmax, v)
        assert abs(r["iso"][v]).max() < 0.05                                     # no isotropic tissue to speak of
    # pure CSF: iso[1] = 1 and no white matter, within CSF_BOUND
    e1, e0 = abs(r["iso"][3, 1] - 1), abs(r["sh"][3, 0]) * np.sqrt(4 * np.pi)
    print("lmax %d: pure CSF: |iso[1] - 1| = %.3g, |sh[0] sqrt(4 pi)| = %.3g, iso[0] = %.3g, niter %d (bound %.3g)"
          % (lmax, e1, e0, r["iso"][3, 0], r["niter"][3], CSF_BOUND))
    assert e1 <= CSF_BOUND and e0 <= CSF_BOUND
    # pure GM and the mixture: only loosely (the trade-off with the WM l = 0 column)
    assert abs(r["iso"][4, 0] - 1) < 0.3 and abs(r["iso"][4, 1]) < 0.1
    assert abs(r["iso"][5].sum() + r["sh"][5, 0] * np.sqrt(4 * np.pi) - 1.0) < 0.1
    assert top[5, 0] == top[0, 0]


def test_skipped_voxels_and_the_reported_figures(fj):
    sph = fj.sphere_362
    bval, bvec = msmt_ref.scheme(nb0=4, ndirs=(20, 20, 20))
    shell, bbar, resp = _response(fj, bval, 4)
    t = msmt_ref.rounded(msmt_ref.design(bval, bvec, sph.vertices, resp.wm_R, resp.iso_r, lmax=4))
    rng = np.random.default_rng(1)
    s = np.stack([msmt_ref.mixture(bvec, shell, bbar, resp.wm_R, resp.iso_r, [rng.normal(size=3)], [0.6], iso_w=(0.2, 0.2)) + rng.normal(0, 30, 64)
                  for _ in range(4)]).astype(np.float32)
    s[2] = -np.abs(s[2])
    r = msmt_ref.rec(s, t["X"], t["B"], t["Y"], 15)
    rp = msmt_ref.rec(s, t["X"], t["B"], t["Y"], 15, perm=np.random.default_rng(2).permutation(64))
    assert r["niter"][2] == 0 and not r["odf"][2].any() and not r["sh"][2].any() and not r["iso"][2].any() and r["a"][2] is None
    assert r["gap"][2] == np.inf and r["setmin"][2] == -1
    keep = [0, 1, 3]
    assert np.array_equal(r["niter"], rp["niter"]) and r["niter"][keep].min() >= 1
    assert all(r["a"][v].shape == (r["niter"][v] + (r["niter"][v] < 50), sph.nvert + 2) for v in keep)
    assert np.all(r["setmin"][keep] <= r["setmax"][keep]) and np.all((r["iso_in"] | r["iso_out"])[keep])
    assert not msmt_ref.undecided(r, rp).any()
    one = msmt_ref.rec(s, t["X"], t["B"], t["Y"], 15, niter=1)
    assert np.array_equal(one["niter"], [1, 1, 0, 1])


def test_response_from_a_tensor_fit(fj):
    """msmt_response: WM is csd_response's tensor through msmt_wm_response at every shell; GM and CSF are per-shell means of the voxels
    selected by fa and md inside the mask; an empty class raises with its name; an empty shell 0 holds 0"""
    shape = (4, 3, 2)
    mk = lambda v: fj.MRI(np.full(shape + (1,), v, np.float32))    # noqa: E731
    # frames out of shell order: b0, 2000, 1000, 1040, b0, 2000
    bval = np.array([5.0, 2000.0, 1000.0, 1040.0, 0.0, 2000.0], np.float32)
    bvec = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [0, 0, 0], [0.6, 0.8, 0]], np.float32)
    fa, md = mk(0.8), mk(0.7e-3)                                    # white matter everywhere ..
    vol = np.full(shape + (6,), 100.0, np.float32, order="F")
    gm = [(0, 0, 0), (0, 1, 0), (0, 2, 1)]                          # .. but three GM voxels, one of them outside the mask ..
    csf = [(3, 0, 0), (3, 1, 1)]                                    # .. two CSF voxels ..
    for k, v in enumerate(gm):
        fa.vol[v], md.vol[v] = 0.1, (0.6e-3, 0.9e-3, 1.1e-3)[k]     # (the interval's ends belong to it)
        vol[v] = np.array([900, 200, 400, 380, 880, 220], np.float32) + 10 * k
    for k, v in enumerate(csf):
        fa.vol[v], md.vol[v] = 0.15, 2.5e-3 + k * 1e-3
        vol[v] = np.array([1500, 10, 80, 70, 1480, 14], np.float32) + 2 * k
    fa.vol[1, 1, 1], md.vol[1, 1, 1] = 0.1, 1.5e-3                  # .. a low-fa voxel between the two md classes: in neither
    fa.vol[2, 2, 0], md.vol[2, 2, 0] = 0.2, 0.9e-3                  # fa == iso_fa is not below it
    vol[1, 1, 1] = vol[2, 2, 0] = 7777.0
    fa.vol[1, 0, 0] = 0.5                                           # no white matter either
    mask = np.ones(shape, np.uint8)
    mask[0, 2, 1] = 0                                               # the third GM voxel
    mask[2, 0, 0] = 0

    class D:
        pass
    d = D()
    d.fa, d.md, d.eigval1, d.eigval2, d.eigval3, d.s0 = fa, md, mk(1.7e-3), mk(0.4e-3), mk(0.2e-3), mk(900.0)
    d.eigval1.vol[1, 0, 0, 0] = d.eigval1.vol[2, 0, 0, 0] = 9.0     # excluded by fa and by the mask
    dwi = fj.MRI(vol, bval, bvec)
    r = fj.msmt_response(dwi, d, fj.MRI(mask), lmax=4)
    assert isinstance(r, fj.MsmtResponse) and np.array_equal(r.shells, [2.5, 1020.0, 2000.0])
    tensor = fj.csd_response(d, mask)
    assert np.array_equal(r.wm_R, fj.msmt_wm_response(*tensor, r.shells, 4)) and r.wm_R.shape == (3, 3)
    # per-shell means over the two GM voxels inside the mask and the two CSF voxels: shell 0 = frames 0, 4; 1 = 2, 3; 2 = 1, 5
    g = np.array([[900, 200, 400, 380, 880, 220], [910, 210, 410, 390, 890, 230]], np.float64)
    c = np.array([[1500, 10, 80, 70, 1480, 14], [1502, 12, 82, 72, 1482, 16]], np.float64)
    want = np.array([[x[:, [0, 4]].mean(), x[:, [2, 3]].mean(), x[:, [1, 5]].mean()] for x in (g, c)])
    assert r.iso_r.dtype == np.float32 and r.iso_r.shape == (2, 3) and np.array_equal(r.iso_r, want.astype(np.float32))
    # the result is what msmt_design takes (on a series of the same three shells with enough directions)
    b2, g2 = msmt_ref.scheme(nb0=4, ndirs=(10, 10), bs=(1020.0, 2000.0))
    assert fj.msmt_design(b2, g2, r, fj.sphere_362, lmax=2)["rank"] == 8
    # an empty class names itself; so does missing white matter (csd_response's error)
    with pytest.raises(ValueError, match="GM response"):
        fj.msmt_response(dwi, d, fj.MRI(mask), gm_md=(1.2e-3, 1.4e-3))
    with pytest.raises(ValueError, match="CSF response"):
        fj.msmt_response(dwi, d, fj.MRI(mask), csf_md=4.0e-3)
    with pytest.raises(ValueError, match="GM response"):
        fj.msmt_response(dwi, d, fj.MRI(mask), iso_fa=0.05)
    with pytest.raises(ValueError, match="fa > 0.95"):
        fj.msmt_response(dwi, d, fj.MRI(mask), wm_fa=0.95)
    # without b <= b0_thresh frames shell 0 is empty: its isotropic entries are 0 and the WM row is the tensor's at b = 0
    keep = [1, 2, 3, 5]
    r0 = fj.msmt_response(fj.MRI(np.asfortranarray(vol[..., keep]), bval[keep], bvec[keep]), d, fj.MRI(mask), lmax=4)
    assert np.array_equal(r0.shells, [0.0, 1020.0, 2000.0]) and not r0.iso_r[:, 0].any() and np.array_equal(r0.iso_r[:, 1:], r.iso_r[:, 1:])
    assert np.array_equal(r0.wm_R[1:], r.wm_R[1:]) and np.isclose(r0.wm_R[0, 0], 4 * np.pi * 900.0, rtol=1e-6)


def test_top_level_exports(fj):
    for name in ("MSMT", "MsmtPlan", "MsmtResponse", "msmt_design", "msmt_rec", "msmt_response", "msmt_shells", "msmt_wm_response", "msmt_write"):
        assert hasattr(fj, name), name
    assert hasattr(fj.msmt, "msmt_rec_device")
