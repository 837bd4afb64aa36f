"""msmt_rec on the GPU against the float64 restatement (tests/msmt_ref.py) on the plan's own tables.

Pass rule, per case and per field (sh, iso, odf): |gpu - ref64| <= 4 d + 1e-6 max|ref64|, d = the largest deviation between the
restatement's two summation orders (the frames permuted) on that case, 1e-6 max = the allowance for the one float32 rounding of the
output.  niter must be equal on every compared voxel, skipped voxels all zero.  A voxel is undecided when gap < 64 e (gap = the smallest
|a_i - thr_i| over its passes and rows, e = the largest |a - a_perm| over its passes); the seeds here are chosen so that the restatement
reports none, and `reference` asserts that -- together with what the pool must exercise: every isotropic row both inside and outside the
set, and both sides of the kernel's complement switch (2 count > nreg).  A peak on a different vertex must be a tie in the float64 odf
within the odf tolerance."""
import numpy as np
import pytest

import csd_ref
import msmt_ref

pytestmark = pytest.mark.gpu

TENSOR = (1.7e-3, 0.3e-3, 1000.0)
W = 8            # voxels per workgroup (one wave each)


@pytest.fixture(scope="module")
def torch_():
    import torch
    return torch


def pool(bvec, shell, bbar, resp, nvox, seed, noise=1.0 / 30.0):
    """samples float32 [nvox, nvol]: 1, 2 and 3 fibres in turn with random axes and random WM / GM / CSF fractions, Gaussian noise
    s0 / 30; voxel 3 is pure WM, 4 pure GM, 5 pure CSF (all with noise), 6 has no positive sample, 7 is of mixed sign"""
    rng = np.random.default_rng(seed)
    nvol = len(shell)
    out = np.zeros((nvox, nvol))
    for i in range(nvox):
        nf = 1 + i % 3
        u = rng.normal(size=(nf, 3))
        w = rng.uniform(0.3, 1.0, nf)
        frac = rng.dirichlet((1.0, 1.0, 1.0))
        if i in (3, 4, 5):
            frac = np.eye(3)[i - 3]
        out[i] = msmt_ref.mixture(bvec, shell, bbar, resp.wm_R, resp.iso_r, u, frac[0] * w / w.sum(), iso_w=tuple(frac[1:][:resp.iso_r.shape[0]]))
        out[i] += rng.normal(0.0, 1000.0 * noise, nvol)
    if nvox > 6:
        out[6] = -np.abs(out[6])
        out[6, 0] = 0.0
    if nvox > 7:
        out[7, ::2] *= -1.0
    return out.astype(np.float32)


def make_case(fj, lmax=8, niso=2, nb0=6, ndirs=(20, 20, 20), sphere="sphere_724", nvox=24, seed=1, scheme_seed=5, **kw):
    sph = getattr(fj, sphere)
    bval, bvec = msmt_ref.scheme(nb0=nb0, ndirs=ndirs, seed=scheme_seed)
    shell, bbar = msmt_ref.shells(bval)
    wm_R, iso_r = msmt_ref.model_responses(bbar, lmax, niso=niso)
    resp = fj.MsmtResponse(bbar, wm_R, iso_r)
    s = pool(bvec, shell, bbar, resp, nvox, seed)
    mask = np.ones(nvox, np.uint8)
    if nvox > 8:
        mask[8] = 0
    return dict(lmax=lmax, niso=niso, sph=sph, bval=bval, bvec=bvec, resp=resp, s=s, mask=mask, kw=kw, nwm=csd_ref.ncoef(lmax),
                label="lmax %d niso %d, %d frames, %s, %s" % (lmax, niso, len(bval), sphere, kw))


def reference(fj, c, t=None):
    """the restatement's two orders on the case's tables (the plan's, or fib_msmt_design's: a test holds them equal) and what the pool
    must exercise; needs no GPU"""
    if t is None:
        t = fj.msmt_design(c["bval"], c["bvec"], c["resp"], c["sph"], lmax=c["lmax"], **{k: v for k, v in c["kw"].items() if k in ("lam", "lam_iso")})
    tau, niter = c["kw"].get("tau", 0.0), c["kw"].get("niter", 50)
    r = msmt_ref.rec(c["s"], t["X"], t["B"], t["Y"], c["nwm"], tau=tau, niter=niter)
    rp = msmt_ref.rec(c["s"], t["X"], t["B"], t["Y"], c["nwm"], tau=tau, niter=niter, perm=np.random.default_rng(7).permutation(c["s"].shape[1]))
    label = c["label"]
    solved = (c["mask"] != 0) & (c["s"] > 0).any(1)
    und = msmt_ref.undecided(r, rp) & solved
    ratio = min((r["gap"][v] / max(np.abs(r["a"][v] - rp["a"][v]).max(), 1e-300) for v in np.nonzero(solved & ~und)[0]), default=np.inf)
    print("%s: undecided %d of %d, smallest gap / e %.3g, solves mean %.2f max %d" % (label, und.sum(), solved.sum(), ratio,
                                                                                     r["niter"][solved].mean(), r["niter"][solved].max()))
    assert und.sum() == 0, "%s: choose another seed: the restatement reports %d undecided voxels" % (label, und.sum())
    assert np.array_equal(r["niter"][solved], rp["niter"][solved])
    nreg = c["sph"].nvert
    for t_ in range(c["niso"]):
        assert r["iso_in"][solved, t_].any() and r["iso_out"][solved, t_].any(), "%s: isotropic row %d is never %s the set" % (
            label, t_, "in" if not r["iso_in"][solved, t_].any() else "out of")
    larger, smaller = 2 * r["setmax"][solved] > nreg, 2 * r["setmin"][solved] <= nreg
    print("%s: voxels with a pass whose WM set is the larger side %d, the smaller side %d" % (label, larger.sum(), smaller.sum()))
    assert larger.any() and smaller.any(), label + ": one side of the complement switch (2 count > nreg) is never met"
    return t, r, rp, solved


def gpu_msmt(fj, torch_, plan, dwi, mask):
    dev = torch_.device("cuda", 0)
    out = fj.msmt.msmt_rec_device(plan, torch_.from_numpy(np.ascontiguousarray(dwi)).to(dev), torch_.from_numpy(np.ascontiguousarray(mask)).to(dev))
    torch_.cuda.synchronize()
    nvox = len(mask)
    return dict(sh=out["sh"].cpu().numpy().T, iso=np.stack([x.cpu().numpy() for x in out["iso"]], 1) if out["iso"] else np.zeros((nvox, 0), np.float32),
                odf=out["odf"].cpu().numpy().T, niter=out["niter"].cpu().numpy(),
                peak=np.stack([p.cpu().numpy().T for p in out["peak"]], 1), f=np.stack([f.cpu().numpy() for f in out["f"]], 1))


def hold(c, got, r, rp, solved):
    """the pass rule of the module docstring; prints each figure before it asserts"""
    label, sph = c["label"], c["sph"]
    for k in ("sh", "iso", "odf", "niter", "peak", "f"):
        assert not got[k][~solved].any(), "%s: %s is not 0 in a skipped voxel" % (label, k)
    assert solved.any()
    assert np.array_equal(got["niter"][solved], r["niter"][solved].astype(np.float32)), \
        "%s: niter %s, restatement %s" % (label, got["niter"][solved], r["niter"][solved])
    tol = {}
    for k in ("sh", "iso", "odf"):
        if not r[k].shape[1]:
            continue
        d = np.abs(r[k][solved] - rp[k][solved]).max()
        tol[k] = 4 * d + 1e-6 * np.abs(r[k][solved]).max()
        err = np.abs(got[k][solved].astype(np.float64) - r[k][solved]).max()
        print("%s: %s  d %.3g  max|ref| %.4g  tolerance %.3g  gpu error %.3g" % (label, k, d, np.abs(r[k][solved]).max(), tol[k], err))
        assert err <= tol[k], "%s: %s deviates by %.3g > %.3g" % (label, k, err, tol[k])
    V = np.asarray(sph.vertices, np.float32)
    pk, amp, top, nval = csd_ref.peaks(r["odf"], V, sph.faces)
    for v in np.nonzero(solved)[0]:
        for k in range(3):
            assert abs(float(got["f"][v, k]) - float(amp[v, k])) <= tol["odf"], "%s: voxel %d peak %d amplitude %g, restatement %g" % (label, v, k, got["f"][v, k], amp[v, k])
            if got["f"][v, k] == 0:
                assert not got["peak"][v, k].any()
                continue
            gi = int(np.argmax(V[:sph.nvert] @ got["peak"][v, k]))
            assert np.array_equal(V[gi], got["peak"][v, k]), "%s: voxel %d peak %d is no vertex" % (label, v, k)
            assert got["f"][v, k] == got["odf"][v, gi]
            if k < nval[v] and gi != top[v, k]:                   # another vertex: a tie in the float64 odf
                assert abs(r["odf"][v, gi] - r["odf"][v, top[v, k]]) <= tol["odf"], "%s: voxel %d peak %d at vertex %d, restatement %d" % (label, v, k, gi, top[v, k])


def run_case(fj, torch_, **kw):
    c = make_case(fj, **kw)
    plan = fj.MsmtPlan(c["bval"], c["bvec"], c["resp"], c["sph"], lmax=c["lmax"], **c["kw"])
    try:
        t, r, rp, solved = reference(fj, c, plan.tables())
        got = gpu_msmt(fj, torch_, plan, c["s"].T, c["mask"])
        hold(c, got, r, rp, solved)
        return c, plan.tables(), r
    finally:
        plan.close()


@pytest.mark.parametrize("lmax,niso", [(8, 0), (8, 1), (8, 2), (6, 1), (6, 2), (4, 2), (2, 2)])
def test_orders_and_tissue_counts(fj, torch_, lmax, niso):
    """n = 45, 46, 47 (six blocks, the last partly filled), 29, 30, 17 (three blocks), 8 (one full block), on three shells and b0"""
    run_case(fj, torch_, lmax=lmax, niso=niso, seed=10 * lmax + niso)


# (nb0, directions per shell, seed of the directions).  With n + 2 frames all but two directions are on the outer shell, where the high
# orders have a response to speak of, and the seed is one whose 45 random directions determine them (sigma_min / sigma_max of X 2.2e-4)
FRAMES = {49: (2, (1, 1, 45), 3), 64: (4, (20, 20, 20), 5), 65: (5, (20, 20, 20), 5), 270: (18, (84, 84, 84), 5), 300: (18, (94, 94, 94), 5),
          512: (5, (169, 169, 169), 5)}


@pytest.mark.parametrize("nvol", sorted(FRAMES))
def test_frame_counts(fj, torch_, nvol):
    """n + 2 frames, one wave's worth of samples and one more, the headline 270, 300, and the limit of 512 where the workgroup's LDS is
    largest (160 448 B)"""
    nb0, ndirs, sseed = FRAMES[nvol]
    c, _, _ = run_case(fj, torch_, nb0=nb0, ndirs=ndirs, scheme_seed=sseed, seed=nvol)
    assert len(c["bval"]) == nvol


def test_a_series_past_the_limit_is_refused(fj):
    bval, bvec = msmt_ref.scheme(nb0=6, ndirs=(169, 169, 169))
    shell, bbar = msmt_ref.shells(bval)
    wm_R, iso_r = msmt_ref.model_responses(bbar, 8)
    with pytest.raises(fj.FibersError) as e:
        fj.MsmtPlan(bval, bvec, fj.MsmtResponse(bbar, wm_R, iso_r), fj.sphere_724, lmax=8)
    assert len(bval) == 513 and e.value.code == -7 and "513" in str(e.value) and "512" in str(e.value), str(e.value)


@pytest.mark.parametrize("name", ["sphere_362", "sphere_642", "sphere_724"])
def test_tessellations(fj, torch_, name):
    """183, 323 and 364 constraint rows beside the two isotropic ones: three, six and six ballot words, the last partly filled"""
    run_case(fj, torch_, sphere=name, seed=31)


@pytest.mark.parametrize("kw", [dict(tau=0.1), dict(niter=1), dict(niter=3), dict(lam=0.3, lam_iso=3.0)], ids=["tau0.1", "niter1", "niter3", "weights"])
def test_threshold_iteration_cap_and_weights(fj, torch_, kw):
    c, t, r = run_case(fj, torch_, seed=5, **kw)
    if "niter" in kw:
        solved = (c["mask"] != 0) & (c["s"] > 0).any(1)
        full = msmt_ref.rec(c["s"], t["X"], t["B"], t["Y"], c["nwm"])
        assert (r["niter"][solved] == kw["niter"]).any() and (full["niter"][solved] > kw["niter"]).any(), "no voxel reaches the cap of %d solves" % kw["niter"]


def test_plan_tables_equal_the_design(fj, torch_):
    c = make_case(fj, lmax=6, niso=2, sphere="sphere_642", lam=0.5, lam_iso=2.0)
    plan = fj.MsmtPlan(c["bval"], c["bvec"], c["resp"], c["sph"], lmax=6, lam=0.5, lam_iso=2.0)
    t, want = plan.tables(), fj.msmt_design(c["bval"], c["bvec"], c["resp"], c["sph"], lmax=6, lam=0.5, lam_iso=2.0)
    assert (plan.n, plan.nwm, plan.niso, plan.nreg, plan.nshells) == (30, 28, 2, 321, 4)
    for k in ("shell", "bbar", "X", "B", "Y"):
        assert np.array_equal(t[k], want[k]), k
    a = gpu_msmt(fj, torch_, plan, c["s"].T, c["mask"])
    b = gpu_msmt(fj, torch_, plan, c["s"].T[:, :11], c["mask"][:11])        # a smaller call on the same plan, then the first one again
    again = gpu_msmt(fj, torch_, plan, c["s"].T, c["mask"])
    plan.close()
    for k in a:
        assert np.array_equal(a[k], again[k]) and np.array_equal(a[k][:11], b[k]), k


K = 61           # distinct voxels of the large call: prime, so a wave's successive voxels (a stride of 8 x the grid apart) differ in kind


@pytest.mark.parametrize("lmax,niso,name", [(8, 2, "sphere_724"), (4, 1, "sphere_362")])
def test_more_voxels_than_one_round_of_the_grid(fj, torch_, lmax, niso, name):
    """msmt_kernel (csrc/msmt.hip) runs min(cdiv(nvox, 8), CUs x (B in LDS ? 1 : 2)) workgroups of 8 waves, a voxel a wave a round (the
    grid rule of fibd_msmt_rec; B is in LDS at lmax 8): with nvox = 2 cap + 8 + 3 every wave takes a second voxel, some a third, and the
    last workgroup is partial.  Voxel i is a copy of voxel i % 61 of a small call that stays inside the first round and passes `hold`;
    every seventh is masked out.  The large call must repeat the small one bit for bit, whatever a wave's previous voxel left in its
    LDS and registers; so must the small call again on the plan whose peak buffers the large one has grown."""
    cu = torch_.cuda.get_device_properties(0).multi_processor_count
    per_cu = 1 if lmax == 8 else 2
    cap = cu * W * per_cu
    nvox = 2 * cap + W + 3
    c = make_case(fj, lmax=lmax, niso=niso, sphere=name, nvox=K, seed=7)
    c["mask"][:] = 1
    plan = fj.MsmtPlan(c["bval"], c["bvec"], c["resp"], c["sph"], lmax=lmax)
    try:
        grid = min(-(-nvox // W), cu * per_cu)
        print("%s: %d CUs, first round = %d voxels (%d workgroups x %d waves), %.2f rounds" % (c["label"], cu, cap, grid, W, nvox / (grid * W)))
        assert grid * W == cap and nvox > 2 * cap and nvox % W and K <= cap
        t, r, rp, solved = reference(fj, c, plan.tables())
        dwi = c["s"].T
        small = gpu_msmt(fj, torch_, plan, dwi, c["mask"])
        hold(c, small, r, rp, solved)
        idx = np.arange(nvox) % K
        mask = (np.arange(nvox) % 7 != 3).astype(np.uint8)
        big = gpu_msmt(fj, torch_, plan, dwi[:, idx], mask)
        inside = mask != 0
        assert cap % K and (2 * cap) % K                                                      # (successive voxels of a wave do differ)
        for k in ("sh", "iso", "odf", "niter", "peak", "f"):
            assert not big[k][~inside].any(), "%s: %s is not 0 in a masked voxel" % (c["label"], k)
            got, want = (np.ascontiguousarray(a, np.float32).view(np.uint32).reshape(nvox, -1) for a in (big[k], small[k][idx]))
            bad = np.nonzero((got != want).any(1) & inside)[0]
            assert not bad.size, "%s: %s differs from the small call in %d voxels, the first %s (rounds %s)" % (
                c["label"], k, bad.size, bad[:8], bad[:8] // cap)
        again = gpu_msmt(fj, torch_, plan, dwi, c["mask"])
        for k in small:
            assert np.array_equal(again[k].view(np.uint32), small[k].view(np.uint32)), "%s: %s of the small call differs after the large one" % (c["label"], k)
    finally:
        plan.close()


def _volume(fj, shape, lmax, niso, sphere, seed):
    """a volume whose voxel i (memory order) is voxel i % 60 of a 60-voxel pool, with a holed mask"""
    n = int(np.prod(shape))
    c = make_case(fj, lmax=lmax, niso=niso, sphere=sphere, nvox=60, seed=seed)
    idx = np.arange(n) % 60
    mask3 = np.ones(shape, np.uint8, order="F")
    mask3[1:3, 1:3, 1] = 0
    mask3[0, :, shape[2] - 1] = 0
    dwi = np.ascontiguousarray(c["s"].T[:, idx])                                          # [nvol, n]
    dwi4 = np.asfortranarray(dwi.T.reshape(shape + (dwi.shape[0],), order="F"))
    return c, dwi, dwi4, mask3, n


def _flat(res, n):
    return dict(sh=res.sh.vol.reshape(n, -1, order="F"), iso=np.stack([x.vol.reshape(n, order="F") for x in res.iso], 1),
                odf=res.odf.vol.reshape(n, -1, order="F"), niter=res.niter.vol.reshape(n, order="F"),
                peak=np.stack([p.vol.reshape(n, 3, order="F") for p in res.peak], 1), f=np.stack([f.vol.reshape(n, order="F") for f in res.f], 1))


@pytest.mark.parametrize("shape,lmax,chunks", [((5, 4, 3), 8, 1), ((16, 13, 6), 4, 2)])
def test_host_path_equals_the_device_path(fj, torch_, monkeypatch, shape, lmax, chunks):
    """fib_msmt_rec byte for byte fibd_msmt_rec: as one chunk, under FIBERS_HOST_CHUNK, and on the device set of one device.  The host
    tier's smallest chunk is 1024 voxels, so the 5 x 4 x 3 volume is always one chunk; in the 16 x 13 x 6 volume (1248 voxels, copies of
    the 60-voxel pool) the boundary at voxel 1024 falls inside."""
    c, dwi, dwi4, mask3, n = _volume(fj, shape, lmax, 2, "sphere_362", 59)
    assert (n > 1024) == (chunks > 1)
    plan = fj.MsmtPlan(c["bval"], c["bvec"], c["resp"], c["sph"], lmax=lmax)
    dev = gpu_msmt(fj, torch_, plan, dwi, mask3.reshape(-1, order="F"))
    c["mask"][:] = 1
    t, r, rp, solved = reference(fj, c, plan.tables())
    first = {k: v[:60] for k, v in dev.items()}
    hold(c, first, r, rp, solved & (mask3.reshape(-1, order="F")[:60] != 0))
    plan.close()
    vol, mask = fj.MRI(dwi4, c["bval"], c["bvec"]), fj.MRI(mask3)

    def same(host):
        h = _flat(host, n)
        for k in dev:
            assert np.array_equal(h[k], dev[k]), "host path %s differs from the device path" % k
    try:
        same(fj.msmt_rec(vol, mask, c["resp"], c["sph"], lmax=lmax))
        monkeypatch.setenv("FIBERS_HOST_CHUNK", "1024")
        same(fj.msmt_rec(vol, mask, c["resp"], c["sph"], lmax=lmax))
        fj.init([0])
        same(fj.msmt_rec(vol, mask, c["resp"], c["sph"], lmax=lmax, device=fj.DEVICE_ALL))
    finally:
        fj.shutdown()


def test_result_geometry_files_and_tractography(fj, tmp_path):
    """msmt_rec returns an MSMT whose volumes carry the input's geometry; msmt_write / read_struct round-trip; prob_stream, stream and
    str_weights take the result like a CSD"""
    shape = (12, 12, 3)
    bval, bvec = msmt_ref.scheme(nb0=6, ndirs=(20, 20, 20))
    shell, bbar = msmt_ref.shells(bval)
    wm_R, iso_r = msmt_ref.model_responses(bbar, 8)
    resp = fj.MsmtResponse(bbar, wm_R, iso_r)
    rng = np.random.default_rng(2)
    vol = np.zeros(shape + (len(bval),), np.float32, order="F")
    mask3 = np.zeros(shape, np.uint8, order="F")
    for x in range(12):
        for y in range(12):
            fib = ([[1, 0, 0]] if 4 <= y < 8 else []) + ([[0, 1, 0]] if 4 <= x < 8 else [])
            if not fib:
                continue
            mask3[x, y, :] = 1
            for z in range(3):
                vol[x, y, z] = msmt_ref.mixture(bvec, shell, bbar, wm_R, iso_r, fib, [0.8 / len(fib)] * len(fib), iso_w=(0.1, 0.1)) + rng.normal(0, 20.0, len(bval))
    v2r = np.array([[-2.0, 0, 0, 90], [0, 0, 2.0, -126], [0, -2.0, 0, 72], [0, 0, 0, 1]], np.float32)
    dwi = fj.MRI(vol, bval, bvec, volres=(2.0, 2.0, 2.0), vox2ras=v2r)
    mask = fj.MRI(mask3, volres=(2.0, 2.0, 2.0), vox2ras=v2r)
    m = fj.msmt_rec(dwi, mask, resp)
    assert isinstance(m, fj.MSMT) and len(m.iso) == 2 and len(m.peak) == 3 and len(m.f) == 3
    assert m.sh.vol.shape == shape + (45,) and m.odf.vol.shape == shape + (362,) and m.iso[1].vol.shape[:3] == shape and m.peak[2].vol.shape == shape + (3,)
    for x in [m.sh, m.odf, m.niter] + m.iso + m.peak + m.f:
        assert np.array_equal(x.vox2ras, v2r) and tuple(x.volres[:3]) == (2.0, 2.0, 2.0)
    assert m.niter.vol.max() >= 1 and not m.odf.vol[mask3 == 0].any() and not m.iso[0].vol[mask3 == 0].any()
    centre = m.peak[0].vol[5, 5, 1], m.peak[1].vol[5, 5, 1]
    assert sorted(int(np.argmax(np.abs(c))) for c in centre) == [0, 1] and m.f[1].vol[5, 5, 1] > 0.3 * m.f[0].vol[5, 5, 1]
    assert int(np.argmax(np.abs(m.peak[0].vol[0, 5, 1]))) == 0 and int(np.argmax(np.abs(m.peak[0].vol[5, 0, 1]))) == 1
    fj.msmt_write(m, str(tmp_path / "msmt"))
    back = fj.read_struct(str(tmp_path / "msmt"), fj.MSMT)
    for k in ("sh", "odf", "niter"):
        assert np.array_equal(getattr(back, k).vol, getattr(m, k).vol), k
    for k in ("iso", "peak", "f"):
        assert len(getattr(back, k)) == len(getattr(m, k))
        for a, b in zip(getattr(back, k), getattr(m, k)):
            assert np.array_equal(a.vol, b.vol), k
    tr = fj.prob_stream(m, fj.sphere_724, mask=mask, nsub=1)
    assert len(tr.npts) > 0 and int(np.max(tr.npts)) >= 6
    w = fj.str_weights(tr, m, mask=mask)
    assert len(w.weights) == len(tr.npts) and np.isfinite(w.weights).all()
    tr2 = fj.stream(m.peak, f=m.f, mask=mask, nsub=1)
    assert len(tr2.npts) > 0 and int(np.max(tr2.npts)) >= 6
