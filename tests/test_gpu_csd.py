"""csd_rec on the GPU against the float64 restatement (tests/csd_ref.py) on the plan's own tables.

Pass rule, per case and per field: |gpu - ref64| <= 4 d + 1e-6 max|ref64|, d = the largest deviation between the restatement's two
summation orders (the shell frames permuted) on that case, 1e-6 max = DESIGN.md §5's allowance for the one float32 rounding of the
output.  niter must be equal on every compared voxel.  Voxels whose restatement margin (min |a - thr| / max|a| over all passes) is
below 1e-9 would be left out; the seeds here are chosen so that the restatement reports none, and `hold` asserts that.  A peak on a
different vertex must be a tie in the float64 odf within the odf tolerance."""
import ctypes as C

import numpy as np
import pytest

import csd_ref

pytestmark = pytest.mark.gpu

RESP = (1.7e-3, 0.3e-3, 1000.0)
W = 8            # voxels per workgroup (one wave each)


@pytest.fixture(scope="module")
def torch_():
    import torch
    return torch


def voxels(bval, bvec, frames, nvox, seed, noise=1.0 / 30.0):
    """shell samples float32 [nvox, nshell]: 1, 2 and 3 fibres in turn with random axes, weights and s0 in [800, 1200], Gaussian noise;
    voxel 3 (if there) is isotropic, 4 has no positive sample, 5 is of mixed sign"""
    rng = np.random.default_rng(seed)
    out = np.zeros((nvox, len(frames)))
    for i in range(nvox):
        nf = 1 + i % 3
        u = rng.normal(size=(nf, 3))
        w = rng.uniform(0.3, 1.0, nf)
        s0 = rng.uniform(800.0, 1200.0)
        out[i] = csd_ref.signal(bval, bvec, frames, u, w / w.sum(), RESP[0], RESP[1], s0)
        if i == 3:
            out[i] = csd_ref.signal(bval, bvec, frames, [], [], RESP[0], RESP[1], s0, iso=1.0)
        out[i] += rng.normal(0.0, s0 * noise, len(frames))
    if nvox > 4:
        out[4] = -np.abs(out[4])
        out[4, 0] = 0.0
    if nvox > 5:
        out[5, ::2] *= -1.0
    return out.astype(np.float32)


def full_dwi(s, frames, nvol, seed):
    """[nvol, nvox]: the shell samples at their frames, noise everywhere else (those frames must not be read)"""
    dwi = np.random.default_rng(seed).uniform(-50.0, 2000.0, (nvol, s.shape[0])).astype(np.float32)
    dwi[frames] = s.T
    return dwi


def gpu_csd(fj, torch_, plan, dwi, mask):
    dev = torch_.device("cuda", 0)
    out = fj.csd.csd_rec_device(plan, torch_.from_numpy(np.ascontiguousarray(dwi)).to(dev), torch_.from_numpy(np.ascontiguousarray(mask)).to(dev))
    torch_.cuda.synchronize()
    return dict(sh=out["sh"].cpu().numpy().T, odf=out["odf"].cpu().numpy().T, niter=out["niter"].cpu().numpy(),
                peak=np.stack([p.cpu().numpy().T for p in out["peak"]], 1), f=np.stack([f.cpu().numpy() for f in out["f"]], 1))


def hold(fj, got, s, mask, t, sphere, label, tau=0.1, niter=50):
    """the pass rule of the module docstring; prints each figure before it asserts.  Returns (d of odf, smallest margin)."""
    r = csd_ref.rec(s, t["X"], t["B"], t["Y"], tau=tau, niter=niter)
    rp = csd_ref.rec(s, t["X"], t["B"], t["Y"], tau=tau, niter=niter, perm=np.random.default_rng(7).permutation(s.shape[1]))
    inside = mask != 0
    solved = inside & (s > 0).any(1)
    low = solved & (r["margin"] < 1e-9)
    print("%s: margin min %.3g, left out %d of %d" % (label, r["margin"][solved].min() if solved.any() else np.inf, low.sum(), len(mask)))
    assert low.sum() == 0, "%s: choose another seed: the restatement reports %d voxels within 1e-9 of another set" % (label, low.sum())
    assert np.array_equal(r["niter"][solved], rp["niter"][solved]), label + ": the restatement's two orders take different numbers of solves"
    for k in ("sh", "odf", "niter", "peak", "f"):
        assert not got[k][~solved].any(), "%s: %s is not 0 in a skipped voxel" % (label, k)
    if not solved.any():
        return 0.0, np.inf
    assert np.array_equal(got["niter"][solved], r["niter"][solved].astype(np.float32)), \
        "%s: niter %s, restatement %s" % (label, got["niter"][solved], r["niter"][solved])
    tol = {}
    for k in ("sh", "odf"):
        d = np.abs(r[k][solved] - rp[k][solved]).max()
        tol[k] = 4 * d + 1e-6 * np.abs(r[k][solved]).max()
        err = np.abs(got[k][solved].astype(np.float64) - r[k][solved]).max()
        print("%s: %s  d %.3g  max|ref| %.4g  tolerance %.3g  gpu error %.3g" % (label, k, d, np.abs(r[k][solved]).max(), tol[k], err))
        assert err <= tol[k], "%s: %s deviates by %.3g > %.3g" % (label, k, err, tol[k])
    # peaks: the existing peak finder on the GPU's float32 odf; against find_peaks! on the restatement's odf
    V = np.asarray(sphere.vertices, np.float32)
    pk, amp, top, nval = csd_ref.peaks(r["odf"], V, sphere.faces)
    for v in np.nonzero(solved)[0]:
        for k in range(3):
            assert abs(float(got["f"][v, k]) - float(amp[v, k])) <= tol["odf"], "%s: voxel %d peak %d amplitude %g, restatement %g" % (label, v, k, got["f"][v, k], amp[v, k])
            if got["f"][v, k] == 0:
                assert not got["peak"][v, k].any()
                continue
            gi = int(np.argmax(V[:sphere.nvert] @ got["peak"][v, k]))
            assert np.array_equal(V[gi], got["peak"][v, k]), "%s: voxel %d peak %d is no vertex" % (label, v, k)
            assert got["f"][v, k] == got["odf"][v, gi]
            if k < nval[v] and gi != top[v, k]:                   # another vertex: a tie in the float64 odf
                assert abs(r["odf"][v, gi] - r["odf"][v, top[v, k]]) <= tol["odf"], "%s: voxel %d peak %d at vertex %d, restatement %d" % (label, v, k, gi, top[v, k])
    return float(np.abs(r["odf"][solved] - rp["odf"][solved]).max()), float(r["margin"][solved].min())


def run_case(fj, torch_, label, ndir, lmax, sphere, nvox, seed, mask=None, bval=None, bvec=None, **kw):
    if bval is None:
        bval, bvec = csd_ref.scheme(ndir, lmax)
    plan = fj.CsdPlan(bval, bvec, RESP, sphere, lmax=lmax, **kw)
    try:
        t = plan.tables()
        s = voxels(bval, bvec, t["frames"], nvox, seed)
        mask = np.ones(nvox, np.uint8) if mask is None else mask
        got = gpu_csd(fj, torch_, plan, full_dwi(s, t["frames"], len(bval), seed + 1), mask)
        return hold(fj, got, s, mask, t, sphere, label, tau=kw.get("tau", 0.1), niter=kw.get("niter", 50))
    finally:
        plan.close()


CASES = [(lmax, nd) for lmax in (2, 4, 6, 8) for nd in sorted({csd_ref.ncoef(lmax), csd_ref.ncoef(lmax) + 1, 47, 61, 64, 84})]


@pytest.mark.parametrize("lmax,ndir", CASES)
def test_orders_and_shell_sizes(fj, torch_, lmax, ndir):
    """lmax 2, 4, 6, 8 with nshell = n, n + 1, 47, 61, 64, 84; 13 voxels: more than one workgroup, the last one partial"""
    run_case(fj, torch_, "lmax %d, %d frames" % (lmax, ndir), ndir, lmax, fj.sphere_724, 13, 100 * lmax + ndir)


@pytest.mark.parametrize("name", ["sphere_362", "sphere_642", "sphere_724"])
@pytest.mark.parametrize("lmax", [6, 8])
def test_tessellations(fj, torch_, name, lmax):
    run_case(fj, torch_, "%s lmax %d" % (name, lmax), 64, lmax, getattr(fj, name), 12, 31 + lmax)


@pytest.mark.parametrize("nvox", [1, W - 1, W, W + 1, 300])
def test_launch_shapes_and_voxel_kinds(fj, torch_, nvox):
    """1, 2 and 3 fibres with noise, an isotropic voxel, one without a positive sample, one of mixed sign; at 300 voxels every tenth is
    masked out.  Skipped outputs are 0 (`hold` asserts it)."""
    mask = np.ones(nvox, np.uint8)
    if nvox >= 300:
        mask[::10] = 0
    d, margin = run_case(fj, torch_, "%d voxels" % nvox, 84, 8, fj.sphere_724, nvox, 11, mask=mask)
    if nvox >= 300:
        print("300 voxels at lmax 8, 84 frames: d(odf) = %.3g, smallest margin %.3g" % (d, margin))


K = 61           # distinct voxels of the large call: prime, so a wave's successive voxels (a stride of 8 x the grid apart) differ in kind


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


@pytest.mark.parametrize("lmax,name,ndir", [(8, "sphere_724", 84), (6, "sphere_642", 61), (2, "sphere_362", 7)])
def test_more_voxels_than_one_round_of_the_grid(fj, torch_, lmax, name, ndir):
    """csd_kernel (csrc/csd.hip) runs min(cdiv(nvox, 8), CUs x (B in LDS ? 1 : 2)) workgroups of CSD_NW = 8 waves, a voxel a wave a
    round (the grid rule of fibd_csd_rec): with nvox = 2 cap + 8 + 3 every wave takes a second voxel, some a third, and the last
    workgroup is partial.  Voxel i is a copy of voxel i % 61 of a small call that stays inside the first round and passes `hold`; every
    seventh is masked out.  The large call must repeat the small one bit for bit, whatever a wave's previous voxel left in its LDS
    (the factor, fw, sw) and registers; so must the small call again on the plan whose peak buffers the large one has grown.  B is in
    LDS at lmax 8, read through the cache at 6 and 2 (n0 == n at 2)."""
    sphere = getattr(fj, name)
    cu = torch_.cuda.get_device_properties(0).multi_processor_count
    cap = cu * W * (1 if lmax == 8 else 2)
    nvox = 2 * cap + W + 3
    label = "lmax %d, %s, %d frames, %d voxels" % (lmax, name, ndir, nvox)
    bval, bvec = csd_ref.scheme(ndir, lmax)
    plan = fj.CsdPlan(bval, bvec, RESP, sphere, lmax=lmax)
    try:
        t = plan.tables()
        grid = min(-(-nvox // W), cu * (1 if lmax == 8 else 2))
        print("%s: %d CUs, first round of csd_kernel's grid rule = %d voxels (%d workgroups x %d waves), %.2f rounds" % (
            label, cu, cap, grid, W, nvox / (grid * W)))
        assert grid * W == cap and nvox > 2 * cap and nvox % W, \
            "%s does not pass two rounds of %d voxels (csd_kernel's grid rule in fibd_csd_rec, csrc/csd.hip, on %d CUs)" % (label, cap, cu)
        assert K <= cap
        s = voxels(bval, bvec, t["frames"], K, 7)
        dwi = full_dwi(s, t["frames"], len(bval), 8)
        ones = np.ones(K, np.uint8)
        small = gpu_csd(fj, torch_, plan, dwi, ones)
        hold(fj, small, s, ones, t, sphere, label + ": the %d distinct voxels" % K)
        # both accumulation routes of P are met: the restatement says so, not the seed
        r = csd_ref.rec(s, t["X"], t["B"], t["Y"])
        solved = (s > 0).any(1)
        larger, smaller = 2 * r["setmax"][solved] > plan.nreg, 2 * r["setmin"][solved] <= plan.nreg
        print("%s: voxels with a pass whose set is the larger side %d, the smaller side %d, of %d solved" % (label, larger.sum(), smaller.sum(), solved.sum()))
        assert larger.any() and smaller.any(), label + ": one side of the complement switch (2 count > nreg) is never met"
        idx = np.arange(nvox) % K
        mask = (np.arange(nvox) % 7 != 3).astype(np.uint8)
        big = gpu_csd(fj, torch_, plan, dwi[:, idx], mask)
        inside = mask != 0
        assert cap % K and (2 * cap) % K                                                      # (successive voxels of a wave do differ)
        for k in ("sh", "odf", "niter", "peak", "f"):
            assert not big[k][~inside].any(), "%s: %s is not 0 in a masked voxel" % (label, k)
            got, want = (np.ascontiguousarray(a, np.float32).view(np.uint32).reshape(nvox, -1) for a in (big[k], small[k][idx]))
            bad = np.nonzero((got != want).any(1) & inside)[0]
            assert not bad.size, "%s: %s differs from the small call in %d voxels, the first %s (rounds %s)" % (
                label, k, bad.size, bad[:8], bad[:8] // cap)
        again = gpu_csd(fj, torch_, plan, dwi, ones)
        for k in small:
            assert _same_bits(again[k], small[k]), "%s: %s of the small call differs after the large one" % (label, k)
    finally:
        plan.close()


@pytest.mark.parametrize("ndir", [65, 128, 129, 255, 256])
def test_shell_sizes_up_to_the_limit(fj, torch_, ndir):
    """the sample load walks lane, lane + 64, ...: one frame past a wave, two and four waves' worth and one frame either side, up to
    CSD_MAXSHELL = 256 (csrc/csd.hip), where the workgroup's LDS is largest"""
    run_case(fj, torch_, "lmax 8, %d frames" % ndir, ndir, 8, fj.sphere_724, 13, 800 + ndir)


def test_a_shell_past_the_limit_is_refused(fj):
    bval, bvec = csd_ref.scheme(257, 8)
    with pytest.raises(fj.FibersError) as e:
        fj.CsdPlan(bval, bvec, RESP, fj.sphere_724, lmax=8)
    assert e.value.code == -7 and "257" in str(e.value) and "256" in str(e.value), str(e.value)


@pytest.mark.parametrize("kw", [dict(niter=1), dict(niter=2), dict(tau=0.0), dict(lam=0.1), dict(tau=0.3, lam=3.0)],
                         ids=["niter1", "niter2", "tau0", "lambda0.1", "tau0.3-lambda3"])
def test_iteration_cap_threshold_and_weight(fj, torch_, kw):
    run_case(fj, torch_, str(kw), 64, 8, fj.sphere_724, 24, 5, **kw)
    run_case(fj, torch_, str(kw) + " lmax 6", 61, 6, fj.sphere_362, 9, 6, **kw)


def test_multi_shell_table_with_interleaved_b0s(fj, torch_):
    """three shells and b0s interleaved frame by frame: the kernel gathers the frames of the chosen shell, here the middle one"""
    rng = np.random.default_rng(3)
    g = rng.normal(size=(64, 3))
    g /= np.linalg.norm(g, axis=1)[:, None]
    bval, bvec = [], []
    for i in range(64):
        bval += [0.0 if i % 2 else 5.0, 1000.0, 2000.0 + (i % 3 - 1) * 40.0, 3000.0]
        bvec += [np.zeros(3), g[(i + 7) % 64], g[i], g[(i + 21) % 64]]
    bval, bvec = np.array(bval, np.float32), np.array(bvec, np.float32)
    plan = fj.CsdPlan(bval, bvec, RESP, fj.sphere_724, lmax=8, shell=2000.0)
    t = plan.tables()
    plan.close()
    assert np.array_equal(t["frames"], np.arange(64) * 4 + 2)
    run_case(fj, torch_, "multi-shell", 64, 8, fj.sphere_724, 20, 41, bval=bval, bvec=bvec, shell=2000.0)
    run_case(fj, torch_, "multi-shell, outer", 64, 6, fj.sphere_642, 10, 42, bval=bval, bvec=bvec)


def test_plan_tables_and_reuse(fj, torch_):
    bval, bvec = csd_ref.scheme(61, 6)
    plan = fj.CsdPlan(bval, bvec, RESP, fj.sphere_642, lmax=6, lam=0.5)
    t, want = plan.tables(), fj.csd_design(bval, bvec, RESP, fj.sphere_642, lmax=6, lam=0.5)
    assert plan.nshell == 61 and plan.n == 28 and plan.nreg == 321
    for k in ("frames", "R", "X", "B", "Y"):
        assert np.array_equal(t[k], want[k]), k
    s = voxels(bval, bvec, t["frames"], 40, 9)
    dwi = full_dwi(s, t["frames"], len(bval), 10)
    mask = np.ones(40, np.uint8)
    a = gpu_csd(fj, torch_, plan, dwi, mask)
    b = gpu_csd(fj, torch_, plan, dwi[:, :17], mask[:17])        # a smaller call on the same plan, then the first one again
    c = gpu_csd(fj, torch_, plan, dwi, mask)
    plan.close()
    for k in a:
        assert np.array_equal(a[k], c[k]) and np.array_equal(a[k][:17], b[k]), k
    hold(fj, a, s, mask, t, fj.sphere_642, "plan reuse")


def _volume(seed=59):
    bval, bvec = csd_ref.scheme(47, 6)
    shape = (9, 7, 5)
    n = int(np.prod(shape))
    frames = csd_ref.shell_frames(bval)
    s = voxels(bval, bvec, frames, n, seed)
    mask3 = np.ones(shape, np.uint8, order="F")
    mask3[2:5, 1:4, 1:3] = 0                                                             # a hole
    mask3[0, :, 4] = 0
    dwi = full_dwi(s, frames, len(bval), seed + 1)                                       # [nvol, n]
    dwi4 = np.asfortranarray(dwi.T.reshape(shape + (len(bval),), order="F"))             # voxel i of s = voxel i in memory order
    return bval, bvec, s, mask3, dwi, dwi4, n


def _flat(res, n):
    return dict(sh=res.sh.vol.reshape(n, -1, order="F"), odf=res.odf.vol.reshape(n, -1, order="F"), niter=res.niter.vol.reshape(n, order="F"),
                peak=np.stack([p.vol.reshape(n, 3, order="F") for p in res.peak], 1), f=np.stack([f.vol.reshape(n, order="F") for f in res.f], 1))


def test_host_path_equals_the_device_path(fj, torch_, monkeypatch):
    """fib_csd_rec on a 9 x 7 x 5 volume with a holed mask: byte for byte fibd_csd_rec, as one chunk, with FIBERS_HOST_CHUNK's schedule
    of several chunks, on the device set of one device, and with two workers on it; the refusals of the host form"""
    bval, bvec, s, mask3, dwi, dwi4, n = _volume()
    plan = fj.CsdPlan(bval, bvec, RESP, fj.sphere_362, lmax=6)
    dev = gpu_csd(fj, torch_, plan, dwi, mask3.reshape(-1, order="F"))
    hold(fj, dev, s, mask3.reshape(-1, order="F"), plan.tables(), fj.sphere_362, "9 x 7 x 5 volume")
    plan.close()
    vol, mask = fj.MRI(dwi4, bval, bvec), fj.MRI(mask3)

    def same(host):
        h = _flat(host, n)
        for k in dev:
            assert np.array_equal(h[k], dev[k]), "host path %s differs from the device path" % k
    try:
        same(fj.csd_rec(vol, mask, RESP, fj.sphere_362, lmax=6))
        monkeypatch.setenv("FIBERS_HOST_CHUNK", "1024")
        same(fj.csd_rec(vol, mask, RESP, fj.sphere_362, lmax=6))
        fj.init([0])
        same(fj.csd_rec(vol, mask, RESP, fj.sphere_362, lmax=6, device=fj.DEVICE_ALL))
        fj.init([0, 0])
        same(fj.csd_rec(vol, mask, RESP, fj.sphere_362, lmax=6, device=fj.DEVICE_ALL))
    finally:
        fj.shutdown()
    from fibers_jl_amd import _lib
    L = fj.lib()
    p = _lib.CsdParams(6, RESP[0], RESP[1], RESP[2], 50.0, 0.0, 0.05, 1.0, 0.1, 50)
    v = np.asfortranarray(fj.sphere_362.vertices, dtype=np.float32)
    fc = np.asfortranarray(fj.sphere_362.faces, dtype=np.int32)
    res = fj.csd_rec(vol, mask, RESP, fj.sphere_362, lmax=6)
    o = _lib.CsdOut(res.sh.vol.ctypes.data, res.odf.vol.ctypes.data, res.niter.vol.ctypes.data,
                    _lib.P3(*[x.vol.ctypes.data for x in res.peak]), _lib.P3(*[x.vol.ctypes.data for x in res.f]))
    args = (v.ctypes.data, v.shape[0], fc.ctypes.data, fc.shape[0], C.byref(p), C.byref(o))
    assert L.fib_csd_rec(0, dwi4.ctypes.data, 9, 7, 5, len(bval), mask3.ctypes.data, 0, None, None, *args) == -4
    assert L.fib_csd_rec(0, dwi4.ctypes.data, 9, 7, 5, len(bval), mask3.ctypes.data, 0, bval.ctypes.data, None, *args) == -5
    with pytest.raises(fj.FibersError, match="at least 28 frames"):
        fj.csd_rec(fj.MRI(np.asfortranarray(dwi4[..., :30]), bval[:30], bvec[:30]), mask, RESP, fj.sphere_362, lmax=6)
    with pytest.raises(fj.FibersError, match="at least 28 frames"):
        fj.CsdPlan(bval[:30], bvec[:30], RESP, fj.sphere_362, lmax=6)


def test_csd_write_round_trips_through_files(fj, tmp_path):
    bval, bvec, s, mask3, dwi, dwi4, n = _volume(60)
    res = fj.csd_rec(fj.MRI(dwi4, bval, bvec), fj.MRI(mask3), RESP, fj.sphere_362, lmax=4)
    assert res.sh.vol.shape == (9, 7, 5, 15) and res.odf.vol.shape == (9, 7, 5, 181) and res.peak[2].vol.shape == (9, 7, 5, 3)
    assert res.niter.vol.max() >= 1 and not res.odf.vol[mask3 == 0].any()
    fj.csd_write(res, str(tmp_path / "csd"))
    back = fj.read_struct(str(tmp_path / "csd"), fj.CSD)
    for k in ("sh", "odf", "niter"):
        assert np.array_equal(getattr(back, k).vol, getattr(res, k).vol), k
    for k in ("peak", "f"):
        for a, b in zip(getattr(back, k), getattr(res, k)):
            assert np.array_equal(a.vol, b.vol), k


def test_tractography_runs_on_a_crossing(fj):
    """two bundles crossing at right angles in a 12 x 12 x 3 slab: prob_stream on the fODF and stream on the peaks return lines, and
    the crossing voxels hold both directions"""
    bval, bvec = csd_ref.scheme(64, 8)
    frames = csd_ref.shell_frames(bval)
    shape = (12, 12, 3)
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
                sig = csd_ref.signal(bval, bvec, frames, fib, [1.0 / len(fib)] * len(fib), *RESP) + rng.normal(0, 20.0, len(frames))
                vol[x, y, z, frames] = sig
                vol[x, y, z, :4] = 1000.0
    csd = fj.csd_rec(fj.MRI(vol, bval, bvec), fj.MRI(mask3), RESP)
    centre = csd.peak[0].vol[5, 5, 1], csd.peak[1].vol[5, 5, 1]
    assert sorted(int(np.argmax(np.abs(c))) for c in centre) == [0, 1] and csd.f[1].vol[5, 5, 1] > 0.3 * csd.f[0].vol[5, 5, 1]
    assert int(np.argmax(np.abs(csd.peak[0].vol[0, 5, 1]))) == 0 and int(np.argmax(np.abs(csd.peak[0].vol[5, 0, 1]))) == 1
    tr = fj.prob_stream(csd, fj.sphere_724, mask=fj.MRI(mask3), nsub=1)
    assert len(tr.npts) > 0 and int(np.max(tr.npts)) >= 6
    tr = fj.stream(csd.peak, f=csd.f, mask=fj.MRI(mask3), nsub=1)
    assert len(tr.npts) > 0 and int(np.max(tr.npts)) >= 6


def test_device_tier_refuses_bad_tensors_in_python(fj, torch_):
    from fibers_jl_amd._dev import ArgError
    bval, bvec = csd_ref.scheme(47, 4)
    plan = fj.CsdPlan(bval, bvec, RESP, fj.sphere_362, lmax=4)
    dev = torch_.device("cuda", 0)
    nvox = 10
    dwi = torch_.rand((len(bval), nvox), device=dev) * 500
    mask = torch_.ones(nvox, dtype=torch_.uint8, device=dev)
    rec = fj.csd.csd_rec_device
    out = rec(plan, dwi, mask)
    assert out["sh"].shape == (15, nvox) and out["odf"].shape == (181, nvox) and out["peak"][0].shape == (3, nvox)

    def strided(t):
        v = torch_.zeros(tuple(t.shape) + (2 * t.element_size(),), dtype=torch_.uint8, device=t.device).view(t.dtype)[..., 0]
        assert not v.is_contiguous() and v.shape == t.shape
        return v
    for name, good in (("dwi", dwi), ("mask", mask)):
        for what, bad in (("a host tensor", good.cpu()), ("a wrong dtype", good.to(torch_.float64)), ("a strided view", strided(good)),
                          ("one element short", good.reshape(-1)[:-1].clone())):
            with pytest.raises(ArgError):
                rec(plan, bad if name == "dwi" else dwi, bad if name == "mask" else mask)
    for k in ("sh", "odf", "niter", "peak", "f"):
        for mut in (lambda t: t.cpu(), lambda t: t.to(torch_.float64), strided, lambda t: t.reshape(-1)[:-1].clone()):
            o = dict(out)
            o[k] = [mut(out[k][0])] + list(out[k][1:]) if isinstance(out[k], list) else mut(out[k])
            with pytest.raises(ArgError):
                rec(plan, dwi, mask, out=o)
    o = dict(out)
    o["peak"] = out["peak"][:2]
    with pytest.raises(ArgError):
        rec(plan, dwi, mask, out=o)
    again = rec(plan, dwi, mask, out=out)
    assert again is out
    plan.close()
