"""NumPy restatement of the registration contract ("Registration", include/fibers_hip.h), independent of the package.  The pyramid,
the range, the binning and the joint histogram are float32 / integer and meant bit for bit; the matrices, the NMI (math.fsum) and the
pattern search are float64.  Volumes are [nz, ny, nx] (x fastest), a series [nframes, nz, ny, nx]; shapes are (nx, ny, nz).  Built
on volxform_ref's pull_back / inside_mask / vol_xform_ref: the sampler is the one of "Volume resampling"."""
import functools
import math

import numpy as np

import volxform_ref as vref

F = np.float32
ROW = 29          # a trace row: level, dof of the stage, chosen index, moved, cost before, 24 candidate costs (NaN beyond 2 dof)


# ---- pyramid and range ------------------------------------------------------------------------------------------------------------
def halve(vol):
    """[nz, ny, nx] -> [ceil(nz/2), ceil(ny/2), ceil(nx/2)]: the float32 sum of the existing voxels of each 2x2x2 block, from 0, dz
    outermost and dx innermost, divided by their count as a float32"""
    v = np.asarray(vol, F)
    nz, ny, nx = v.shape
    oz, oy, ox = (nz + 1) // 2, (ny + 1) // 2, (nx + 1) // 2
    pad = np.zeros((2 * oz, 2 * oy, 2 * ox), F)             # (x + 0 is x for every x once the sum has started from +0)
    cnt = np.zeros(pad.shape, F)
    pad[:nz, :ny, :nx] = v
    cnt[:nz, :ny, :nx] = 1
    s, c = np.zeros((oz, oy, ox), F), np.zeros((oz, oy, ox), F)
    with np.errstate(all="ignore"):
        for dz in range(2):
            for dy in range(2):
                for dx in range(2):
                    s = (s + pad[dz::2, dy::2, dx::2]).astype(F)
                    c = c + cnt[dz::2, dy::2, dx::2]
        return (s / c).astype(F)


def _key(bits):
    return np.where(bits & np.uint32(0x80000000), ~bits, bits | np.uint32(0x80000000))


def _unkey(k):
    k = np.uint32(k)
    return np.uint32(k & np.uint32(0x7FFFFFFF)) if k & np.uint32(0x80000000) else np.uint32(~k)


def vol_range(vol, nbins):
    """(lo, hi, scale, nfinite) of one volume: the extremes of the finite values by the ordered-uint key, scale = float32(nbins) /
    (hi - lo); without a finite value (0, 0, NaN, 0)"""
    b = np.ascontiguousarray(vol, F).reshape(-1).view(np.uint32)
    fin = (b & np.uint32(0x7F800000)) != np.uint32(0x7F800000)
    if not fin.any():
        return F(0), F(0), F(np.nan), 0
    k = _key(b[fin])
    lo = np.array([_unkey(k.min())], np.uint32).view(F)[0]
    hi = np.array([_unkey(k.max())], np.uint32).view(F)[0]
    with np.errstate(all="ignore"):
        scale = F(nbins) / F(hi - lo)
    return lo, hi, F(scale), int(fin.sum())


def bins(v, lo, scale, nbins):
    """(bin int64, has-a-bin bool): t = (v - lo) * scale in float32, two roundings; no bin iff t is NaN; else clamp(floor(t), 0, nbins - 1)"""
    with np.errstate(all="ignore"):
        t = ((np.asarray(v, F) - F(lo)).astype(F) * F(scale)).astype(F)
        ok = ~np.isnan(t)
        b = np.clip(np.floor(np.where(ok, t, F(0))), F(0), F(nbins - 1)).astype(np.int64)
    return b, ok


# ---- the joint histogram ----------------------------------------------------------------------------------------------------------
def reg_hist(fixed, rng_f, moving, rng_m, jobs, nbins):
    """fixed [nzf, nyf, nxf]; moving [nframes, nzm, nym, nxm]; rng_f = (lo, hi, scale, n), rng_m one such per frame; jobs = [(frame,
    M float32 [4, 4] fixed voxel -> moving voxel)].  uint32 [njobs, nbins, nbins]."""
    fixed = np.asarray(fixed, F)
    moving = np.asarray(moving, F)
    outshape = fixed.shape[::-1]
    inshape = moving.shape[1:][::-1]
    fin = np.isfinite(fixed)
    ba, oka = bins(fixed, rng_f[0], rng_f[2], nbins)
    fin &= oka
    out = np.zeros((len(jobs), nbins, nbins), np.uint32)
    for j, (f, M) in enumerate(jobs):
        v = vref.vol_xform_ref(np.asarray(M, F), moving[f], inshape, outshape, "trilinear", F(np.nan))[0]
        bv, ok = bins(v, rng_m[f][0], rng_m[f][2], nbins)
        ok &= fin
        out[j] = np.bincount(ba[ok] * nbins + bv[ok], minlength=nbins * nbins).reshape(nbins, nbins).astype(np.uint32)
    return out


def reg_hist_loop(fixed, rng_f, frame, rng_m, M, nbins):
    """the same for one job, voxel by voxel in Python with a scalar binning of its own (the check of reg_hist and of bins)"""
    def bin1(x, lo, scale):
        with np.errstate(all="ignore"):
            t = F(F(F(x) - F(lo)) * F(scale))
        if math.isnan(t):
            return None
        return 0 if t < 0 else nbins - 1 if t >= nbins else int(math.floor(t))

    nzf, nyf, nxf = fixed.shape
    inshape = frame.shape[::-1]
    p = vref.pull_back(M, (nxf, nyf, nzf))
    ok = vref.inside_mask(p, inshape)
    v = vref.vol_xform_ref(np.asarray(M, F), frame, inshape, (nxf, nyf, nzf), "trilinear", F(0))[0]
    h = np.zeros((nbins, nbins), np.uint32)
    for k in range(nzf):
        for j in range(nyf):
            for i in range(nxf):
                a = fixed[k, j, i]
                if not np.isfinite(a) or not ok[k, j, i]:
                    continue
                bv, ba = bin1(v[k, j, i], rng_m[0], rng_m[2]), bin1(a, rng_f[0], rng_f[2])
                if bv is None or ba is None:
                    continue
                h[ba, bv] += 1
    return h


# ---- matrices ---------------------------------------------------------------------------------------------------------------------
def level_matrix(level):
    """D_l: level-l voxel x sits at level-0 voxel 2^l x + (2^l - 1) / 2"""
    D = np.eye(4)
    D[0, 0] = D[1, 1] = D[2, 2] = 2.0 ** level
    D[:3, 3] = (2.0 ** level - 1.0) / 2.0
    return D


def reg_G(theta, fixed_vox2ras, fixed_size):
    """G(theta) = C A C^-1, fixed RAS -> moving RAS, float64"""
    th = np.zeros(12)
    th[:len(theta)] = theta
    rx, ry, rz = np.deg2rad(th[3:6])
    Rx = np.array([[1, 0, 0], [0, math.cos(rx), -math.sin(rx)], [0, math.sin(rx), math.cos(rx)]])
    Ry = np.array([[math.cos(ry), 0, math.sin(ry)], [0, 1, 0], [-math.sin(ry), 0, math.cos(ry)]])
    Rz = np.array([[math.cos(rz), -math.sin(rz), 0], [math.sin(rz), math.cos(rz), 0], [0, 0, 1]])
    Sh = np.array([[1, th[9], th[10]], [0, 1, th[11]], [0, 0, 1]])
    S = np.diag(np.exp(th[6:9]))
    L = Rz @ Ry @ Rx @ Sh @ S
    V = np.asarray(fixed_vox2ras, F).astype(np.float64).reshape(4, 4)
    c = (V @ np.append((np.asarray(fixed_size, np.float64) - 1.0) / 2.0, 1.0))[:3]
    G = np.eye(4)
    G[:3, :3] = L
    G[:3, 3] = c + th[:3] - L @ c
    return G


def reg_matrix(theta, fixed_vox2ras, fixed_size, moving_vox2ras, level):
    """out2in of a level: float32(inv(V_mov D_l) G (V_fix D_l)), rounded once"""
    Vf = np.asarray(fixed_vox2ras, F).astype(np.float64).reshape(4, 4)
    Vm = np.asarray(moving_vox2ras, F).astype(np.float64).reshape(4, 4)
    D = level_matrix(level)
    return (np.linalg.inv(Vm @ D) @ reg_G(theta, fixed_vox2ras, fixed_size) @ (Vf @ D)).astype(F)


# ---- the cost ---------------------------------------------------------------------------------------------------------------------
def _entropy(c, N):
    c = [int(x) for x in np.asarray(c).reshape(-1) if x]
    return math.log(N) - math.fsum(x * math.log(x) for x in c) / N


def nmi(hist, nfinite, min_overlap=0.5):
    h = np.asarray(hist).astype(np.int64)
    N = int(h.sum())
    if N < min_overlap * nfinite or N == 0:
        return -math.inf
    hj = _entropy(h, N)
    if hj == 0:
        return -math.inf
    return (_entropy(h.sum(axis=1), N) + _entropy(h.sum(axis=0), N)) / hj


# ---- the driver -------------------------------------------------------------------------------------------------------------------
def level_sizes(size, levels):
    out = [tuple(int(v) for v in size)]
    for _ in range(levels - 1):
        out.append(tuple((n + 1) // 2 for n in out[-1]))
    return out


def default_levels(fixed_size, moving_size):
    """1 + the largest l <= 3 at which both volumes keep every dimension >= 8 (at least one level)"""
    n = 1
    for l in range(1, 4):
        if min(level_sizes(fixed_size, l + 1)[l] + level_sizes(moving_size, l + 1)[l]) >= 8:
            n = l + 1
    return n


def steps(level, dof, fixed_size, fixed_res):
    res = np.asarray(fixed_res, F).astype(np.float64)
    h = 2.0 ** level * float(res.min())
    s = 0.0
    for n, r in zip(fixed_size, res):
        s = s + (float(n) * float(r)) ** 2
    R = 0.5 * math.sqrt(s) / math.sqrt(3.0)
    st = np.zeros(12)
    st[:3] = h
    st[3:6] = (h / R) * (180.0 / math.pi)
    st[6:12] = h / R
    return st[:dof]


class Pyramid:
    """the levels of a fixed volume [nz, ny, nx] and a moving series [nframes, nz, ny, nx] with their ranges"""

    def __init__(self, fixed, moving, levels, nbins):
        self.fixed, self.moving = [np.asarray(fixed, F)], [np.asarray(moving, F)]
        for _ in range(levels - 1):
            self.fixed.append(halve(self.fixed[-1]))
            self.moving.append(np.stack([halve(m) for m in self.moving[-1]]))
        self.rng_f = [vol_range(f, nbins) for f in self.fixed]
        self.rng_m = [[vol_range(m, nbins) for m in ms] for ms in self.moving]
        self.nbins = nbins

    def costs(self, level, frame, mats, min_overlap=0.5):
        h = reg_hist(self.fixed[level], self.rng_f[level], self.moving[level], self.rng_m[level], [(frame, M) for M in mats], self.nbins)
        return [nmi(x, self.rng_f[level][3], min_overlap) for x in h]


def search(pyr, frame, fixed_geom, moving_vox2ras, dof=6, levels=1, halvings=4, maxit=80, min_overlap=0.5, theta0=None):
    """the pattern search: (theta float64 [dof], final cost, trace rows [niter, ROW], smallest relative gap between the two best of
    {current, candidates} over all iterations, theta at the end of the 6-parameter schedule).  fixed_geom = (size, res, vox2ras) of level 0."""
    size, res, Vf = fixed_geom
    theta = np.zeros(dof) if theta0 is None else np.array(theta0, np.float64)
    stages = [(l, 6) for l in range(levels - 1, -1, -1)] + ([(0, 12)] if dof == 12 else [])
    trace, gap, cur, rigid = [], math.inf, -math.inf, None
    for level, nd in stages:
        if nd == 12:
            rigid = theta.copy()
        def mat(th):
            return reg_matrix(th, Vf, size, moving_vox2ras, level)
        step = steps(level, nd, size, res)
        cur = pyr.costs(level, frame, [mat(theta)], min_overlap)[0]
        fails = it = 0
        while fails < halvings + 1 and it < maxit:
            cands = []
            for i in range(nd):
                for sg in (1.0, -1.0):
                    c = theta.copy()
                    c[i] = c[i] + sg * step[i]
                    cands.append(c)
            costs = pyr.costs(level, frame, [mat(c) for c in cands], min_overlap)
            best = int(np.argmax(costs))
            top = sorted([cur] + costs, reverse=True)[:2]
            if math.isfinite(top[0]):
                gap = min(gap, (top[0] - top[1]) / abs(top[0]) if math.isfinite(top[1]) else math.inf)
            row = [level, nd, best, 0, cur] + costs + [math.nan] * (24 - 2 * nd)
            if costs[best] > cur:
                theta, cur, row[3] = cands[best], costs[best], 1
            else:
                step = step / 2.0
                fails += 1
            trace.append(row)
            it += 1
    return theta, cur, np.array(trace, np.float64).reshape(-1, ROW), gap, (theta.copy() if rigid is None else rigid)


def xfm_matrices(theta, fixed_vox2ras, fixed_size, moving_vox2ras):
    """(ras2ras, vox2vox) of the result, moving -> fixed: float32(inv(G)), float32(inv(V_fix) inv(G) V_mov)"""
    Gi = np.linalg.inv(reg_G(theta, fixed_vox2ras, fixed_size))
    Vf = np.asarray(fixed_vox2ras, F).astype(np.float64).reshape(4, 4)
    Vm = np.asarray(moving_vox2ras, F).astype(np.float64).reshape(4, 4)
    return Gi.astype(F), (np.linalg.inv(Vf) @ Gi @ Vm).astype(F)


def voxrot(vox2vox):
    u, _, vt = np.linalg.svd(np.asarray(vox2vox, np.float64)[:3, :3])
    return u @ vt


def rotate_bvec(bvec, vox2vox):
    """bvec_out = voxrot(vox2vox) bvec in float64, rounded once; zero rows stay zero"""
    b = np.asarray(bvec, F).astype(np.float64).reshape(-1, 3)
    return (b @ voxrot(vox2vox).T).astype(F)


# ---- the phantom of the tests -----------------------------------------------------------------------------------------------------
BLOBS = (((9.0, 5.0, -4.0), 5.0, 0.9), ((-8.0, 7.0, 3.0), 4.0, -0.5), ((4.0, -9.0, 6.0), 6.0, 0.6),
         ((-6.0, -6.0, -7.0), 4.5, 0.8), ((11.0, -3.0, 2.0), 3.5, -0.4), ((-3.0, 10.0, -5.0), 5.5, 0.5))   # centre mm, sigma mm, weight
TRUE6 = (1.7, -1.1, 0.9, 3.0, -2.5, 4.0)
TRUE12 = TRUE6 + tuple(math.log(s) for s in (1.05, 0.96, 1.03)) + (0.03, -0.02, 0.025)


def phantom_at(ras, semi):
    """the phantom at RAS points [..., 3] (mm about the origin): a soft-edged ellipsoid of semi-axes `semi` plus six Gaussian blobs"""
    r = np.sqrt(((ras / np.asarray(semi, np.float64)) ** 2).sum(-1))
    v = 1.0 / (1.0 + np.exp((r - 1.0) * 8.0))
    for c, s, w in BLOBS:
        v = v + w * np.exp(-((ras - np.asarray(c)) ** 2).sum(-1) / (2.0 * s * s)) * (r < 1.0)
    return v


def geometry(size, res=2.0):
    """vox2ras of a grid of `size` voxels of `res` mm centred on the RAS origin"""
    V = np.eye(4)
    V[0, 0] = V[1, 1] = V[2, 2] = res
    V[:3, 3] = -res * (np.asarray(size, np.float64) - 1.0) / 2.0
    return V.astype(F)


def remap(v, kind=0):
    """a non-linear, non-monotone-free remap of intensities (another contrast)"""
    return np.sqrt(np.maximum(v, 0.0)) * 700.0 + 40.0 * v * v if kind == 0 else 900.0 * np.exp(-1.3 * v) + 15.0 * v


def phantom_pair(size, theta_true, kind=0):
    """(fixed [nz, ny, nx], moving [nz, ny, nx], vox2ras): the moving image is the remapped phantom pulled back through G(theta_true)"""
    nx, ny, nz = size
    V = geometry(size)
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    ras = np.stack([i, j, k, np.ones_like(i)], -1).astype(np.float64) @ V.astype(np.float64).T
    semi = tuple(0.40 * 2.0 * n for n in size)
    fixed = (1000.0 * phantom_at(ras[..., :3], semi)).astype(F)
    Gi = np.linalg.inv(reg_G(np.asarray(theta_true, np.float64), V, size))
    moving = remap(phantom_at((ras @ Gi.T)[..., :3], semi), kind).astype(F)
    return fixed, moving, V


def residual_mm(theta, theta_true, size, V):
    """|G(theta) x - G(theta_true) x| in mm at every fixed voxel: (max, mean)"""
    nx, ny, nz = size
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    ras = np.stack([i, j, k, np.ones_like(i)], -1).astype(np.float64) @ np.asarray(V, np.float64).T
    d = ras @ (reg_G(theta, V, size) - reg_G(np.asarray(theta_true, np.float64), V, size)).T
    n = np.sqrt((d[..., :3] ** 2).sum(-1))
    return float(n.max()), float(n.mean())


CASES = {"28": ((28, 24, 20), 1, 6), "27": ((27, 23, 19), 1, 6), "41": ((41, 36, 29), 2, 6), "41x12": ((41, 36, 29), 2, 12)}


@functools.lru_cache(maxsize=None)
def case(name, nbins=32):
    """a driver case, computed once: dict(size, levels, dof, fixed, moving, V, true, theta, cost, trace, gap, rigid)"""
    size, levels, dof = CASES[name]
    true = TRUE12 if dof == 12 else TRUE6
    fixed, moving, V = phantom_pair(size, true)
    pyr = Pyramid(fixed, moving[None], levels, nbins)
    theta, cost, trace, gap, rigid = search(pyr, 0, (size, (2.0, 2.0, 2.0), V), V, dof=dof, levels=levels)
    return dict(size=size, levels=levels, dof=dof, fixed=fixed, moving=moving, V=V, true=true, theta=theta, cost=cost, trace=trace, gap=gap,
                rigid=rigid)


# ---- the histogram cases of the GPU tests -------------------------------------------------------------------------------------------
def hist_volumes(fshape, mshape, nframes, seed):
    """smooth-ish volumes with NaN voxels in both, an Inf in the moving series: (fixed [nz, ny, nx], moving [nframes, nz, ny, nx])"""
    rng = np.random.default_rng(seed)
    fixed = rng.normal(100, 30, fshape[::-1]).astype(F)
    moving = (rng.normal(-5, 2, (nframes,) + tuple(mshape[::-1])) * np.linspace(1, 3, nframes)[:, None, None, None]).astype(F)
    if fixed.size > 20:
        fixed.reshape(-1)[[5, fixed.size // 2]] = np.nan
        moving.reshape(-1)[[7, moving.size // 3]] = np.nan
        moving.reshape(-1)[moving.size // 2] = np.inf
    return fixed, moving


def hist_jobs(njobs, nframes, M0, projective=False):
    """njobs (frame, matrix) pairs around M0: a frame map that is neither monotone nor injective, matrices shifted job by job"""
    jobs = []
    for j in range(njobs):
        M = np.array(M0, F).reshape(4, 4).copy()
        M[:3, 3] += F(0.37) * F(j) * np.array([1, -1, 0.5], F)
        if projective and j % 2:
            M[3, :3] = (F(0.004), F(-0.003), F(0.002))
        jobs.append(((2, 0, 2, 1, 0, 0, 2, 1, 1, 0, 2, 2, 1)[j % 13] % nframes, M))
    return jobs
