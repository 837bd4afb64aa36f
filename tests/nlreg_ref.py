"""NumPy restatement of the non-linear registration contract ("Non-linear registration", include/fibers_hip.h), independent of the
package: the matrices of a level, the normalised values, one demons iteration (moving sample, fixed gradient, force, cost), the
Gaussian regularisation, the step between levels, the whole pyramid and the Jacobian map.  float32 element-wise, every multiply, add
and divide rounded on its own, in the contract's order; the matrices and the taps are float64 rounded once.  Built on warp_ref.sample
/ warp_ref.xfm_point / warp_ref.warp_volume (the field sample and the warp of a volume), volxform_ref (the sampler) and register_ref
(halve, vol_range, level_matrix).  Volumes are [nz, ny, nx] (x fastest), fields [3, nz, ny, nx], shapes (nx, ny, nz).  `mutant`
switches in one deliberate error, for the tests of the tests (tests/test_nlreg_ref.py)."""
import math

import numpy as np

import register_ref as R
import warp_ref as W

F = np.float32
MUTANTS = ("zero_fill", "taps_from_plus_r", "diff_sign", "central_faces", "fma")
_SAMPLE_MUTANT = {"zero_fill": "zero_outside", "fma": "fma"}      # what a mutant means inside warp_ref.sample


def _f64(m):
    return np.eye(4) if m is None else np.asarray(m, F).astype(np.float64).reshape(4, 4)


# ---- what a level needs -----------------------------------------------------------------------------------------------------------
def level_matrices(fixed_v2r, moving_v2r, post, level, step):
    """(to_ras float32 [4, 4], from_ras float32 [4, 4], T float32 [3, 3], kappa float32): float32(V_fix D_l),
    float32(inv(V_mov D_l) post), float32(inv(L)^T) with L the linear part of V_fix D_l, float32(1 / (2^l step)^2)"""
    D = R.level_matrix(level)
    Vf, Vm = _f64(fixed_v2r) @ D, _f64(moving_v2r) @ D
    ell = 2.0 ** level * float(F(step))
    return Vf.astype(F), (np.linalg.inv(Vm) @ _f64(post)).astype(F), np.linalg.inv(Vf[:3, :3]).T.astype(F), F(1.0 / (ell * ell))


def norm_of(vol):
    """(lo, s) of a level volume: lo, hi by fibd_vol_range's rule, s = float32(1) / (hi - lo); a volume without two distinct finite
    values is refused"""
    lo, hi, _, n = R.vol_range(vol, 8)
    if n == 0 or hi == lo:
        raise ValueError("constant volume")
    with np.errstate(all="ignore"):
        return F(lo), F(F(1) / F(F(hi) - F(lo)))


def normalise(v, lo, s):
    with np.errstate(all="ignore"):
        return ((np.asarray(v, F) - F(lo)).astype(F) * F(s)).astype(F)


def dif(a, axis, mutant=None):
    """the difference rule along `axis` of an array: central in the interior, one-sided on the two faces, 0 on an axis of size 1"""
    a = np.moveaxis(np.asarray(a, F), axis, 0)
    out = np.zeros(a.shape, F)
    if a.shape[0] > 1:
        with np.errstate(all="ignore"):
            out[1:-1] = ((a[2:] - a[:-2]).astype(F) * F(0.5)).astype(F)
            out[0], out[-1] = a[1] - a[0], a[-1] - a[-2]
            if mutant == "central_faces":                          # the central formula on the clamped neighbours
                out[0], out[-1] = ((a[1] - a[0]).astype(F) * F(0.5)).astype(F), ((a[-1] - a[-2]).astype(F) * F(0.5)).astype(F)
    return np.moveaxis(out, 0, axis)


# ---- one iteration ----------------------------------------------------------------------------------------------------------------
def moving_sample(field, to_ras, from_ras, moving, mutant=None):
    """the value fibd_warp_volume gives at every fixed voxel (to_field the identity); NaN where the sample is absent"""
    nz, ny, nx = field.shape[1:]
    mov = np.ascontiguousarray(moving, F)
    return W.warp_volume(field, to_ras, np.eye(4, dtype=F), from_ras, mov[None], mov.shape[::-1], (nx, ny, nz), "trilinear", F(np.nan),
                         mutant=_SAMPLE_MUTANT.get(mutant))[0]


def step(fixed, moving, norm, mats, field, mutant=None):
    """steps 1-5: (d' [3, nz, ny, nx], ssd: the exact sum of the float32 squares as a float, count)"""
    to_ras, from_ras, T, kappa = mats
    lo_f, s_f, lo_m, s_m = norm
    field = np.asarray(field, F)
    with np.errstate(all="ignore"):
        # an absent sample and a non-finite one both give u = 0 and are not counted: NaN stands for both
        m = normalise(moving_sample(field, to_ras, from_ras, moving, mutant), lo_m, s_m)
        f = normalise(fixed, lo_f, s_f)
        v = [dif(f, 2, mutant), dif(f, 1, mutant), dif(f, 0, mutant)]                  # voxel axes x, y, z
        g = [((T[c, 0] * v[0] + T[c, 1] * v[1]).astype(F) + T[c, 2] * v[2]).astype(F) for c in range(3)]
        diff = (m - f).astype(F) if mutant == "diff_sign" else (f - m).astype(F)
        sq = (diff * diff).astype(F)
        den = (((g[0] * g[0] + g[1] * g[1]).astype(F) + g[2] * g[2]).astype(F) + (sq * F(kappa)).astype(F)).astype(F)
        ok = np.isfinite(f) & np.isfinite(m) & np.isfinite(g[0]) & np.isfinite(g[1]) & np.isfinite(g[2]) & np.isfinite(den) & (den != 0)
        q = np.where(ok, (diff / np.where(ok, den, F(1))).astype(F), F(0))
        out = np.stack([(field[c] + np.where(ok, (q * g[c]).astype(F), F(0))).astype(F) for c in range(3)])
    ssd = math.fsum(sq[ok].astype(np.float64).tolist())
    return out, ssd, int(ok.sum())


def ssd_bound(ssd, count):
    """|sum in any order - exact sum| <= count 2^-53 sum of the (non-negative) terms"""
    return count * 2.0 ** -53 * ssd


# ---- regularisation ---------------------------------------------------------------------------------------------------------------
def taps(sigma):
    """(r, w float32 [2 r + 1]): r = ceil(3 sigma), w_t = float32(exp(-t^2 / (2 sigma^2)) / sum), the sum added for t = -r .. r"""
    s = float(F(sigma))
    r = int(math.ceil(3.0 * s))
    if r == 0:
        return 0, np.ones(1, F)
    e = [math.exp(-(float(t) * float(t)) / (2.0 * s * s)) for t in range(-r, r + 1)]
    tot = 0.0
    for x in e:
        tot += x
    return r, np.array([x / tot for x in e], np.float64).astype(F)


def smooth(field, sigma, mutant=None):
    """step 6: the x pass over the whole field, then y, then z; acc = +0, then acc + w_t v[clamp(i + t)] for t = -r .. r"""
    field = np.array(field, F)
    if float(sigma) == 0.0:
        return field
    r, w = taps(sigma)
    order = range(r, -r - 1, -1) if mutant == "taps_from_plus_r" else range(-r, r + 1)
    with np.errstate(all="ignore"):
        for axis in (3, 2, 1):
            n = field.shape[axis]
            acc = np.zeros(field.shape, F)
            for t in order:
                at = np.arange(n) + t
                v = np.take(field, np.clip(at, 0, n - 1), axis=axis)
                if mutant == "zero_fill":
                    shape = [1, 1, 1, 1]
                    shape[axis] = n
                    v = np.where(((at < 0) | (at > n - 1)).reshape(shape), F(0), v)
                acc = (acc + (w[t + r] * v).astype(F)).astype(F)
            field = acc
    return field


# ---- between levels ---------------------------------------------------------------------------------------------------------------
def upsample(coarse, shape, mutant=None):
    """fine voxel y takes S(0.5 y - 0.25) of the coarse field; shape = (nx, ny, nz) of the fine grid"""
    nx, ny, nz = shape
    q = (F(0.5) * W.grid_points(shape) - F(0.25)).astype(F)
    s = W.sample(np.asarray(coarse, F), q, F, _SAMPLE_MUTANT.get(mutant))
    return np.ascontiguousarray(s.T).reshape(3, nz, ny, nx)


def level_sizes(shape, levels):
    out = [tuple(int(n) for n in shape)]
    for _ in range(1, levels):
        out.append(tuple((n + 1) // 2 for n in out[-1]))
    return out


def niter_list(niter, levels):
    return [int(niter)] * levels if np.isscalar(niter) else [int(n) for n in niter]


def run(fixed, fixed_v2r, moving, moving_v2r, post=None, levels=None, niter=30, sigma=1.0, step_mm=None, mutant=None):
    """the whole pyramid: (field [3, nz, ny, nx], cost [levels, max niter], count, ssd) with rows from the coarsest level; `ssd` are the
    exact sums behind the costs (for the bound)"""
    fixed, moving = np.asarray(fixed, F), np.asarray(moving, F)
    if levels is None:
        levels = R.default_levels(fixed.shape[::-1], moving.shape[::-1])
    n = niter_list(niter, levels)
    assert len(n) == levels
    if step_mm is None:
        step_mm = float(np.sqrt((_f64(fixed_v2r)[:3, :3] ** 2).sum(axis=0)).min())
    fp, mp = [fixed], [moving]
    for _ in range(1, levels):
        fp.append(R.halve(fp[-1]))
        mp.append(R.halve(mp[-1]))
    norms = [norm_of(fp[l]) + norm_of(mp[l]) for l in range(levels)]
    width = max(1, max(n))
    cost, ssd, count = np.full((levels, width), np.nan), np.zeros((levels, width)), np.zeros((levels, width), np.int64)
    field = None
    for row, l in enumerate(range(levels - 1, -1, -1)):
        shape = fp[l].shape[::-1]
        field = np.zeros((3,) + fp[l].shape, F) if field is None else upsample(field, shape, mutant)
        mats = level_matrices(fixed_v2r, moving_v2r, post, l, step_mm)
        for it in range(n[row]):
            field, s, c = step(fp[l], mp[l], norms[l], mats, field, mutant)
            ssd[row, it], count[row, it] = s, c
            cost[row, it] = s / c if c else np.nan
            field = smooth(field, sigma, mutant)
    return field, cost, count, ssd


def warped(field, fixed_v2r, moving, moving_v2r, post=None):
    """the moving volume through the final field onto the fixed grid: mri_warp(warp, moving, outref=fixed, post=post), 0 outside"""
    nz, ny, nx = field.shape[1:]
    mov = np.ascontiguousarray(moving, F)
    A, Q, B = W.volume_matrices(fixed_v2r, fixed_v2r, moving_v2r, None, post)
    return W.warp_volume(field, A, Q, B, mov[None], mov.shape[::-1], (nx, ny, nz), "trilinear", F(0))[0]


# ---- the Jacobian map -------------------------------------------------------------------------------------------------------------
def jacobian_matrix(field_v2r):
    return np.linalg.inv(_f64(field_v2r)[:3, :3]).astype(F)


def jacobian(field, field_v2r, mutant=None):
    """det(I + dd/dx) [nz, ny, nx]: D[c][k] by the difference rule, G = D Linv in k order, the cofactor expansion along the first row"""
    field = np.asarray(field, F)
    Li = jacobian_matrix(field_v2r)
    with np.errstate(all="ignore"):
        D = [[dif(field[c], 2 - k, mutant) for k in range(3)] for c in range(3)]
        J = [[None] * 3 for _ in range(3)]
        for c in range(3):
            for r in range(3):
                g = ((D[c][0] * Li[0, r] + D[c][1] * Li[1, r]).astype(F) + D[c][2] * Li[2, r]).astype(F)
                J[c][r] = (F(1) + g).astype(F) if c == r else g
        m0 = (J[1][1] * J[2][2] - J[1][2] * J[2][1]).astype(F)
        m1 = (J[1][0] * J[2][2] - J[1][2] * J[2][0]).astype(F)
        m2 = (J[1][0] * J[2][1] - J[1][1] * J[2][0]).astype(F)
        return ((J[0][0] * m0 - J[0][1] * m1).astype(F) + J[0][2] * m2).astype(F)


# ---- the tests' volumes -------------------------------------------------------------------------------------------------------------
def scene(ras, box, seed=0):
    """a smooth positive scene at RAS points [..., 3]: five Gaussian blobs inside `box` = (lo, hi) plus a ramp along x, float32"""
    lo, hi = (np.asarray(b, np.float64) for b in box)
    rng = np.random.default_rng(seed)
    v = 0.1 * (ras[..., 0] - lo[0]) / (hi[0] - lo[0])
    for _ in range(5):
        c = lo + rng.uniform(0.2, 0.8, 3) * (hi - lo)
        w = rng.uniform(0.15, 0.3) * (hi - lo).min()
        v = v + rng.uniform(0.5, 1.0) * np.exp(-((ras - c) ** 2).sum(axis=-1) / (2 * w * w))
    return (100.0 * v).astype(F)


def pair(fshape=(20, 17, 13), mshape=(18, 19, 15), fres=(2.0, 2.0, 2.0), mres=(2.1, 1.9, 2.0), seed=0, amp=1.2):
    """the tests' main case: (fixed, fixed_v2r, moving, moving_v2r), two oblique grids over one scene; the moving volume sees the scene
    through a smooth displacement of `amp` mm"""
    Vf = W.oblique_vox2ras(fres)
    Vm = W.oblique_vox2ras(mres, angles_deg=(17.0, 12.0), origin=(-6.0, 4.0, -5.0))
    rf, rm = W.node_ras(Vf, fshape), W.node_ras(Vm, mshape)
    box = (rf.reshape(-1, 3).min(axis=0), rf.reshape(-1, 3).max(axis=0))
    d = amp * np.stack([np.sin(rm[..., 1] / 6 + 0.3), 0.8 * np.cos(rm[..., 2] / 7), 0.6 * np.sin((rm[..., 0] + rm[..., 1]) / 8)], axis=-1)
    return scene(rf, box, seed), Vf, scene(rm + d, box, seed), Vm


def rigid(deg=5.0, shift=(0.8, -0.5, 0.3)):
    """a rigid fixed RAS -> moving RAS matrix, float32 [4, 4]: `deg` degrees about z and a shift in mm"""
    a = np.deg2rad(deg)
    M = np.eye(4)
    M[:3, :3] = [[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]
    M[:3, 3] = shift
    return M.astype(F)
