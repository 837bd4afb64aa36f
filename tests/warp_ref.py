"""NumPy restatement of the non-linear warp contract ("Non-linear warps", include/fibers_hip.h), independent of the package: the
sample S(q), the warp of a point, the warp of a volume (on volxform_ref's sampler), the fixed-point inverse, the matrices of str_warp /
mri_warp and the LPS -> RAS rule of the ITK vector image.  Element-wise in the float type `ft` (float32: every multiply and add rounded
on its own, in the contract's order; float64 for a run of the same arithmetic at higher precision).  A field is [3, nz, ny, nx] (the
planar layout of the C ABI, C-ordered here); points are [N, 3].  `mutant` switches in one deliberate error, for the tests of the tests
(tests/test_warp_ref.py)."""
import numpy as np

import volxform_ref as V

F = np.float32
MUTANTS = ("fma", "clamp_after_floor", "zero_outside", "lps_sign", "origin_ignored")


def xfm_point(m, p, ft=F):
    """xfm_point (csrc/xfm_apply.inc): aff, then per row lin / aff"""
    m = np.asarray(m, ft).reshape(4, 4)
    p = np.asarray(p, ft).reshape(-1, 3)
    with np.errstate(all="ignore"):
        aff = ft(0) + m[3, 0] * p[:, 0]
        aff = aff + m[3, 1] * p[:, 1]
        aff = aff + m[3, 2] * p[:, 2]
        aff = aff + m[3, 3]
        out = np.empty(p.shape, ft)
        for r in range(3):
            lin = ft(0) + m[r, 0] * p[:, 0]
            lin = lin + m[r, 1] * p[:, 1]
            lin = lin + m[r, 2] * p[:, 2]
            lin = lin + m[r, 3]
            out[:, r] = lin / aff
    return out


def _lerp(g, a, f, b, ft, mutant):
    """g*a + f*b, each operation rounded (mutant "fma": the sum contracts the second product)"""
    if mutant == "fma" and ft == F:
        return (np.asarray(f, np.float64) * np.asarray(b, np.float64) + np.asarray(g * a, np.float64)).astype(F)
    return g * a + f * b


def sample(field, q, ft=F, mutant=None):
    """S(q) for q [N, 3] in field-voxel coordinates -> [N, 3]"""
    field = np.asarray(field, ft)
    nz, ny, nx = field.shape[1:]
    q = np.asarray(q, ft).reshape(-1, 3)
    nan = np.isnan(q).any(axis=1)
    lo, hi, fr, gr = [], [], [], []
    out_of_grid = np.zeros(q.shape[0], bool)
    with np.errstate(all="ignore"):
        for c, n in enumerate((nx, ny, nz)):
            qq = np.where(nan, ft(0), q[:, c])
            top = ft(n - 1)
            out_of_grid |= (qq < 0) | (qq > top)
            if mutant == "clamp_after_floor":
                fl = np.floor(qq)
                f = (qq - fl).astype(ft)
                i0 = np.clip(np.nan_to_num(fl, posinf=1e9, neginf=-1e9), 0, n - 1).astype(np.int64)
            else:
                qc = np.where(qq < 0, ft(0), np.where(qq > top, top, qq)).astype(ft)
                fl = np.floor(qc)
                f = (qc - fl).astype(ft)
                i0 = fl.astype(np.int64)
            lo.append(i0)
            hi.append(np.minimum(i0 + 1, n - 1))
            fr.append(f)
            gr.append((ft(1) - f).astype(ft))
        (x0, y0, z0), (x1, y1, z1), (fx, fy, fz), (gx, gy, gz) = lo, hi, fr, gr
        out = np.empty(q.shape, ft)
        for c in range(3):
            a = field[c]
            c00 = _lerp(gx, a[z0, y0, x0], fx, a[z0, y0, x1], ft, mutant)
            c10 = _lerp(gx, a[z0, y1, x0], fx, a[z0, y1, x1], ft, mutant)
            c01 = _lerp(gx, a[z1, y0, x0], fx, a[z1, y0, x1], ft, mutant)
            c11 = _lerp(gx, a[z1, y1, x0], fx, a[z1, y1, x1], ft, mutant)
            c0 = _lerp(gy, c00, fy, c10, ft, mutant)
            c1 = _lerp(gy, c01, fy, c11, ft, mutant)
            out[:, c] = _lerp(gz, c0, fz, c1, ft, mutant)
    if mutant == "zero_outside":
        out[out_of_grid] = 0
    out[nan] = np.nan
    return out


def warp_points(field, to_ras, to_field, from_ras, p, ft=F, mutant=None, parts=False):
    """p' = xfm_point(from_ras, xfm_point(to_ras, p) + S(xfm_point(to_field, p))); parts=True also returns (x, q, y)"""
    shape = np.shape(p)
    x = xfm_point(to_ras, p, ft)
    q = xfm_point(to_field, p, ft)
    with np.errstate(all="ignore"):
        y = (x + sample(field, q, ft, mutant)).astype(ft)
    out = xfm_point(from_ras, y, ft).reshape(shape)
    return (out, x, q, y) if parts else out


def grid_points(shape, ft=F):
    """the voxel indices (i, j, k) of a grid of `shape` = (nx, ny, nz) as floats, [nz*ny*nx, 3], x fastest"""
    nx, ny, nz = shape
    k, j, i = np.meshgrid(np.arange(nz, dtype=ft), np.arange(ny, dtype=ft), np.arange(nx, dtype=ft), indexing="ij")
    return np.stack([i.ravel(), j.ravel(), k.ravel()], axis=1)


def warp_volume(field, to_ras, to_field, from_ras, vol, inshape, outshape, interp, outside, mutant=None):
    """vol [nframes, nzi, nyi, nxi] sampled at the warp of every output voxel by volxform_ref's sampler (vol_xform_ref with its
    pull-back replaced by the warped positions) -> [nframes, nzo, nyo, nxo]"""
    nxo, nyo, nzo = outshape
    pw = warp_points(field, to_ras, to_field, from_ras, grid_points(outshape), F, mutant)
    p = [np.ascontiguousarray(pw[:, c]).reshape(nzo, nyo, nxo) for c in range(3)]
    saved = V.pull_back
    V.pull_back = lambda M, shape: p
    try:
        return V.vol_xform_ref(None, vol, inshape, outshape, interp, outside)
    finally:
        V.pull_back = saved


def invert(field, out_to_ras, ras_to_field, outshape, niter, ft=F, mutant=None):
    """(inv [3, nzo, nyo, nxo], err [nzo, nyo, nxo]): x <- y - S(x) niter times from x = y = xfm_point(out_to_ras, voxel)"""
    nxo, nyo, nzo = outshape
    y = xfm_point(out_to_ras, grid_points(outshape, ft), ft)
    x = y.copy()
    with np.errstate(all="ignore"):
        for _ in range(niter):
            x = (y - sample(field, xfm_point(ras_to_field, x, ft), ft, mutant)).astype(ft)
        inv = (x - y).astype(ft)
        r = ((x + sample(field, xfm_point(ras_to_field, x, ft), ft, mutant)).astype(ft) - y).astype(ft)
        err = np.abs(r).max(axis=1)                                  # (np.max propagates NaN)
    return np.ascontiguousarray(inv.T).reshape(3, nzo, nyo, nxo), err.reshape(nzo, nyo, nxo)


# ---- the matrices of the Python layer, restated ----------------------------------------------------------------------------------------
def _f64(m):
    return np.eye(4) if m is None else np.asarray(m, F).astype(np.float64).reshape(4, 4)


def shift(v):
    T = np.eye(4)
    T[:3, 3] = v
    return T


def point_matrices(field_v2r, in_v2r, out_v2r, pre=None, post=None, origin=1, ft=F, mutant=None):
    """str_warp's (to_ras, to_field, from_ras): float64 products of the float32 fields, rounded once to `ft`; pre / post are ras2ras
    matrices or None"""
    to_ras = _f64(pre) @ _f64(in_v2r) @ shift(-float(origin))
    to_field = np.linalg.inv(_f64(field_v2r)) @ to_ras
    from_ras = np.linalg.inv(_f64(out_v2r)) @ _f64(post)
    if mutant != "origin_ignored":
        from_ras = shift(float(origin)) @ from_ras
    return to_ras.astype(ft), to_field.astype(ft), from_ras.astype(ft)


def volume_matrices(field_v2r, out_v2r, in_v2r, pre=None, post=None, ft=F):
    """mri_warp's (to_ras, to_field, from_ras)"""
    to_ras = _f64(pre) @ _f64(out_v2r)
    return to_ras.astype(ft), (np.linalg.inv(_f64(field_v2r)) @ to_ras).astype(ft), (np.linalg.inv(_f64(in_v2r)) @ _f64(post)).astype(ft)


def invert_matrices(field_v2r, out_v2r, ft=F):
    return _f64(out_v2r).astype(ft), np.linalg.inv(_f64(field_v2r)).astype(ft)


def lps_to_ras(vol, mutant=None):
    """[..., 3] components in LPS -> RAS: frames 0 and 1 negated"""
    out = np.array(vol, F)
    out[..., 0] = -out[..., 0]
    if mutant != "lps_sign":
        out[..., 1] = -out[..., 1]
    return out


# ---- the tests' geometry and fields ----------------------------------------------------------------------------------------------------
def oblique_vox2ras(res, angles_deg=(20.0, 10.0), origin=(-7.0, 5.5, -4.0)):
    """an oblique vox2ras: rotations about z and x, voxel sizes `res`, a shift"""
    az, ax = np.deg2rad(angles_deg[0]), np.deg2rad(angles_deg[1])
    Rz = np.array([[np.cos(az), -np.sin(az), 0], [np.sin(az), np.cos(az), 0], [0, 0, 1]])
    Rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
    A = np.eye(4)
    A[:3, :3] = (Rz @ Rx) * np.asarray(res, np.float64)
    A[:3, 3] = origin
    return A.astype(F)


def node_ras(v2r, shape):
    """float64 RAS coordinates of the nodes of a grid, [nz, ny, nx, 3]"""
    nx, ny, nz = shape
    g = grid_points(shape, np.float64)
    return (g @ _f64(v2r)[:3, :3].T + _f64(v2r)[:3, 3]).reshape(nz, ny, nx, 3)


def affine_field(v2r, shape, L, t):
    """d = (L - I) x + t at the grid nodes, float32 [3, nz, ny, nx] (and the float64 values it was rounded from)"""
    x = node_ras(v2r, shape)
    d = x @ (np.asarray(L, np.float64) - np.eye(3)).T + np.asarray(t, np.float64)
    d = np.ascontiguousarray(np.moveaxis(d, 3, 0))
    return d.astype(F), d


def smooth_field(v2r, shape, amp):
    """amp * (sin(y/6 + 0.3), 0.8 cos(z/7), 0.6 sin((x + y)/8)) mm at the grid nodes, float32 [3, nz, ny, nx]"""
    r = node_ras(v2r, shape)
    x, y, z = r[..., 0], r[..., 1], r[..., 2]
    return (amp * np.stack([np.sin(y / 6 + 0.3), 0.8 * np.cos(z / 7), 0.6 * np.sin((x + y) / 8)])).astype(F)


def ulp32(v):
    """the spacing of float32 at magnitude v"""
    return float(np.spacing(F(abs(v))))
