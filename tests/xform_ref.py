"""NumPy restatement of the reference's transform layer, written from util.jl:126-454 and trk.jl:275-347 only (the way
st_recon_ref.py restates structens.jl).  Tests hold the package's `Xform` functions and the HIP kernels to it.

- apply_f32: xfm_apply!'s loop (util.jl:401-420) in float32, one rounding per multiply and per add, in the reference's order.
- apply_fma: the same loop as a compiler that contracts a*b+c into fma would evaluate it (used to show that a test can tell the two
  apart).
- lta_vox2ras / derive_lta: the float64 derivation of xfm_read(ltafile) (util.jl:228-262).
- str_xform / str_merge: trk.jl:316-347 and 275-308 on this package's packed `Tract`."""
import numpy as np


def apply_f32(m, pts):
    """xfm_apply(xfm, point) for float32 points [N, 3] (or 3N): out_aff, then per row out_lin / out_aff"""
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):       # (non-finite points give NaN, as in the reference)
        return _apply_f32(m, pts)


def _apply_f32(m, pts):
    m = np.asarray(m, np.float32)
    p = np.asarray(pts, np.float32).reshape(-1, 3)
    aff = np.zeros(p.shape[0], np.float32)
    for j in range(3):
        aff = aff + m[3, j] * p[:, j]
    aff = aff + m[3, 3]
    out = np.empty_like(p)
    for i in range(3):
        lin = np.zeros(p.shape[0], np.float32)
        for j in range(3):
            lin = lin + m[i, j] * p[:, j]
        lin = lin + m[i, 3]
        out[:, i] = lin / aff
    return out.reshape(np.shape(pts))


def _fma32(a, b, c):
    """float32 fma: a*b is exact in float64; the sum is rounded to float64 and then to float32 (a double rounding that can only
    matter in ties, which apply_fma's callers do not rely on)"""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def apply_fma(m, pts):
    m = np.asarray(m, np.float32)
    p = np.asarray(pts, np.float32).reshape(-1, 3)
    aff = np.zeros(p.shape[0], np.float32)
    for j in range(3):
        aff = _fma32(m[3, j], p[:, j], aff)
    aff = aff + m[3, 3]
    out = np.empty_like(p)
    for i in range(3):
        lin = np.zeros(p.shape[0], np.float32)
        for j in range(3):
            lin = _fma32(m[i, j], p[:, j], lin)
        lin = lin + m[i, 3]
        out[:, i] = lin / aff
    return out.reshape(np.shape(pts))


def lta_vox2ras(size, res, xras, yras, zras, cras):
    """float64 [xras*r1 yras*r2 zras*r3 | cras - M*size/2] (util.jl:228-248)"""
    M = np.stack([np.asarray(xras, np.float64) * res[0], np.asarray(yras, np.float64) * res[1],
                  np.asarray(zras, np.float64) * res[2]], axis=1)
    out = np.eye(4)
    out[:3, :3] = M
    out[:3, 3] = np.asarray(cras, np.float64) - M @ np.asarray(size, np.float64) / 2
    return out


def derive_lta(regtype, regmat, src, dst):
    """(invox2ras, outvox2ras, vox2vox, ras2ras) in float64 (util.jl:250-262); src / dst: dicts of size, res, xras, yras, zras, cras"""
    A = lta_vox2ras(src["size"], src["res"], src["xras"], src["yras"], src["zras"], src["cras"])
    B = lta_vox2ras(dst["size"], dst["res"], dst["xras"], dst["yras"], dst["zras"], dst["cras"])
    R = np.asarray(regmat, np.float64)
    if regtype == 0:
        return A, B, R, B @ R @ np.linalg.inv(A)
    return A, B, np.linalg.inv(B) @ R @ A, R


def str_xform(xfm, tr):
    """trk.jl:316-347 on a packed Tract: new geometry, points through apply_f32, every other field carried over"""
    import dataclasses
    return dataclasses.replace(tr, xyz=apply_f32(xfm.vox2vox, tr.xyz), volsize=tuple(int(v) for v in xfm.outsize),
                               volres=tuple(float(v) for v in xfm.outres), vox2ras=np.asarray(xfm.outvox2ras, np.float32).copy())


def str_merge(*trs):
    """trk.jl:275-308: counts, points, scalars and properties back to back (header checks are the package's to test)"""
    xyz = np.concatenate([t.xyz for t in trs])
    npts = np.concatenate([t.npts for t in trs])
    sc = None if trs[0].scalars is None else np.concatenate([t.scalars for t in trs])
    pr = None if trs[0].properties is None else np.concatenate([t.properties for t in trs])
    return xyz, npts, sc, pr
