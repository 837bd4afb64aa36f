"""A NumPy restatement of dti_fit / adc_fit (dti.jl:164-335) in a precision of the caller's choice (TEST INFRASTRUCTURE, NumPy only).

The design matrix is built in Float32 as the reference builds it (dti.jl:131-140, dti.jl:68-69) and then cast; everything after it
-- the pseudo-inverse, the logarithms, the fit, the eigen-decomposition (LAPACK's `eigh`, not the closed form) and dti_maps -- runs
in `dtype`.  With float64 this is what the float32 kernels and the float32 oracle are measured against.

Branch selection is the reference's (dti.jl:291-303): `ipos = s .> 0` (false for NaN and -Inf, true for +Inf and for denormals);
npos == nvol -> pinv(A) * log.(s); npos > 6 && any(ipos[ib0]) -> pinv(A[ipos, :]) * log.(s[ipos]) with LinearAlgebra.pinv's
rtol = eps(Float32) * min(m, n); anything else -> zeros.  The row-subset fit is vectorised: the non-positive rows of A and the
matching logarithms are set to zero, which leaves the singular values, the cut-off and the solution of the subset unchanged
(pinv([A_sub; 0]) = [pinv(A_sub), 0]); tests/test_dti_ref.py proves that against an explicit per-voxel pinv.

Volumes are [..., nvol] with a mask [...]; the samples are used as given (float32 from the kernels' inputs; float64 for the
known-answer tests, where rounding the samples to float32 would cost 6e-8)."""
import numpy as np

EPS32 = float(np.finfo(np.float32).eps)
OUTSIDE, FULL, SUBSET, ZEROS = 0, 1, 2, 3                      # per-voxel branch codes
FIELDS = ("s0", "eigval1", "eigval2", "eigval3", "eigvec1", "eigvec2", "eigvec3", "rd", "md", "fa")


def design_dti(bval, bvec):
    """A [nvol, 7] in Float32 (dti.jl:131-140)"""
    f32 = np.float32
    bval = np.asarray(bval, f32).reshape(-1)
    g = np.asarray(bvec, f32).reshape(-1, 3)
    A = np.empty((bval.shape[0], 7), f32)
    A[:, 0] = g[:, 0] ** 2
    A[:, 1] = f32(2) * g[:, 0] * g[:, 1]
    A[:, 2] = f32(2) * g[:, 0] * g[:, 2]
    A[:, 3] = g[:, 1] ** 2
    A[:, 4] = f32(2) * g[:, 1] * g[:, 2]
    A[:, 5] = g[:, 2] ** 2
    A[:, :6] *= -bval[:, None]
    A[:, 6] = 1
    return A


def design_adc(bval):
    """A [nvol, 2] in Float32 (dti.jl:68-69)"""
    bval = np.asarray(bval, np.float32).reshape(-1)
    return np.stack([-bval, np.ones_like(bval)], axis=1)


def random_tensors(evals, n, rng):
    """n tensors with the eigenvalues `evals` ([3] or [n, 3]) under random rotations: d6 [n, 6] (xx, xy, xz, yy, yz, zz), float64"""
    q, r = np.linalg.qr(rng.normal(size=(n, 3, 3)))
    q = q * np.sign(np.diagonal(r, axis1=1, axis2=2))[:, None, :]
    D = np.einsum("nik,nk,njk->nij", q, np.broadcast_to(np.asarray(evals, np.float64), (n, 3)), q)
    return np.stack([D[:, 0, 0], D[:, 0, 1], D[:, 0, 2], D[:, 1, 1], D[:, 1, 2], D[:, 2, 2]], 1)


def tensor_signal(bval, bvec, d6, s0):
    """the noise-free signal s0 * exp(-b g'Dg) [n, nvol] of the tensors d6 [n, 6] in float64, through the Float32 design matrix
    (so that the fit recovers d6 exactly, not up to the rounding of b * g_i * g_j)"""
    A = design_dti(bval, bvec).astype(np.float64)
    return np.asarray(s0, np.float64).reshape(-1, 1) * np.exp(np.asarray(d6, np.float64) @ A[:, :6].T)


CLASSES = {"generic": (1.7e-3, 0.9e-3, 0.3e-3), "prolate": (1.7e-3, 0.3e-3, 0.3e-3), "oblate": (1.2e-3, 1.2e-3, 0.3e-3),
           "isotropic": (3e-3, 3e-3, 3e-3)}


def axis_scheme(b=1000.0):
    """a b0 and +-x, +-y, +-z: rank 4, the xy, xz and yz columns of A are zero"""
    e = np.eye(3, dtype=np.float32)
    return np.array([0.0] + [b] * 6, np.float32), np.vstack([np.zeros((1, 3), np.float32), e, -e])


def coplanar_scheme(ndir=28, nb0=4, b=1000.0, extra=8, seed=1):
    """nb0 b0 frames, ndir directions in the plane z = 0 and `extra` directions off it: knocking the `extra` frames out leaves a
    positive subset of nb0 + ndir rows and rank 4 (xx, xy, yy, 1)"""
    th = np.pi * (np.arange(ndir) + 0.5) / ndir
    plane = np.stack([np.cos(th), np.sin(th), np.zeros(ndir)], 1)
    off = np.random.default_rng(seed).normal(size=(extra, 3))
    off /= np.linalg.norm(off, axis=1, keepdims=True)
    bvec = np.vstack([np.zeros((nb0, 3)), plane, off]).astype(np.float32)
    bval = np.concatenate([np.zeros(nb0), np.full(ndir + extra, b)]).astype(np.float32)
    return bval, bvec


def coplanar_signal(bval, bvec, n, seed):
    """noisy generic tensors on coplanar_scheme() with all b0 frames but one and every direction off the plane knocked out"""
    rng = np.random.default_rng(seed)
    s = tensor_signal(bval, bvec, random_tensors(CLASSES["generic"], n, rng), rng.uniform(800.0, 1200.0, n))
    s = np.maximum(s + rng.normal(scale=20.0, size=s.shape), 1.0).astype(np.float32)
    s[:, 1:4] = 0                                                            # one b0 left
    s[:, 32:] = -1                                                           # the directions off the plane
    return s


def pinv_ref(A, dtype=np.float64):
    """LinearAlgebra.pinv(A): singular values <= eps(Float32) * min(m, n) * the largest are dropped"""
    A = np.asarray(A, dtype)
    nz = (A != 0).any(0)                                    # pinv([B 0]) = [pinv(B); 0]: a zero column of A gives a row of exact zeros
    P = np.zeros(A.shape[::-1], dtype)                      # (LAPACK's singular vectors leak ~1e-16 into such a row)
    P[nz] = np.linalg.pinv(A[:, nz], rcond=EPS32 * min(A.shape))
    return P


def _fit_d(dwi, mask, bval, A32, dtype, chunk=16384):
    """the branch table and the solution vector d [nvox, np] of every voxel; also branch [nvox] and the number of subset solves"""
    A = A32.astype(dtype)
    nvol, npar = A.shape
    s = np.asarray(dwi)
    assert s.shape[-1] == nvol, "dwi must be [..., nvol]"
    shape = s.shape[:-1]
    s = s.reshape(-1, nvol)
    m = np.asarray(mask).reshape(-1) != 0                                   # dti.jl:261
    assert m.shape[0] == s.shape[0], "mask does not match the volume"
    bval = np.asarray(bval, np.float32).reshape(-1)
    ib0 = bval == bval.min()                                                # dti.jl:117
    with np.errstate(all="ignore"):
        pos = s > 0                                                         # dti.jl:291
    npos = pos.sum(1)
    full = m & (npos == nvol)                                               # dti.jl:294
    sub = m & ~full & (npos > 6) & pos[:, ib0].any(1)                       # dti.jl:297
    branch = np.where(full, FULL, np.where(sub, SUBSET, np.where(m, ZEROS, OUTSIDE))).astype(np.int8)
    d = np.zeros((s.shape[0], npar), dtype)
    nz = (A != 0).any(0)                                                    # (as in pinv_ref)
    with np.errstate(all="ignore"):
        if full.any():
            d[full] = np.log(s[full].astype(dtype)) @ pinv_ref(A, dtype).T  # dti.jl:295-296
        idx = np.flatnonzero(sub)
        for c0 in range(0, idx.size, chunk):                                # dti.jl:298
            ii = idx[c0:c0 + chunk]
            p = pos[ii]
            logs = np.where(p, np.log(np.where(p, s[ii], 1).astype(dtype)), 0)
            A0 = np.where(p[:, :, None], A[None, :, nz], 0)
            P = np.linalg.pinv(A0, rcond=EPS32 * min(7, npar))              # npos >= 7: min(npos, np) = np
            d[ii[:, None], np.flatnonzero(nz)[None]] = np.einsum("vji,vi->vj", P, logs)
    return d, branch, int(sub.sum()), shape


def dti_maps(l1, l2, l3):
    """dti.jl:325-335"""
    rd = l2 + l3
    md = (l1 + rd) / 3
    rd = rd / 2
    with np.errstate(all="ignore"):
        fa = np.sqrt(((l1 - md) ** 2 + (l2 - md) ** 2 + (l3 - md) ** 2) / (l1 ** 2 + l2 ** 2 + l3 ** 2) * 1.5)
    return rd, md, fa


def dti_fit_ref(dwi, mask, bval, bvec, dtype=np.float64):
    """dti_fit(dwi, mask) -> dict: the ten fields ([...] and [..., 3]), d [..., 7], D [..., 3, 3] (the tensor), branch [...] and
    nsubset (the number of row-subset solves).  Voxels whose tensor is not finite (+Inf samples) come back NaN in the
    eigen-decomposition and the maps; s0 = exp(d7) as computed."""
    d, branch, nsub, shape = _fit_d(dwi, mask, bval, design_dti(bval, bvec), dtype)
    n = d.shape[0]
    D = np.empty((n, 3, 3), dtype)
    for (i, j), k in zip(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)), range(6)):       # dti.jl:307-311
        D[:, i, j] = d[:, k]
        D[:, j, i] = d[:, k]
    solved = (branch == FULL) | (branch == SUBSET)
    fin = solved & np.isfinite(D).all((1, 2))
    w = np.full((n, 3), np.nan, dtype)
    E = np.full((n, 3, 3), np.nan, dtype)
    if fin.any():
        w[fin], E[fin] = np.linalg.eigh(D[fin])                             # ascending; columns are the eigenvectors
    w[~solved] = 0
    E[~solved] = 0
    l1, l2, l3 = w[:, 2], w[:, 1], w[:, 0]                                  # dti.jl:313
    rd, md, fa = dti_maps(l1, l2, l3)
    with np.errstate(all="ignore"):
        s0 = np.where(solved, np.exp(d[:, 6]), 0)                           # dti.jl:305
    out = dict(s0=s0, eigval1=l1, eigval2=l2, eigval3=l3, eigvec1=E[:, :, 2], eigvec2=E[:, :, 1], eigvec3=E[:, :, 0],
               rd=np.where(solved, rd, 0), md=np.where(solved, md, 0), fa=np.where(solved, fa, 0), d=d, D=np.where(solved[:, None, None], D, 0))
    out = {k: np.ascontiguousarray(v).reshape(shape + v.shape[1:]) for k, v in out.items()}
    out["branch"] = branch.reshape(shape)
    out["nsubset"] = nsub
    return out


def adc_fit_ref(dwi, mask, bval, dtype=np.float64):
    """adc_fit(dwi, mask) (dti.jl:164-213) -> dict: adc, s0 [...], d [..., 2], branch [...], nsubset"""
    d, branch, nsub, shape = _fit_d(dwi, mask, bval, design_adc(bval), dtype)
    solved = (branch == FULL) | (branch == SUBSET)
    with np.errstate(all="ignore"):
        s0 = np.where(solved, np.exp(d[:, 1]), 0)                           # dti.jl:212
    return dict(adc=d[:, 0].reshape(shape), s0=s0.reshape(shape), d=d.reshape(shape + (2,)), branch=branch.reshape(shape), nsubset=nsub)


# ------------------------------------------------------------------------------------------------------------------------------
# deviations of a float32 result from the restatement (the unit of every figure)
# ------------------------------------------------------------------------------------------------------------------------------
ILL_R = 1.0 - 1e-3            # |r| of the closed-form solver above which its acos is ill-conditioned (util.solver_r)
VEC_GAP = 1e-2                # eigenvectors are compared in direction where ref64's eigenvalue gap exceeds this fraction of |eigval1|


def comparable(ref):
    """the voxels whose values are compared: solved by the restatement, with a finite tensor and a finite S0"""
    solved = (ref["branch"] == FULL) | (ref["branch"] == SUBSET)
    if "D" in ref:
        return solved & np.isfinite(ref["D"]).all((-1, -2)) & np.isfinite(ref["s0"])
    return solved & np.isfinite(ref["d"]).all(-1) & np.isfinite(ref["s0"])


def ill_conditioned(ref):
    """the voxels in which the closed form's acos is ill-conditioned: |r| > 1 - 1e-3, r from ref64's eigenvalues"""
    from util import solver_r
    with np.errstate(all="ignore"):
        return np.abs(solver_r(ref["eigval1"], ref["eigval2"], ref["eigval3"])) > ILL_R


def dti_errors(got, ref):
    """per-voxel deviations of the ten fields `got` from the restatement `ref` (dti_fit_ref): the eigenvalues, rd and md in
    units of the voxel's |eigval1|, s0 relative, fa absolute; per eigenvector k the residual |D64 v - l64_k v| / |eigval1| (res),
    | |v| - 1 | (norm) and, where ref64's gap to the neighbouring eigenvalues exceeds VEC_GAP * |eigval1|, 1 - |v . v64| (dir, 0
    elsewhere); orth = the largest |v_i . v_j|.  Every entry has the shape of the volume; voxels outside comparable(ref) hold 0."""
    ok = comparable(ref)
    shape = ok.shape
    g = {k: np.asarray(got[k], np.float64).reshape(shape + ((3,) if "vec" in k else ())) for k in FIELDS}
    with np.errstate(all="ignore"):
        lam1 = np.abs(ref["eigval1"])
        unit = np.where(ok & (lam1 > 0), lam1, 1.0)
        e = {k: np.abs(g[k] - ref[k]) / unit for k in ("eigval1", "eigval2", "eigval3", "rd", "md")}
        e["s0"] = np.abs(g["s0"] - ref["s0"]) / np.where(ok, np.abs(ref["s0"]), 1.0)
        e["fa"] = np.abs(g["fa"] - ref["fa"])
        gap12 = (ref["eigval1"] - ref["eigval2"]) > VEC_GAP * lam1
        gap23 = (ref["eigval2"] - ref["eigval3"]) > VEC_GAP * lam1
        for k, sep in ((1, gap12), (2, gap12 & gap23), (3, gap23)):
            v = g["eigvec%d" % k]
            Dv = np.einsum("...ij,...j->...i", ref["D"], v)
            e["res%d" % k] = np.linalg.norm(Dv - ref["eigval%d" % k][..., None] * v, axis=-1) / unit
            e["norm%d" % k] = np.abs(np.linalg.norm(v, axis=-1) - 1.0)
            e["dir%d" % k] = np.where(sep, 1.0 - np.abs((v * ref["eigvec%d" % k]).sum(-1)), 0.0)
        e["orth"] = np.maximum(np.maximum(np.abs((g["eigvec1"] * g["eigvec2"]).sum(-1)), np.abs((g["eigvec1"] * g["eigvec3"]).sum(-1))),
                               np.abs((g["eigvec2"] * g["eigvec3"]).sum(-1)))
    return {k: np.where(ok, v, 0.0) for k, v in e.items()}


def adc_errors(adc, s0, ref):
    """adc absolute, s0 relative; 0 outside comparable(ref)"""
    ok = comparable(ref)
    with np.errstate(all="ignore"):
        e = dict(adc=np.abs(np.asarray(adc, np.float64).reshape(ok.shape) - ref["adc"]),
                 s0=np.abs(np.asarray(s0, np.float64).reshape(ok.shape) - ref["s0"]) / np.where(ok, np.abs(ref["s0"]), 1.0))
    return {k: np.where(ok, v, 0.0) for k, v in e.items()}


def class_max(err, ill):
    """{field: (max over the well-conditioned voxels, max over the ill-conditioned ones)}"""
    return {k: (float(v[~ill].max()) if (~ill).any() else 0.0, float(v[ill].max()) if ill.any() else 0.0) for k, v in err.items()}
