"""A NumPy restatement of dki_fit ("DKI") in a precision of the caller's choice (TEST INFRASTRUCTURE, NumPy only).

    ln S = ln S0 - b g'Dg + (b^2 / 6) sum_ijkl g_i g_j g_k g_l V_ijkl,      V = MD^2 W

22 unknowns: d[0:6] = Dxx Dxy Dxz Dyy Dyz Dzz, d[6:21] = V in the order KT_ORDER, d[21] = ln S0.  The design is built in float64 from
the float32 tables with b in ms/um^2 and pseudo-inverted with LinearAlgebra.pinv's cut-off (eps32 * min(m, n)); rows 0-5 of the
pseudo-inverse are then scaled by 1e-3 and rows 6-20 by 1e-6.  With dtype float64 everything after that stays float64 (the truth the
kernels are measured against); with float32 the pseudo-inverse and the direction table are rounded once, as the library rounds them, and
the logarithms, the fit, the eigen-decomposition (LAPACK's `eigh`) and the maps run in float32.

Per voxel: mask == 0, max(s) <= 0 or a NaN sample -> every output 0; otherwise d = pA log(max(s, min_signal)).
K(n) = clip(V(n) / max(D(n), min_diffusivity)^2, min_kurtosis, max_kurtosis), both written as comparisons (NaN passes through).
mk = the sequential sum of K over rows 0 .. nverts/2 - 1 of the tessellation divided by their number; ak = K(eigvec1);
rk = the mean of K(cos(phi) eigvec2 + sin(phi) eigvec3) over phi = m pi / 16, m = 0..15; kt = d[6:21] / md^2."""
import numpy as np

import dti_ref as DR

EPS32 = DR.EPS32
KT_ORDER = ("xxxx", "yyyy", "zzzz", "xxxy", "xxxz", "xyyy", "yyyz", "xzzz", "yzzz", "xxyy", "xxzz", "yyzz", "xxyz", "xyyz", "xyzz")
KT_POW = tuple((w.count("x"), w.count("y"), w.count("z")) for w in KT_ORDER)
KT_MULT = (1, 1, 1, 4, 4, 4, 4, 4, 4, 6, 6, 6, 12, 12, 12)
FIELDS = DR.FIELDS + ("mk", "ak", "rk", "kt")
DEFAULTS = dict(min_signal=1e-4, min_diffusivity=1e-6, min_kurtosis=-3.0 / 7.0, max_kurtosis=10.0)
NPHI = 16


def dir_rows(n, dtype=np.float64):
    """n [..., 3] -> [..., 21]: xx 2xy 2xz yy 2yz zz, then the 15 quartic monomials times their multiplicities; computed in dtype"""
    n = np.asarray(n, dtype)
    x, y, z = n[..., 0], n[..., 1], n[..., 2]
    two = dtype(2)
    cols = [x * x, two * (x * y), two * (x * z), y * y, two * (y * z), z * z]
    for (a, b, c), mult in zip(KT_POW, KT_MULT):
        cols.append(dtype(mult) * (x ** a * y ** b * z ** c))
    return np.stack(cols, -1)


def design(bval, bvec):
    """the float64 design [nvol, 22] from the float32 tables, b in ms/um^2"""
    b = np.asarray(bval, np.float32).reshape(-1).astype(np.float64) / 1000.0
    rows = dir_rows(np.asarray(bvec, np.float32).reshape(-1, 3).astype(np.float64))
    A = np.empty((b.shape[0], 22))
    A[:, :6] = -b[:, None] * rows[:, :6]
    A[:, 6:21] = (b * b / 6.0)[:, None] * rows[:, 6:]
    A[:, 21] = 1.0
    return A


ROW_SCALE = np.concatenate([np.full(6, 1e-3), np.full(15, 1e-6), [1.0]])


def pinv_scaled(bval, bvec):
    """(pA float64 [22, nvol] with its rows scaled to mm^2/s and mm^4/s^2, rank under pinv's cut-off)"""
    A = design(bval, bvec)
    sv = np.linalg.svd(A, compute_uv=False)
    rank = int((sv > EPS32 * min(A.shape) * sv.max()).sum())
    return np.linalg.pinv(A, rcond=EPS32 * min(A.shape)) * ROW_SCALE[:, None], rank


def model_signal(bval, bvec, d6, v15, s0):
    """the noise-free model signal [n, nvol] in float64 through the float64 design of the float32 tables (so that the fit returns
    d6 [n, 6] in mm^2/s and v15 [n, 15] in mm^4/s^2 exactly, not up to the rounding of the tables)"""
    A = design(bval, bvec)
    e = np.asarray(d6, np.float64) @ (A[:, :6] * 1e3).T + np.asarray(v15, np.float64) @ (A[:, 6:21] * 1e6).T
    return np.asarray(s0, np.float64).reshape(-1, 1) * np.exp(e)


def isotropic_v(w):
    """V(n) == w for every unit n: xxxx = yyyy = zzzz = w, xxyy = xxzz = yyzz = w / 3"""
    v = np.zeros(15)
    v[:3] = w
    v[9:12] = w / 3.0
    return v


def kurtosis(rows, d, p, dtype):
    """K of the directions rows [nvox, ndir, 21] (or [ndir, 21] for all voxels) for the solutions d [nvox, 22]"""
    rows = np.asarray(rows, dtype)
    if rows.ndim == 2:
        dn, vn = d[:, :6] @ rows[:, :6].T, d[:, 6:21] @ rows[:, 6:].T
    else:
        dn, vn = np.einsum("vk,vnk->vn", d[:, :6], rows[..., :6]), np.einsum("vk,vnk->vn", d[:, 6:21], rows[..., 6:])
    floor = dtype(np.float32(p["min_diffusivity"]))
    lo, hi = dtype(np.float32(p["min_kurtosis"])), dtype(np.float32(p["max_kurtosis"]))
    with np.errstate(all="ignore"):
        den = np.where(dn < floor, floor, dn)
        k = vn / (den * den)
        if lo < hi:
            k = np.where(k < lo, lo, k)
            k = np.where(k > hi, hi, k)
    return k


def dki_fit_ref(dwi, mask, bval, bvec, verts, dtype=np.float64, phi0=0.0, eigen=None, **params):
    """dki_fit -> dict: the 14 fields ([...], [..., 3], kt [..., 15]), d [..., 22], D [..., 3, 3], branch [...] (dti_ref's codes: FULL
    where the voxel is solved, ZEROS where it is skipped, OUTSIDE).  phi0: an offset of the radial quadrature's angles (tests).
    eigen: None for LAPACK's `eigh` in dtype, or the eigen-solver to restate -- a callable d6 [n, 6] -> (eigenvalues [n, 3] ascending,
    eigenvectors [n, 3, 3] in columns); the GPU tests pass the oracle's float32 closed form (the algorithm the definition names)
    for the float32 figure, as the DTI tests do."""
    dtype = np.dtype(dtype).type
    p = dict(DEFAULTS, **params)
    pA, rank = pinv_scaled(bval, bvec)
    assert rank == 22, "the scheme does not determine the 22 unknowns (rank %d)" % rank
    if dtype is np.float32:
        pA = pA.astype(np.float32)
    s = np.asarray(dwi)
    nvol = pA.shape[1]
    assert s.shape[-1] == nvol, "dwi must be [..., nvol]"
    shape = s.shape[:-1]
    s = s.reshape(-1, nvol)
    n = s.shape[0]
    m = np.asarray(mask).reshape(-1) != 0
    with np.errstate(all="ignore"):
        nan = np.isnan(s).any(1)
        solved = m & ~nan & (np.where(np.isnan(s), -np.inf, s).max(1) > 0)
        lo = np.float32(p["min_signal"]).astype(s.dtype)
        logs = np.log(np.where(s < lo, lo, s).astype(dtype))
        d = (logs @ pA.T).astype(dtype)
    d[~solved] = 0
    D = np.empty((n, 3, 3), dtype)
    for (i, j), k in zip(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)), range(6)):
        D[:, i, j] = d[:, k]
        D[:, j, i] = d[:, k]
    fin = solved & np.isfinite(D).all((1, 2))
    w = np.full((n, 3), np.nan, dtype)
    E = np.full((n, 3, 3), np.nan, dtype)
    if fin.any():
        w[fin], E[fin] = np.linalg.eigh(D[fin]) if eigen is None else eigen(d[fin, :6])
    w[~solved] = 0
    E[~solved] = 0
    l1, l2, l3 = w[:, 2], w[:, 1], w[:, 0]
    rd, md, fa = DR.dti_maps(l1, l2, l3)
    e1, e2, e3 = E[:, :, 2], E[:, :, 1], E[:, :, 0]
    with np.errstate(all="ignore"):
        s0 = np.where(solved, np.exp(d[:, 21]), 0)
        v = np.asarray(verts, np.float32)
        table = dir_rows(v[: v.shape[0] // 2].astype(np.float64)).astype(dtype)       # built in float64, rounded once
        K = kurtosis(table, d, p, dtype)
        mk = np.cumsum(K, axis=1, dtype=dtype)[:, -1] / dtype(K.shape[1])             # a sequential sum in vertex order
        ak = kurtosis(dir_rows(e1, dtype)[:, None, :], d, p, dtype)[:, 0]
        phi = phi0 + np.arange(NPHI) * np.pi / NPHI
        c, sn = np.cos(phi).astype(dtype), np.sin(phi).astype(dtype)
        ring = c[None, :, None] * e2[:, None, :] + sn[None, :, None] * e3[:, None, :]
        rk = np.cumsum(kurtosis(dir_rows(ring, dtype), d, p, dtype), axis=1, dtype=dtype)[:, -1] / dtype(NPHI)
        kt = d[:, 6:21] / (md * md)[:, None]
    z = ~solved
    out = dict(s0=s0, eigval1=l1, eigval2=l2, eigval3=l3, eigvec1=e1, eigvec2=e2, eigvec3=e3, rd=np.where(z, 0, rd), md=np.where(z, 0, md),
               fa=np.where(z, 0, fa), mk=np.where(z, 0, mk), ak=np.where(z, 0, ak), rk=np.where(z, 0, rk), kt=np.where(z[:, None], 0, kt),
               d=d, D=np.where(z[:, None, None], 0, D))
    out = {k: np.ascontiguousarray(v).reshape(shape + v.shape[1:]) for k, v in out.items()}
    out["branch"] = np.where(solved, DR.FULL, np.where(m, DR.ZEROS, DR.OUTSIDE)).astype(np.int8).reshape(shape)
    return out


def dki_errors(got, ref):
    """dti_ref.dti_errors for the ten DTI fields, plus mk absolute; ak absolute where ref64's gap between eigval1 and eigval2 exceeds
    VEC_GAP * |eigval1| (the axis it is measured along); rk absolute where the gap between eigval2 and eigval3 exceeds it too (the
    quadrature starts at eigvec2, and where a clip is active K(phi) is not smooth, so the 16-point rule depends on that start, which
    is arbitrary where the two are degenerate); 0 elsewhere; kt in units of the case's largest |W|.  Voxels outside
    dti_ref.comparable(ref) hold 0."""
    e = DR.dti_errors(got, ref)
    ok = DR.comparable(ref)
    shape = ok.shape
    with np.errstate(all="ignore"):
        gap12 = (ref["eigval1"] - ref["eigval2"]) > DR.VEC_GAP * np.abs(ref["eigval1"])
        gap23 = (ref["eigval2"] - ref["eigval3"]) > DR.VEC_GAP * np.abs(ref["eigval1"])
        e["mk"] = np.abs(np.asarray(got["mk"], np.float64).reshape(shape) - ref["mk"])
        for k, gap in (("ak", gap12), ("rk", gap12 & gap23)):
            e[k] = np.where(gap, np.abs(np.asarray(got[k], np.float64).reshape(shape) - ref[k]), 0.0)
        unit = np.abs(ref["kt"][ok]).max() if ok.any() else 1.0
        e["kt"] = np.abs(np.asarray(got["kt"], np.float64).reshape(shape + (15,)) - ref["kt"]).max(-1) / (unit if unit > 0 else 1.0)
    for k in ("mk", "ak", "rk", "kt"):
        e[k] = np.where(ok, e[k], 0.0)
    return e


# ------------------------------------------------------------------------------------------------------------------------------
# schemes and signals of the tests
# ------------------------------------------------------------------------------------------------------------------------------
def shells_scheme(nb0, ndirs, bs, seed, b0=0.0):
    """nb0 frames at b0, then ndirs[k] directions at bs[k] (a direction set of its own per shell)"""
    from fibers_jl_amd import phantom
    bval, bvec = [np.full(nb0, b0)], [np.tile(np.array([[1.0, 0.0, 0.0]], np.float32), (nb0, 1))]
    for k, (nd, b) in enumerate(zip(ndirs, bs)):
        bval.append(np.full(nd, b))
        bvec.append(phantom.sphere_dirs(nd, seed + k))
    return np.concatenate(bval).astype(np.float32), np.vstack(bvec).astype(np.float32)


def scheme(nvol, seed=3):
    """22 frames (1 + 10 + 11 at b = 1000, 2000), 61 frames (1 + 30 + 30 at b = 1000, 2500), 270 frames (the headline scheme)"""
    from fibers_jl_amd import phantom
    if nvol == 270:
        return phantom.scheme_gqi(18, 84, (1000.0, 2000.0, 3000.0), seed)
    if nvol == 61:
        return shells_scheme(1, (30, 30), (1000.0, 2500.0), seed)
    assert nvol == 22
    return shells_scheme(1, (10, 11), (1000.0, 2000.0), seed)


def compartment_signal(bval, bvec, evals, n, rng, s0, noise=0.0):
    """n voxels of three compartments that share their axes (random rotations): the eigenvalues `evals` scaled by 0.5, 1 and 1.5
    with fractions 0.3, 0.4, 0.3 (mean `evals`, apparent kurtosis about 0.4).  noise: a fraction of the S0 scale, clipped at 1e-3
    of it (every sample stays positive).  float32 [n, nvol]"""
    A = DR.design_dti(bval, bvec).astype(np.float64)
    d6 = DR.random_tensors(evals, n, rng)
    e = d6 @ A[:, :6].T
    s = sum(f * np.exp(c * e) for f, c in ((0.3, 0.5), (0.4, 1.0), (0.3, 1.5)))
    s0 = np.broadcast_to(np.asarray(s0, np.float64), (2,))
    s = rng.uniform(s0[0], s0[1], (n, 1)) * s
    if noise:
        scale = 0.5 * (s0[0] + s0[1])
        s = np.maximum(s + rng.normal(scale=noise * scale, size=s.shape), 1e-3 * scale)
    return s.astype(np.float32)
