"""A NumPy / SciPy restatement of constrained spherical deconvolution as include/fibers_hip.h defines it ("Constrained spherical
deconvolution"), in a chosen float type.  Test infrastructure only.

The basis comes from scipy.special.lpmv, the quadrature from numpy's leggauss, the initial fit from lstsq and the constrained solves
from LAPACK's Cholesky: nothing is shared with the library.  `rec` takes tables as float32 arrays -- a plan's, or `design`'s float64
tables rounded -- and reports, per voxel, the number of solves and the margin min |a - thr| / max |a| over all passes: how close the
voxel came to a different set.  perm: a permutation of the shell frames, i.e. a second summation order of X'X and X's."""
from math import factorial

import numpy as np
from scipy.linalg import solve_triangular
from scipy.special import lpmv

f32 = np.float32


def ncoef(lmax):
    return (lmax + 1) * (lmax + 2) // 2


def sh_basis(dirs, lmax):
    """[ndir, n] float64: real even harmonics, column l (l + 1) / 2 + m"""
    d = np.asarray(dirs, np.float64).reshape(-1, 3)
    d = d / np.linalg.norm(d, axis=1)[:, None]
    ct, phi = np.clip(d[:, 2], -1.0, 1.0), np.arctan2(d[:, 1], d[:, 0])
    Y = np.zeros((d.shape[0], ncoef(lmax)))
    for l in range(0, lmax + 1, 2):
        for m in range(-l, l + 1):
            am = abs(m)
            N = np.sqrt((2 * l + 1) / (4 * np.pi) * factorial(l - am) / factorial(l + am))
            P = lpmv(am, l, ct)
            ang = np.sqrt(2.0) * np.cos(m * phi) if m > 0 else (1.0 if m == 0 else np.sqrt(2.0) * np.sin(am * phi))
            Y[:, l * (l + 1) // 2 + m] = N * P * ang
    return Y


def response_R(bbar, lpar, lperp, s0, lmax):
    """R_l, l = 0, 2, .. lmax: sqrt(4 pi / (2l + 1)) 2 pi int s0 exp(-bbar (lperp + (lpar - lperp) t^2)) Y_l0(t) dt"""
    t, w = np.polynomial.legendre.leggauss(64)
    sig = s0 * np.exp(-bbar * (lperp + (lpar - lperp) * t * t))
    out = []
    for l in range(0, lmax + 1, 2):
        yl0 = np.sqrt((2 * l + 1) / (4 * np.pi)) * lpmv(0, l, t)
        out.append(np.sqrt(4 * np.pi / (2 * l + 1)) * 2 * np.pi * np.sum(w * sig * yl0))
    return np.array(out)


def shell_frames(bval, b0_thresh=50.0, shell=None, b_tol=0.05):
    b = np.asarray(bval, f32)
    sh = f32(b.max() if shell is None else shell)
    return np.nonzero((b > f32(b0_thresh)) & (np.abs(b - sh) <= f32(b_tol) * sh))[0].astype(np.int32)


def design(bval, bvec, verts, response, lmax=8, b0_thresh=50.0, shell=None, b_tol=0.05, lam=1.0):
    """float64 tables: dict(frames, bbar, R, X [nshell, n], B [nreg, n], Y [nreg, n]); verts: the whole tessellation [2 nreg, 3].
    The response is taken as the float32 values the library receives."""
    lpar, lperp, s0 = (float(f32(v)) for v in response)
    frames = shell_frames(bval, b0_thresh, shell, b_tol)
    bbar = float(np.mean(np.asarray(bval, f32)[frames].astype(np.float64)))
    R = response_R(bbar, lpar, lperp, s0, lmax)
    col_l = np.concatenate([[l] * (2 * l + 1) for l in range(0, lmax + 1, 2)])
    X = sh_basis(np.asarray(bvec, f32).reshape(-1, 3)[frames], lmax) * R[col_l // 2][None, :]
    nreg = np.asarray(verts).shape[0] // 2
    Y = sh_basis(np.asarray(verts, f32)[:nreg], lmax)
    B = Y * (float(f32(lam)) * R[0] * len(frames) / nreg)
    return dict(frames=frames, bbar=bbar, R=R, X=X, B=B, Y=Y)


def rounded(t):
    """the float32 tables of a float64 design"""
    return {k: (v.astype(f32) if k in ("R", "X", "B", "Y") else v) for k, v in t.items()}


def rec(s, X, B, Y, tau=0.1, niter=50, dtype=np.float64, perm=None):
    """s: float32 [nvox, nshell] shell samples; X, B, Y: float32 tables.  Returns dict(sh [nvox, n], odf [nvox, nreg], niter [nvox],
    margin [nvox] (inf for a skipped voxel)) in `dtype`; a voxel without a positive sample is skipped (zeros).  setmin, setmax [nvox]:
    the smallest and the largest number of directions in the set over the voxel's passes (-1 for a skipped voxel): a kernel may sum
    the set's rows or, where the set is the larger side (2 count > nreg), subtract the complement's, and these say which it met."""
    s = np.asarray(s, f32)
    X, B, Y = (np.asarray(a, f32).astype(dtype) for a in (X, B, Y))
    if perm is not None:
        X, s = X[perm], s[:, perm]
    nvox, n, nreg = s.shape[0], X.shape[1], B.shape[0]
    n0 = min(n, 15)
    XtX = X.T @ X
    tauB = dtype(f32(tau)) * B[0, 0]
    sh = np.zeros((nvox, n), dtype)
    odf = np.zeros((nvox, nreg), dtype)
    nit = np.zeros(nvox, np.int32)
    margin = np.full(nvox, np.inf)
    setmin, setmax = np.full(nvox, -1, np.int64), np.full(nvox, -1, np.int64)
    for v in range(nvox):
        sv = s[v].astype(dtype)
        if not (s[v] > 0).any():
            continue
        z = X.T @ sv
        f = np.zeros(n, dtype)
        f[:n0] = np.linalg.lstsq(X[:, :n0], sv, rcond=None)[0]
        thr = tauB * f[0]
        prev = None
        for _ in range(niter):
            a = B @ f
            with np.errstate(invalid="ignore", divide="ignore"):
                margin[v] = min(margin[v], float(np.min(np.abs(a - thr)) / np.max(np.abs(a))))
            cur = a < thr
            count = int(cur.sum())
            setmin[v], setmax[v] = (count if setmin[v] < 0 else min(setmin[v], count)), max(setmax[v], count)
            if prev is not None and np.array_equal(cur, prev):
                break
            Bs = B[cur]
            L = np.linalg.cholesky(XtX + Bs.T @ Bs)
            f = solve_triangular(L.T, solve_triangular(L, z, lower=True), lower=False)
            nit[v] += 1
            prev = cur
        sh[v] = f
        odf[v] = np.maximum(Y @ f, 0)
    return dict(sh=sh, odf=odf, niter=nit, margin=margin, setmin=setmin, setmax=setmax)


def peaks(odf, verts, faces, npeak=3):
    """(peak [nvox, npeak, 3], f [nvox, npeak], isort [nvox, npeak], nvalid [nvox]) of float32 ODFs by the reference's find_peaks!"""
    from oracle import oracle_np
    o = np.asarray(odf, f32)
    nreg = o.shape[1]
    faces0 = oracle_np.fold_faces(faces, nreg)
    V = np.asarray(verts, f32)
    pk = np.zeros((o.shape[0], npeak, 3), f32)
    amp = np.zeros((o.shape[0], npeak), f32)
    top = np.zeros((o.shape[0], npeak), np.int64)
    nval = np.zeros(o.shape[0], np.int64)
    for v in range(o.shape[0]):
        isort, nvalid, _ = oracle_np.find_peaks(o[v], faces0)
        top[v], nval[v] = isort[:npeak], nvalid
        for k in range(min(nvalid, npeak)):
            pk[v, k], amp[v, k] = V[isort[k]], o[v, isort[k]]
    return pk, amp, top, nval


def signal(bval, bvec, frames, fibres, weights, lpar, lperp, s0, iso=0.0, d_iso=1.0e-3):
    """noise-free multi-tensor signal on the shell frames: sum_k w_k s0 exp(-b (lperp + (lpar - lperp) (g.u_k)^2)) + iso s0 exp(-b d_iso)"""
    b = np.asarray(bval, np.float64)[frames]
    g = np.asarray(bvec, np.float64).reshape(-1, 3)[frames]
    out = iso * s0 * np.exp(-b * d_iso)
    for u, w in zip(fibres, weights):
        u = np.asarray(u, np.float64) / np.linalg.norm(u)
        out = out + w * s0 * np.exp(-b * (lperp + (lpar - lperp) * (g @ u) ** 2))
    return out


# seeds whose random directions determine the harmonics comfortably when the shell has no frame to spare (sigma_min / sigma_max of X
# above 2e-4; most seeds are ten times worse there, and the golden spiral of phantom.sphere_dirs is antipodally symmetric: rank n - 1)
_SEEDS = {(8, 45): 142, (8, 46): 142, (6, 28): 108, (6, 29): 108, (4, 15): 131, (4, 16): 36, (2, 6): 133, (2, 7): 11}


def scheme(ndir=64, lmax=8, b=3000.0, nb0=4, seed=None):
    """(bval, bvec): nb0 frames at b = 5 first, then ndir random directions on one shell"""
    rng = np.random.default_rng(_SEEDS.get((lmax, ndir), 5) if seed is None else seed)
    g = rng.normal(size=(ndir, 3))
    g /= np.linalg.norm(g, axis=1)[:, None]
    bval = np.concatenate([np.full(nb0, 5.0), np.full(ndir, b)]).astype(f32)
    return bval, np.concatenate([np.zeros((nb0, 3)), g]).astype(f32)
