"""A NumPy / SciPy restatement of multi-shell multi-tissue deconvolution as include/fibers_hip.h defines it ("Multi-shell multi-tissue
deconvolution"), in a chosen float type.  Test infrastructure only.

Nothing is shared with the library: the basis and the response quadrature are csd_ref's (scipy's lpmv, numpy's leggauss), the shell
walk, the tables and the loop are written out here, the initial fit is lstsq and the constrained solves LAPACK's Cholesky.  `rec`
takes tables as float32 arrays -- a plan's, or `design`'s float64 tables rounded -- and reports per voxel the number of solves, the
smallest and largest number of WM rows in the set, whether each isotropic row was ever in the set and ever out of it, gap = the smallest
|a_i - thr_i| over all passes and rows, and `a` of every pass (so that two summation orders can be compared pass by pass).  perm: a
permutation of the frames, i.e. a second summation order of X'X and X's."""
import numpy as np
from scipy.linalg import solve_triangular

import csd_ref
from csd_ref import ncoef, sh_basis

f32 = np.float32


def shells(bval, b0_thresh=50.0, b_tol=0.05):
    """(shell int32 [nvol], bbar float64 [nshells]): shell 0 = the frames with b <= b0_thresh; the others walked in ascending b, ties in
    frame order, a frame joining the current shell while b <= (1 + 2 b_tol) b_first"""
    b = np.asarray(bval, f32)
    lim = 1.0 + 2.0 * float(f32(b_tol))
    shell = np.zeros(len(b), np.int32)
    hi = np.nonzero(b > f32(b0_thresh))[0]
    cur, first = 0, 0.0
    for i in hi[np.argsort(b[hi], kind="stable")]:
        if cur == 0 or not float(b[i]) <= lim * first:
            cur, first = cur + 1, float(b[i])
        shell[i] = cur
    bbar = np.array([float(np.mean(b[shell == s].astype(np.float64))) if (shell == s).any() else 0.0 for s in range(cur + 1)])
    return shell, bbar


def wm_response(lpar, lperp, s0, bbar, lmax):
    """[nshells, lmax / 2 + 1] float64: csd_ref's R_l of the float32 tensor at every shell's mean b"""
    lpar, lperp, s0 = (float(f32(v)) for v in (lpar, lperp, s0))
    return np.stack([csd_ref.response_R(float(b), lpar, lperp, s0, lmax) for b in bbar])


def design(bval, bvec, verts, wm_R, iso_r, lmax=8, b0_thresh=50.0, b_tol=0.05, lam=1.0, lam_iso=1.0):
    """float64 tables: dict(shell, bbar, X [nvol, n], B [nreg + niso, n], Y [nreg, n]); verts: the whole tessellation [2 nreg, 3].  The
    responses are taken as the float32 values the library receives."""
    shell, bbar = shells(bval, b0_thresh, b_tol)
    nwm = ncoef(lmax)
    R = np.asarray(wm_R, f32).astype(np.float64).reshape(len(bbar), -1)[:, :lmax // 2 + 1]
    iso = np.asarray(iso_r, f32).astype(np.float64).reshape(-1, len(bbar)) if np.size(iso_r) else np.zeros((0, len(bbar)))
    niso, nvol = iso.shape[0], len(shell)
    col_l = np.concatenate([[l] * (2 * l + 1) for l in range(0, lmax + 1, 2)])
    g = np.asarray(bvec, f32).reshape(-1, 3).astype(np.float64)
    X = np.zeros((nvol, nwm + niso))
    for i in range(nvol):
        if shell[i] == 0:
            X[i, 0] = np.sqrt(1.0 / (4.0 * np.pi)) * R[0, 0]
        else:
            X[i, :nwm] = sh_basis(g[i], lmax)[0] * R[shell[i]][col_l // 2]
        X[i, nwm:] = iso[:, shell[i]]
    nreg = np.asarray(verts).shape[0] // 2
    Y = np.zeros((nreg, nwm + niso))
    Y[:, :nwm] = sh_basis(np.asarray(verts, f32)[:nreg], lmax)
    B = np.zeros((nreg + niso, nwm + niso))
    B[:nreg] = Y * (float(f32(lam)) * R[shell, 0].sum() / nreg)
    for t in range(niso):
        B[nreg + t, nwm + t] = float(f32(lam_iso)) * iso[t, shell].sum()
    return dict(shell=shell, bbar=bbar, X=X, B=B, Y=Y)


def rounded(t):
    """the float32 tables of a float64 design"""
    return {k: (v.astype(f32) if k in ("X", "B", "Y") else v) for k, v in t.items()}


def rec(s, X, B, Y, nwm, tau=0.0, niter=50, dtype=np.float64, perm=None):
    """s: float32 [nvox, nvol] samples; X, B, Y: float32 tables; nwm: the number of WM columns.  Returns dict(sh [nvox, nwm], iso [nvox,
    niso], odf [nvox, nreg], niter [nvox], setmin, setmax [nvox] (WM rows in the set; -1 for a skipped voxel), iso_in, iso_out [nvox,
    niso] bool, gap [nvox] (inf for a skipped voxel), a: per voxel the [passes, nreg + niso] amplitudes) in `dtype`."""
    s = np.asarray(s, f32)
    X, B, Y = (np.asarray(a, f32).astype(dtype) for a in (X, B, Y))
    if perm is not None:
        X, s = X[perm], s[:, perm]
    nvox, n = s.shape[0], X.shape[1]
    niso = n - nwm
    nreg = B.shape[0] - niso
    idx0 = list(range(min(nwm, 15))) + list(range(nwm, n))
    XtX = X.T @ X
    tauB = dtype(f32(tau)) * B[0, 0]
    out = dict(sh=np.zeros((nvox, nwm), dtype), iso=np.zeros((nvox, niso), dtype), odf=np.zeros((nvox, nreg), dtype),
               niter=np.zeros(nvox, np.int32), setmin=np.full(nvox, -1, np.int64), setmax=np.full(nvox, -1, np.int64),
               iso_in=np.zeros((nvox, niso), bool), iso_out=np.zeros((nvox, niso), bool), gap=np.full(nvox, np.inf), a=[None] * nvox)
    for v in range(nvox):
        if not (s[v] > 0).any():
            continue
        sv = s[v].astype(dtype)
        z = X.T @ sv
        f = np.zeros(n, dtype)
        f[idx0] = np.linalg.lstsq(X[:, idx0], sv, rcond=None)[0]
        thr = np.zeros(nreg + niso, dtype)
        thr[:nreg] = tauB * f[0]
        prev, hist = None, []
        for _ in range(niter):
            a = B @ f
            hist.append(a)
            out["gap"][v] = min(out["gap"][v], float(np.min(np.abs(a - thr))))
            cur = a < thr
            count = int(cur[:nreg].sum())
            out["setmin"][v] = count if out["setmin"][v] < 0 else min(out["setmin"][v], count)
            out["setmax"][v] = max(out["setmax"][v], count)
            out["iso_in"][v] |= cur[nreg:]
            out["iso_out"][v] |= ~cur[nreg:]
            if prev is not None and np.array_equal(cur, prev):
                break
            Bs = B[cur]
            L = np.linalg.cholesky(XtX + Bs.T @ Bs)
            f = solve_triangular(L.T, solve_triangular(L, z, lower=True), lower=False)
            out["niter"][v] += 1
            prev = cur
        out["sh"][v], out["iso"][v] = f[:nwm], f[nwm:]
        out["odf"][v] = np.maximum(Y @ f, 0)
        out["a"][v] = np.array(hist)
    return out


def undecided(r, rp):
    """bool [nvox]: gap < 64 e, e = the largest |a - a_perm| of the voxel over its passes (two summation orders of the restatement); a
    voxel whose two orders take different numbers of passes is undecided"""
    bad = np.zeros(len(r["a"]), bool)
    for v, (a, ap) in enumerate(zip(r["a"], rp["a"])):
        if a is None:
            continue
        bad[v] = a.shape != ap.shape or r["gap"][v] < 64.0 * float(np.abs(a - ap).max())
    return bad


# ---- schemes and signals ------------------------------------------------------------------------------------------------------------
def scheme(nb0=6, ndirs=(20, 20, 20), bs=(1000.0, 2000.0, 3000.0), seed=5, b0=5.0):
    """(bval, bvec): nb0 frames at b0 first, then ndirs[k] random directions on shell bs[k]"""
    rng = np.random.default_rng(seed)
    bval, bvec = [np.full(nb0, b0)], [np.zeros((nb0, 3))]
    for nd, b in zip(ndirs, bs):
        g = rng.normal(size=(nd, 3))
        bval.append(np.full(nd, b))
        bvec.append(g / np.linalg.norm(g, axis=1)[:, None])
    return np.concatenate(bval).astype(f32), np.concatenate(bvec).astype(f32)


def model_responses(bbar, lmax, tensor=(1.7e-3, 0.3e-3, 1000.0), gm=(0.8e-3, 900.0), csf=(3.0e-3, 1500.0), niso=2):
    """(wm_R float32 [nshells, lmax / 2 + 1], iso_r float32 [niso, nshells]) of a prolate WM tensor and mono-exponential GM and CSF"""
    wm_R = wm_response(*tensor, bbar, lmax).astype(f32)
    iso_r = np.array([s0 * np.exp(-np.asarray(bbar) * d) for d, s0 in (gm, csf)][:niso], f32).reshape(niso, len(bbar))
    return wm_R, iso_r


def mixture(bvec, shell, bbar, wm_R, iso_r, fibres, weights, iso_w=(), tensor=(1.7e-3, 0.3e-3, 1000.0)):
    """noise-free signal of every frame from the model's own responses: sum_k w_k s0 exp(-bbar_s (lperp + (lpar - lperp) (g.u_k)^2)) +
    sum_t iso_w[t] iso_r[t][s], s the frame's shell; a shell-0 frame has no direction and takes the model's
    row for a unit fODF (sh[0] = Y_00), w_k Y_00^2 R_0(0)"""
    lpar, lperp, s0 = (float(f32(v)) for v in tensor)
    shell = np.asarray(shell)
    g = np.asarray(bvec, np.float64).reshape(-1, 3)
    b = np.asarray(bbar, np.float64)[shell]
    mean0 = float(np.asarray(wm_R, np.float64)[0, 0]) / (4.0 * np.pi)
    out = np.zeros(len(shell))
    for u, w in zip(fibres, weights):
        u = np.asarray(u, np.float64) / np.linalg.norm(u)
        out += w * np.where(shell == 0, mean0, s0 * np.exp(-b * (lperp + (lpar - lperp) * (g @ u) ** 2)))
    for t, w in enumerate(iso_w):
        out += w * np.asarray(iso_r, np.float64)[t][shell]
    return out
