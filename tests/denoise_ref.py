"""NumPy float64 restatement of dwi_denoise (include/fibers_hip.h "Marchenko-Pastur PCA denoising"), by two routes:
`eigh` of the Gram matrix and `svd` of X.  Test infrastructure only.  Besides the outputs it returns, per voxel, the two margins
that say how far the inputs are from a discontinuity of the definition: the decision margin of the rule and the spectral gap at
the cut."""
import functools

import numpy as np

ESTIMATORS = ("exp1", "exp2")
SIGMA = 1000.0 / 30.0

# (shape, N, P, k)
CASES = [((6, 5, 4), 16, 3, 2),       # M > N
         ((6, 5, 4), 40, 3, 3),       # M < N, r = 27 odd
         ((7, 6, 5), 30, 5, 3),
         ((7, 6, 5), 130, 5, 4),      # r = 125, the replay at its largest odd size
         ((5, 5, 5), 125, 5, 3),      # M = N
         ((8, 7, 7), 128, 7, 4),      # r = 128, the limit
         ((9, 8, 7), 64, 7, 4),
         ((3, 3, 3), 20, 3, 2),       # every voxel shares one patch, c runs over all 27 rows
         ((6, 5, 4), 2, 3, 1)]
# More output voxels than the kernel has persistent workgroups (DN_MAXWG = 512 in csrc/denoise.hip, a voxel a ticket): every workgroup
# goes round its loop at least twice.  Kept out of CASES, whose parametrisations stay as they are; (case, estimators held on the GPU).
LARGE_CASES = [((13, 13, 13), 16, 3, 2),     # 2197 voxels = 4.3 x 512; M = 27 > N, r = 16
               ((13, 13, 13), 40, 3, 3),     # M < N, r = 27 odd: the phantom index is live
               ((11, 10, 10), 130, 5, 4)]    # 1100 voxels; r = 125, the longest replay
LARGE_HELD = [(LARGE_CASES[0], "exp1"), (LARGE_CASES[0], "exp2"), (LARGE_CASES[1], "exp2"), (LARGE_CASES[2], "exp2")]
SEED = 20


def case_id(case):
    shape, N, P, k = case
    return "%dx%dx%d-N%d-P%d-k%d" % (shape + (N, P, k))


def phantom(shape, N, k, seed=SEED):
    """k smooth positive weight fields (cosines of random plane waves, component j divided by j + 1) times k frame profiles in
    [0.2, 1], scale 1000, Gaussian noise of sigma = 1000 / 30, rounded to float32: [nx,ny,nz,N] column-major"""
    rng = np.random.default_rng(seed)
    x, y, z = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")
    sig = np.zeros(shape + (N,))
    for j in range(k):
        kv = rng.uniform(-0.6, 0.6, 3)
        w = (np.cos(kv[0] * x + kv[1] * y + kv[2] * z + rng.uniform(0, 2 * np.pi)) + 1.5) / (j + 1)
        sig += w[..., None] * rng.uniform(0.2, 1.0, N)
    vol = 1000.0 * sig + rng.normal(0.0, SIGMA, sig.shape)
    return np.asfortranarray(vol.astype(np.float32))


def patch_start(v, n, P):
    return min(max(v - P // 2, 0), n - P)


def rule(lam_eig, q, estimator):
    """eigenvalues ascending -> (cutoff, sigma^2, decision margin over p >= cutoff - 1)"""
    r = len(lam_eig)
    lam = np.maximum(lam_eig, 0.0) / q
    clam, cutoff, sig2 = 0.0, 0, 0.0
    s1s, s2s = np.zeros(r), np.zeros(r)
    for p in range(r):
        clam += lam[p]
        gam = (p + 1) / q if estimator == "exp1" else (p + 1) / (q - (r - p - 1))
        s1, s2 = clam / (p + 1), (lam[p] - lam[0]) / (4.0 * np.sqrt(gam))
        s1s[p], s2s[p] = s1, s2
        if s2 < s1:
            sig2, cutoff = s1, p + 1
    lo = max(cutoff - 1, 0)
    den = np.maximum(s1s[lo:], s2s[lo:])
    margin = float(np.min(np.abs(s2s[lo:] - s1s[lo:]) / np.where(den > 0, den, 1.0))) if np.any(den > 0) else np.inf
    return cutoff, sig2, margin


def _patch(X, estimator, route):
    """X [M, N] float64 -> (rows [M, N]: the denoised row of every voxel of the patch, sigma, rank, margin, gap)"""
    M, N = X.shape
    r, q = min(M, N), max(M, N)
    if route == "eigh":
        G = X @ X.T if M <= N else X.T @ X
        w, V = np.linalg.eigh(G)
    else:
        U, s, Vt = np.linalg.svd(X, full_matrices=False)
        w, V = (s ** 2)[::-1], (U if M <= N else Vt.T)[:, ::-1]
    cutoff, sig2, margin = rule(w, q, estimator)
    E = V[:, cutoff:]
    Pm = E @ E.T
    rows = Pm @ X if M <= N else X @ Pm           # row c: X' (E E' e_c), or E E' x_c
    if cutoff == 0:
        rows = X.copy()
    gap = (w[cutoff] - w[cutoff - 1]) / w[-1] if 0 < cutoff < r and w[-1] > 0 else np.inf
    return rows, np.sqrt(sig2), r - cutoff, margin, gap


def denoise(vol, P, estimator="exp2", route="eigh", mask=None):
    """vol [nx,ny,nz,N] -> dict(dwi [nx,ny,nz,N], sigma, rank, margin, gap [nx,ny,nz]), float64; outside the mask the outputs are 0"""
    nx, ny, nz, N = vol.shape
    v = np.asarray(vol, np.float64)
    out = dict(dwi=np.zeros(v.shape), sigma=np.zeros((nx, ny, nz)), rank=np.zeros((nx, ny, nz)), margin=np.full((nx, ny, nz), np.inf),
               gap=np.full((nx, ny, nz), np.inf))
    done = {}
    for z in range(nz):
        for y in range(ny):
            for x in range(nx):
                if mask is not None and not mask[x, y, z]:
                    continue
                x0, y0, z0 = patch_start(x, nx, P), patch_start(y, ny, P), patch_start(z, nz, P)
                if (x0, y0, z0) not in done:
                    # row (dz P + dy) P + dx
                    X = v[x0:x0 + P, y0:y0 + P, z0:z0 + P, :].transpose(2, 1, 0, 3).reshape(P ** 3, N)
                    done[(x0, y0, z0)] = _patch(X, estimator, route)
                rows, sigma, rank, margin, gap = done[(x0, y0, z0)]
                c = ((z - z0) * P + (y - y0)) * P + (x - x0)
                out["dwi"][x, y, z] = rows[c]
                out["sigma"][x, y, z], out["rank"][x, y, z], out["margin"][x, y, z], out["gap"][x, y, z] = sigma, rank, margin, gap
    return out


@functools.lru_cache(maxsize=None)
def case_volume(case):
    shape, N, P, k = case
    vol = phantom(shape, N, k)
    vol.setflags(write=False)
    return vol


@functools.lru_cache(maxsize=None)
def case_reference(case, estimator):
    """(eigh route, svd route, d_rows, d_sigma): d = the largest absolute difference between the two routes.  Computed once per
    session and shared; do not modify."""
    shape, N, P, k = case
    vol = case_volume(case)
    a, b = denoise(vol, P, estimator, "eigh"), denoise(vol, P, estimator, "svd")
    return a, b, float(np.abs(a["dwi"] - b["dwi"]).max()), float(np.abs(a["sigma"] - b["sigma"]).max())
