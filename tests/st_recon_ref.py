"""NumPy float64 restatement of st_recon (structens.jl:40-88) as DESIGN.md §5 takes ImageFiltering to compute it.  Test
infrastructure only: the product computes this on the GPU (fibers.jl_amd/csrc/structens.hip).

    image = G_sigma * vol              (sigma > 0)
    g_d   = Scharr_d * image           (d = x, y, z)
    S     = G_rho * (g g^T)            (rho > 0; six products)
    eigen(Symmetric(S, :L))

Every filter is a correlation whose input is extended by reflection about its edge voxel (`Pad(:reflect)`, numpy.pad's
"reflect", scipy.ndimage's "mirror"), each filter reflecting its OWN input."""
import math

import numpy as np

SCHARR_D = np.array([-0.5, 0.0, 0.5])              # KernelFactors.scharr: derivative factor (correlation: f[i+1] - f[i-1])
SCHARR_S = np.array([3.0, 10.0, 3.0]) / 16.0       # ... and the smoothing factor along the two other axes


def radius(s):
    return 2 * math.ceil(s) if s > 0 else 0


def gaussian_taps(s):
    """KernelFactors.gaussian(s): 4 ceil(s) + 1 taps exp(-x^2 / (2 s^2)), normalised to sum 1 (float64)"""
    R = radius(s)
    x = np.arange(-R, R + 1, dtype=np.float64)
    w = np.exp(-x * x / (2.0 * s * s))
    return w / w.sum()


def reflect_index(i, n):
    """index i of an axis of length n mirrored about the edge voxels, repeatedly; length 1 gives 0"""
    i = np.asarray(i)
    if n == 1:
        return np.zeros_like(i)
    p = 2 * (n - 1)
    i = np.mod(i, p)
    return np.where(i < n, i, p - i)


def correlate1d(a, w, axis):
    """out[i] = sum_k w[k] a[reflect(i + k - r)] along `axis` (r = len(w) // 2)"""
    a = np.asarray(a, np.float64)
    r = len(w) // 2
    n = a.shape[axis]
    out = np.zeros_like(a)
    for k, wk in enumerate(w):
        idx = reflect_index(np.arange(n) + k - r, n)
        out += wk * np.take(a, idx, axis=axis)
    return out


def separable(a, ws):
    """ws[d] applied along axis d, one after the other (each reflects its own input, which for a separable kernel is the same
    as reflecting once)"""
    for d, w in enumerate(ws):
        a = correlate1d(a, w, d)
    return a


def gradients(vol, sigma):
    image = separable(vol, [gaussian_taps(sigma)] * 3) if sigma > 0 else np.asarray(vol, np.float64)
    out = []
    for d in range(3):
        ws = [SCHARR_S, SCHARR_S, SCHARR_S]
        ws[d] = SCHARR_D
        out.append(separable(image, ws))
    return out


def structure_tensor(vol, sigma, rho):
    """the six smoothed volumes (Sxx, Sxy, Sxz, Syy, Syz, Szz) st_recon decomposes, float64"""
    gx, gy, gz = gradients(vol, sigma)
    S = [gx * gx, gx * gy, gx * gz, gy * gy, gy * gz, gz * gz]
    if rho > 0:
        w = gaussian_taps(rho)
        S = [separable(s, [w] * 3) for s in S]
    return S


def st_recon(vol, sigma, rho):
    """-> (eigvec [nx,ny,nz,3,3], eigval [nx,ny,nz,3], S [6 volumes]) in float64; ascending eigenvalues, eigvec[..., :, j]"""
    S = structure_tensor(vol, sigma, rho)
    sxx, sxy, sxz, syy, syz, szz = S
    M = np.stack([np.stack([sxx, sxy, sxz], -1), np.stack([sxy, syy, syz], -1), np.stack([sxz, syz, szz], -1)], -2)
    val, vec = np.linalg.eigh(M)
    return vec, val, S
