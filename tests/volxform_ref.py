"""NumPy restatement of the volume resampling contract ("Volume resampling", include/fibers_hip.h), independent of the package:
float32 element-wise, every multiply and add rounded on its own, in the contract's order.  Volumes are [nframes, nz, ny, nx] (x
fastest: the planar layout of the C ABI, C-ordered here); voxel coordinates are 0-based array indices.  `M` is the OUTPUT -> INPUT
matrix, float32 [4, 4]."""
import numpy as np

F = np.float32


def pull_back(M, outshape):
    """p = xfm_point(M, i, j, k) for every output voxel: three float32 arrays [nzo, nyo, nxo]"""
    m = np.asarray(M, F).reshape(4, 4)
    nx, ny, nz = outshape
    k, j, i = np.meshgrid(np.arange(nz, dtype=F), np.arange(ny, dtype=F), np.arange(nx, dtype=F), indexing="ij")
    with np.errstate(all="ignore"):
        aff = F(0) + m[3, 0] * i
        aff = aff + m[3, 1] * j
        aff = aff + m[3, 2] * k
        aff = aff + m[3, 3]
        p = []
        for r in range(3):
            lin = F(0) + m[r, 0] * i
            lin = lin + m[r, 1] * j
            lin = lin + m[r, 2] * k
            lin = lin + m[r, 3]
            p.append((lin / aff).astype(F))
    return p


def inside_mask(p, inshape):
    """0 <= rint(p_c) <= n_c - 1 for every component, on the float values (NaN fails, -0.0 passes)"""
    ok = np.ones(p[0].shape, bool)
    with np.errstate(invalid="ignore"):
        for c in range(3):
            r = np.rint(p[c])
            ok &= (r >= F(0)) & (r <= F(inshape[c] - 1))
    return ok


def vol_xform_ref(M, vol, inshape, outshape, interp, outside):
    """vol [nframes, nzi, nyi, nxi] (or [nzi, nyi, nxi]) of a 32-bit element type -> [nframes, nzo, nyo, nxo] in the same type;
    `outside` is a value of that type (its bit pattern is the fill)."""
    vol = np.ascontiguousarray(vol)
    assert vol.dtype.itemsize == 4
    nxi, nyi, nzi = inshape
    v = vol.reshape(-1, nzi, nyi, nxi)
    p = pull_back(M, outshape)
    ok = inside_mask(p, inshape)
    fill = np.array([outside]).astype(vol.dtype).view(np.uint32)[0]
    out = np.empty((v.shape[0],) + p[0].shape, np.uint32)
    if interp == "nearest":
        with np.errstate(invalid="ignore"):
            ix, iy, iz = (np.where(ok, np.rint(c), F(0)).astype(np.int64) for c in p)
        w = v.view(np.uint32)
        for f in range(v.shape[0]):
            out[f] = np.where(ok, w[f][iz, iy, ix], fill)
        return out.view(vol.dtype)
    assert interp == "trilinear" and vol.dtype == F
    lo, hi, fr, gr = [], [], [], []
    for c, n in zip(p, inshape):
        with np.errstate(invalid="ignore"):
            fl = np.floor(c)
            f = (c - fl).astype(F)
            i0 = np.where(ok, fl, F(0)).astype(np.int64)
        lo.append(np.clip(i0, 0, n - 1))
        hi.append(np.clip(i0 + 1, 0, n - 1))
        fr.append(f)
        gr.append((F(1) - f).astype(F))
    (x0, y0, z0), (x1, y1, z1), (fx, fy, fz), (gx, gy, gz) = lo, hi, fr, gr
    with np.errstate(all="ignore"):
        for f in range(v.shape[0]):
            a = v[f]
            c00 = gx * a[z0, y0, x0] + fx * a[z0, y0, x1]
            c10 = gx * a[z0, y1, x0] + fx * a[z0, y1, x1]
            c01 = gx * a[z1, y0, x0] + fx * a[z1, y0, x1]
            c11 = gx * a[z1, y1, x0] + fx * a[z1, y1, x1]
            c0 = gy * c00 + fy * c10
            c1 = gy * c01 + fy * c11
            res = (gz * c0 + fz * c1).astype(F)
            out[f] = np.where(ok, res.view(np.uint32), fill)
    return out.view(F)


def oblique(inshape=None):
    """the tests' oblique input -> output vox2vox: rotations of 20 deg about z and 10 deg about x, scale 1.25, shift (1.5, -0.75, 0.4)"""
    az, ax = np.deg2rad(20.0), np.deg2rad(10.0)
    Rz = np.array([[np.cos(az), -np.sin(az), 0], [np.sin(az), np.cos(az), 0], [0, 0, 1]])
    Rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
    A = np.eye(4)
    A[:3, :3] = 1.25 * (Rz @ Rx)
    A[:3, 3] = (1.5, -0.75, 0.4)
    return A.astype(F)


def out2in(vox2vox):
    """float32(inv(float64(vox2vox))), rounded once: the rule of the Python layer, restated"""
    return np.linalg.inv(np.asarray(vox2vox, F).astype(np.float64)).astype(F)
