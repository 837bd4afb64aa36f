"""NumPy restatement of the tract maps (include/fibers_hip.h, "Tract maps"), written from the definitions there and from nothing else:
the voxel of a point is np.rint (ties to even) with the inside test made on the float value; the maps are counts over voxels /
(line, voxel) pairs; a sample is a fancy index; the statistics are SEQUENTIAL float64 sums rounded to float32 once.  Pinned by
hand-counted answers in tests/test_tractmap_ref.py; the GPU results are held to it in tests/test_gpu_tractmap.py."""
import numpy as np

POINTS, LINES, ENDPOINTS = 0, 1, 2


def voxel(xyz, shape):
    """linear voxel index (int64, x fastest) of every point, -1 where the point is not inside"""
    p = np.asarray(xyz, np.float32).reshape(-1, 3)
    nx, ny, nz = (int(v) for v in shape)
    with np.errstate(invalid="ignore"):
        v = np.rint(p)                                                        # float32, ties to even
        inside = ((v[:, 0] >= 1) & (v[:, 0] <= nx) & (v[:, 1] >= 1) & (v[:, 1] <= ny) & (v[:, 2] >= 1) & (v[:, 2] <= nz))   # NaN: False
    w = np.where(inside[:, None], v, 1).astype(np.int64)
    lin = (w[:, 0] - 1) + nx * ((w[:, 1] - 1) + ny * (w[:, 2] - 1))
    return np.where(inside, lin, -1)


def _check(npts, npoints):
    npts = np.asarray(npts, np.int64).reshape(-1)
    if (npts < 0).any() or int(npts.sum()) != npoints:
        raise ValueError("npts must be non-negative and sum to npoints")
    return npts


def density(xyz, npts, shape, mode, into=None):
    """(D uint32 [nvox], n_outside); `into`: accumulate (a copy is returned)"""
    p = np.asarray(xyz, np.float32).reshape(-1, 3)
    npts = _check(npts, p.shape[0])
    nvox = int(shape[0]) * int(shape[1]) * int(shape[2])
    lin = voxel(p, shape)
    if mode == POINTS:
        add = np.bincount(lin[lin >= 0], minlength=nvox)
        nout = int((lin < 0).sum())
    elif mode == LINES:
        line = np.repeat(np.arange(npts.size, dtype=np.int64), npts)
        pairs = np.unique(line[lin >= 0] * nvox + lin[lin >= 0])             # each (line, voxel) pair once
        add = np.bincount(pairs % nvox, minlength=nvox)
        nout = int((lin < 0).sum())
    elif mode == ENDPOINTS:
        off = np.concatenate([[0], np.cumsum(npts)])
        has = npts >= 1
        ends = lin[np.concatenate([off[:-1][has], off[1:][has] - 1])]       # first and last point of every non-empty line
        add = np.bincount(ends[ends >= 0], minlength=nvox)
        nout = int((ends < 0).sum())
    else:
        raise ValueError("mode")
    d = np.zeros(nvox, np.uint64) if into is None else np.asarray(into, np.uint32).reshape(-1).astype(np.uint64)
    return ((d + add.astype(np.uint64)) & np.uint64(0xFFFFFFFF)).astype(np.uint32), nout


def sample(xyz, vol, shape, outside=0.0):
    """S float32 [npoints, nframes]; vol planar [nframes, nvox]"""
    nvox = int(shape[0]) * int(shape[1]) * int(shape[2])
    vol = np.asarray(vol, np.float32).reshape(-1, nvox)
    lin = voxel(xyz, shape)
    s = np.full((lin.size, vol.shape[0]), np.float32(outside), np.float32)
    s[lin >= 0] = vol[:, lin[lin >= 0]].T
    return s


def _seq_sum(t):
    """((t0 + t1) + t2) + ... in float64: np.cumsum accumulates one element after the other (np.sum would add pairwise)"""
    return np.cumsum(np.asarray(t, np.float64))[-1] if len(t) else np.float64(0)


def stats(xyz, npts, volres, scalars=None):
    """(P float32 [nlines, 1 + ns], bound float64 [nlines, 1 + ns]): the sequential float64 results rounded once, and next to each the
    term of the tolerance that comes from the freedom of the summation order, n * 2^-52 * sum|t_i| / d (the header's bound with its
    factor doubled: the derived tolerance of the tests)"""
    p = np.asarray(xyz, np.float32).reshape(-1, 3)
    npts = _check(npts, p.shape[0])
    sc = np.zeros((p.shape[0], 0), np.float32) if scalars is None else np.asarray(scalars, np.float32).reshape(p.shape[0], -1)
    r = np.asarray(volres, np.float32).astype(np.float64)
    ns = sc.shape[1]
    P = np.zeros((npts.size, 1 + ns), np.float32)
    B = np.zeros((npts.size, 1 + ns), np.float64)
    p64, s64 = p.astype(np.float64), sc.astype(np.float64)
    o = 0
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for l, n in enumerate(npts):
            n = int(n)
            q = p64[o:o + n]
            if n >= 2:
                u = (q[1:] - q[:-1]) * r
                t = np.sqrt((u[:, 0] * u[:, 0] + u[:, 1] * u[:, 1]) + u[:, 2] * u[:, 2])
                P[l, 0] = np.float32(_seq_sum(t))
                B[l, 0] = t.size * 2.0 ** -52 * np.abs(t).sum()
            for c in range(ns):
                P[l, 1 + c] = np.float32(_seq_sum(s64[o:o + n, c]) / np.float64(n)) if n else np.float32(np.nan)
                B[l, 1 + c] = n * 2.0 ** -52 * np.abs(s64[o:o + n, c]).sum() / n if n else 0.0
            o += n
    return P, B


def ulp32(x):
    """the float32 ulp at |x| (spacing to the next float32 away from zero); NaN / Inf -> NaN"""
    x = np.abs(np.asarray(x, np.float32))
    with np.errstate(invalid="ignore", over="ignore"):
        return (np.nextafter(x, np.float32(np.inf)) - x).astype(np.float64)


def stats_close(got, ref, bound):
    """|got - ref| <= ulp32(ref) + bound, NaN matching NaN and Inf matching Inf: the derived tolerance, element by element"""
    got, ref = np.asarray(got, np.float32), np.asarray(ref, np.float32)
    same_special = (np.isnan(ref) & np.isnan(got)) | (np.isinf(ref) & (got == ref))
    with np.errstate(invalid="ignore"):
        ok = np.abs(got.astype(np.float64) - ref.astype(np.float64)) <= ulp32(ref) + bound
    return np.where(np.isfinite(ref), ok, same_special)
