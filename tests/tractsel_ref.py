"""NumPy restatement of tract selection and connectomes (include/fibers_hip.h, "Tract selection and connectomes"), written from the
definitions there and from nothing else: plain loops over the lines, the voxel of a point and the inside test taken from
tests/tractmap_ref.py, every float64 sum SEQUENTIAL.  Pinned by hand-counted answers in tests/test_tractsel_ref.py; the GPU results
are held to it in tests/test_gpu_tractsel.py."""
import numpy as np

from tractmap_ref import _check, _seq_sum, voxel

U32 = 0xFFFFFFFF


def roi_pack(rois):
    """roibits uint32 [nvox] from rois [nroi, nvox] (any dtype): bit r is set iff ROI r is non-zero"""
    rois = np.asarray(rois)
    assert rois.ndim == 2 and rois.shape[0] <= 32
    bits = np.zeros(rois.shape[1], np.uint32)
    for r in range(rois.shape[0]):
        bits |= (rois[r] != 0).astype(np.uint32) << np.uint32(r)
    return bits


def hits(xyz, npts, shape, roibits):
    """uint32 [nlines, 3] = {visit, end0, end1} of every line"""
    p = np.asarray(xyz, np.float32).reshape(-1, 3)
    npts = _check(npts, p.shape[0])
    roibits = np.asarray(roibits, np.uint32).reshape(-1)
    lin = voxel(p, shape)
    h = np.zeros((npts.size, 3), np.uint32)
    o = 0
    for l, n in enumerate(npts):
        n = int(n)
        if n:
            v = lin[o:o + n]
            h[l] = (np.bitwise_or.reduce(roibits[v[v >= 0]], initial=0), roibits[v[0]] if v[0] >= 0 else 0, roibits[v[-1]] if v[-1] >= 0 else 0)
        o += n
    return h


def rule(h, npts, visit_all=0, visit_none=0, end_any=0, end_both=0, min_npts=0, max_npts=0):
    """keep uint8 [nlines] from the predicates and the point counts"""
    keep = np.zeros(len(npts), np.uint8)
    for l, n in enumerate(npts):
        v, e0, e1 = (int(x) for x in h[l])
        keep[l] = ((v & visit_all) == visit_all and (v & visit_none) == 0 and ((e0 | e1) & end_any) == end_any
                   and (e0 & e1 & end_both) == end_both and min_npts <= n and (max_npts == 0 or n <= max_npts))
    return keep


def select(xyz, npts, shape, roibits, **kw):
    """(keep uint8 [nlines], hits uint32 [nlines, 3], counts [kept lines, kept points])"""
    h = hits(xyz, npts, shape, roibits)
    n = np.asarray(npts, np.int64).reshape(-1)
    keep = rule(h, n, **kw)
    return keep, h, [int(keep.sum()), int(n[keep != 0].sum())]


def gather(xyz, npts, keep, scalars=None):
    """(xyz_out, npts_out int32, index_out int64, scalars_out or None): the lines with keep != 0, in input order, as copies"""
    p = np.asarray(xyz, np.float32).reshape(-1, 3)
    npts = _check(npts, p.shape[0])
    off = np.concatenate([[0], np.cumsum(npts)])
    idx = [l for l in range(npts.size) if keep[l] != 0]
    rows = np.concatenate([np.arange(off[l], off[l + 1]) for l in idx]) if idx else np.zeros(0, np.int64)
    sc = None if scalars is None else np.asarray(scalars, np.float32).reshape(p.shape[0], -1)[rows]
    return p[rows], npts[idx].astype(np.int32), np.asarray(idx, np.int64), sc


def node(lin, labels, remap, L):
    """node of a line end whose voxel index is lin (-1: outside)"""
    if lin < 0:
        return 0
    y = int(labels[lin])
    if remap is not None:
        y = int(remap[y]) if 0 <= y < len(remap) else 0
    return y if 1 <= y <= L else 0


def length64(q, r64):
    """the LINE STATISTICS column-0 sum of q float64 [n, 3], kept in float64; and its terms"""
    if q.shape[0] < 2:
        return np.float64(0), np.zeros(0)
    with np.errstate(invalid="ignore", over="ignore"):
        u = (q[1:] - q[:-1]) * r64
        t = np.sqrt((u[:, 0] * u[:, 0] + u[:, 1] * u[:, 1]) + u[:, 2] * u[:, 2])
        return _seq_sum(t), t


def connectome(xyz, npts, shape, labels, L, remap=None, volres=None, into=None):
    """(C uint32 [L+1, L+1], W float64 [L+1, L+1] or None (volres None), assign int32 [nlines, 2], n_lines, bound float64 [L+1, L+1]):
    `into` = (C, W) to accumulate into (copies are returned).  bound is the derived tolerance of a cell, (n_max + m) * 2^-52 * W."""
    p = np.asarray(xyz, np.float32).reshape(-1, 3)
    npts = _check(npts, p.shape[0])
    labels = np.asarray(labels, np.int32).reshape(-1)
    lin = voxel(p, shape)
    C = np.zeros((L + 1, L + 1), np.uint64) if into is None else np.asarray(into[0], np.uint32).astype(np.uint64)
    W = None if volres is None else (np.zeros((L + 1, L + 1), np.float64) if into is None else np.array(into[1], np.float64))
    nmax = np.zeros((L + 1, L + 1), np.int64)
    assign = np.zeros((npts.size, 2), np.int32)
    r64 = None if volres is None else np.asarray(volres, np.float32).astype(np.float64)
    p64 = p.astype(np.float64)
    o = count = 0
    with np.errstate(invalid="ignore", over="ignore"):
        for l, n in enumerate(npts):
            n = int(n)
            if n >= 1:
                a, b = node(lin[o], labels, remap, L), node(lin[o + n - 1], labels, remap, L)
                i, j = min(a, b), max(a, b)
                assign[l] = (a, b)
                count += 1
                C[i, j] += 1
                if i != j:
                    C[j, i] += 1
                if W is not None:
                    ln = length64(p64[o:o + n], r64)[0]
                    W[i, j] = W[i, j] + ln
                    nmax[i, j] = max(nmax[i, j], n)
                    if i != j:
                        W[j, i] = W[j, i] + ln
                        nmax[j, i] = max(nmax[j, i], n)
            o += n
        Cu = (C & np.uint64(U32)).astype(np.uint32)
        bound = None if W is None else (nmax + Cu.astype(np.int64)) * 2.0 ** -52 * W
    return Cu, W, assign, count, bound


def mean_length(C, W):
    """W / C where C > 0, else 0"""
    out = np.zeros(W.shape, np.float64)
    np.divide(W, C, out=out, where=C > 0)
    return out


def weights_close(got, ref, bound, C):
    """per cell: |got - ref| <= bound where ref is finite; NaN matches NaN and Inf the same Inf (a non-finite length makes the cell
    non-finite in any order of summation: lengths are >= 0 or NaN); cells with C == 0 are exactly 0"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    with np.errstate(invalid="ignore"):
        ok = np.abs(got - ref) <= bound
    special = (np.isnan(ref) & np.isnan(got)) | (np.isinf(ref) & (got == ref))
    ok = np.where(np.isfinite(ref), ok, special)
    return np.where(np.asarray(C) == 0, got == 0, ok)
