"""NumPy restatement of the bundle tools (include/fibers_hip.h, "Bundle tools"), written from the definitions there and from nothing
else: the cumulative lengths are a SEQUENTIAL float64 cumsum of the LINE STATISTICS terms, the segment of a row is
np.searchsorted(c, t, 'right') - 1 capped at n - 2, the MDF sums run over k one element after the other, and the centroid sums are
sequential float64 sums in line order.  Pinned by known answers in tests/test_bundle_ref.py; the GPU results are held to it in
tests/test_gpu_bundle.py."""
import numpy as np

NAN32 = np.array([0x7FC00000], np.uint32).view(np.float32)[0]


def _check(npts, npoints):
    npts = np.asarray(npts, np.int64).reshape(-1)
    if (npts < 0).any() or int(npts.sum()) != npoints:
        raise ValueError("npts must be non-negative and sum to npoints")
    return npts


def _res(volres):
    return np.asarray(volres, np.float32).astype(np.float64)


def seg_lengths(q64, r):
    """l_i of consecutive rows of q64 (float64 copies of float32 points): the term of the str_stats length"""
    u = (q64[1:] - q64[:-1]) * r
    return np.sqrt((u[:, 0] * u[:, 0] + u[:, 1] * u[:, 1]) + u[:, 2] * u[:, 2])


def resample_line(p, K, r):
    """(rows float32 [K, 3], T, n): one line, unflipped"""
    p = np.asarray(p, np.float32).reshape(-1, 3)
    n = p.shape[0]
    out = np.empty((K, 3), np.float32)
    if n == 0:
        out[:] = NAN32
        return out, np.float64(np.nan)
    if n == 1:
        out[:] = p[0]
        return out, np.float64(0)
    q = p.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        l = seg_lengths(q, r)
        c = np.concatenate([[0.0], np.cumsum(l)])                             # sequential: c_{i+1} = c_i + l_i
        T = c[-1]
        if not np.isfinite(T):
            out[:] = NAN32
            return out, T
        k = np.arange(1, K - 1, dtype=np.float64)
        t = (T * k) / np.float64(K - 1)
        j = np.minimum(np.searchsorted(c, t, "right") - 1, n - 2)
        den = c[j + 1] - c[j]
        a = np.where(den > 0, np.clip((t - c[j]) / np.where(den > 0, den, 1.0), 0.0, 1.0), 0.0)
        out[1:K - 1] = (q[j] + a[:, None] * (q[j + 1] - q[j])).astype(np.float32)
    out[0] = p[0]
    out[K - 1] = p[n - 1]
    return out, T


def resample(xyz, npts, volres, K, flip=None):
    """out float32 [nlines, K, 3]"""
    p = np.asarray(xyz, np.float32).reshape(-1, 3)
    npts = _check(npts, p.shape[0])
    r = _res(volres)
    out = np.empty((npts.size, K, 3), np.float32)
    o = 0
    for i, n in enumerate(npts):
        rows, _ = resample_line(p[o:o + n], K, r)
        out[i] = rows[::-1] if flip is not None and flip[i] else rows
        o += int(n)
    return out


def resample_bound(xyz, npts, volres):
    """per line: n * 2^-50 * T / min(r) + 2^-50 * max|p|, the part of the resampling tolerance that does not depend on the value itself
    (NaN where T is not finite)"""
    p = np.asarray(xyz, np.float32).reshape(-1, 3)
    npts = _check(npts, p.shape[0])
    r = _res(volres)
    b = np.zeros(npts.size)
    o = 0
    with np.errstate(invalid="ignore", over="ignore"):
        for i, n in enumerate(npts):
            n = int(n)
            if n >= 2:
                q = p[o:o + n].astype(np.float64)
                T = np.cumsum(seg_lengths(q, r))[-1]
                b[i] = n * 2.0 ** -50 * T / r.min() + 2.0 ** -50 * np.abs(q).max()
            o += n
    return b


def mdf(lines, models, volres):
    """(d float64 [nlines, nmodels], f uint8 [nlines, nmodels]): the MDF distance of every pair and whether the flipped sum won"""
    a = np.asarray(lines, np.float32).astype(np.float64)
    m = np.asarray(models, np.float32).astype(np.float64)
    K = a.shape[1]
    r = _res(volres)
    dd = np.zeros((a.shape[0], m.shape[0]))
    df = np.zeros((a.shape[0], m.shape[0]))
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(K):                                                   # sequential over k, from 0
            for s, mk in ((dd, m[:, k]), (df, m[:, K - 1 - k])):
                u = (a[:, None, k, :] - mk[None, :, :]) * r
                s += np.sqrt((u[..., 0] * u[..., 0] + u[..., 1] * u[..., 1]) + u[..., 2] * u[..., 2])
        dd /= np.float64(K)
        df /= np.float64(K)
        f = df < dd
    return np.where(f, df, dd), f.astype(np.uint8)


def assign(lines, models, volres, thresh, pairs=None):
    """(label int32, dist float32, flip uint8, dist_all float32 [nlines, nmodels]); `pairs`: the result of mdf() on the same arguments"""
    d, f = mdf(lines, models, volres) if pairs is None else pairs
    nl = d.shape[0]
    label = np.full(nl, -1, np.int32)
    dist = np.full(nl, NAN32, np.float32)
    flip = np.zeros(nl, np.uint8)
    th = np.float64(np.float32(thresh))
    for i in range(nl):
        real = np.flatnonzero(~np.isnan(d[i]))                               # a NaN is larger than everything
        if real.size:
            best = real[np.argmin(d[i, real])]                               # np.argmin: the first of equal minima
            dist[i] = np.float32(d[i, best])
            flip[i] = f[i, best]
            if d[i, best] <= th:
                label[i] = best
    with np.errstate(over="ignore"):
        dall = d.astype(np.float32)
    dall[np.isnan(dall)] = NAN32                                             # one NaN, whatever sign and payload the arithmetic left
    return label, dist, flip, dall


def centroids(lines, label, flip, nmodels):
    """(sums float64 [nmodels, K, 3], counts uint32 [nmodels], bound float64 [nmodels, K, 3]): sequential float64 sums in line order and,
    next to each cell, (N_b - 1) * 2^-52 * sum|t|"""
    a = np.asarray(lines, np.float32)
    K = a.shape[1]
    S, A, N = np.zeros((nmodels, K, 3)), np.zeros((nmodels, K, 3)), np.zeros(nmodels, np.int64)
    for i in range(a.shape[0]):
        b = int(label[i])
        if 0 <= b < nmodels:
            row = (a[i, ::-1] if flip is not None and flip[i] else a[i]).astype(np.float64)
            S[b] += row
            A[b] += np.abs(row)
            N[b] += 1
    return S, (N & 0xFFFFFFFF).astype(np.uint32), np.maximum(N - 1, 0)[:, None, None] * 2.0 ** -52 * A


def ulp32(x):
    x = np.abs(np.asarray(x, np.float32))
    with np.errstate(invalid="ignore", over="ignore"):
        return (np.nextafter(x, np.float32(np.inf)) - x).astype(np.float64)
