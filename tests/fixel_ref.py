"""NumPy restatement of the tractogram weights (include/fibers_hip.h, "Tractogram weights"), written from the definitions there and
from nothing else, integer for integer: existence of a fixel, the fixel of a point in float32 (every operation rounded on its own),
uint64 sums (NumPy's wrap as uint64 sums do), the ISRA update in float64 in the order the header writes it.  Pinned by hand-derived
answers in tests/test_fixel_ref.py; the GPU results are held to it bit for bit in tests/test_gpu_fixel.py (cost: within the bound)."""
import math

import numpy as np

from tractmap_ref import voxel

Q_ONE = 1 << 20
Q_CLAMP = (1 << 32) - 1
TD_LIMIT = 1 << 44
F32 = np.float32


def cos2_of(ang_deg):
    return F32(math.cos(math.radians(float(ang_deg))) ** 2)


def _planar(ovec, f, shape):
    """ovec[k] -> float32 [3, nvox], f[k] -> float32 [nvox] (x fastest)"""
    nvox = int(shape[0]) * int(shape[1]) * int(shape[2])
    return [np.asarray(o, F32).reshape(3, nvox) for o in ovec], [np.asarray(a, F32).reshape(nvox) for a in f]


def exists(ovec, f, mask, f_thresh, shape):
    """bool [nvec, nvox]"""
    ov, fs = _planar(ovec, f, shape)
    nvox = fs[0].size
    m = np.ones(nvox, bool) if mask is None else (np.asarray(mask).reshape(nvox) != 0)
    out = np.zeros((len(ov), nvox), bool)
    with np.errstate(invalid="ignore"):
        for k in range(len(ov)):
            out[k] = m & np.isfinite(fs[k]) & (fs[k] > F32(f_thresh)) & np.isfinite(ov[k]).all(axis=0) & (ov[k] != 0).any(axis=0)
    return out


def assign(xyz, npts, shape, ovec, f, mask, f_thresh, cos2):
    """(ids int32 [npoints], points unassigned, lines without an assigned point)"""
    p = np.asarray(xyz, F32).reshape(-1, 3)
    npts = np.asarray(npts, np.int64).reshape(-1)
    if (npts < 0).any() or int(npts.sum()) != p.shape[0]:
        raise ValueError("npts must be non-negative and sum to npoints")
    ov, fs = _planar(ovec, f, shape)
    nvox = fs[0].size
    ex = exists(ovec, f, mask, f_thresh, shape)
    lin = voxel(p, shape)
    ids = np.full(p.shape[0], -1, np.int32)
    cos2 = F32(cos2)
    lines_without = 0
    o = 0
    with np.errstate(invalid="ignore", over="ignore"):
        for n in npts:
            n = int(n)
            got = 0
            if n >= 2:
                q = p[o:o + n]
                t = np.empty_like(q)
                t[1:-1] = q[2:] - q[:-2]
                t[0] = q[1] - q[0]
                t[-1] = q[-1] - q[-2]
                for i in range(n):
                    v = int(lin[o + i])
                    tx, ty, tz = t[i]
                    if v < 0 or not (np.isfinite(tx) and np.isfinite(ty) and np.isfinite(tz)) or (tx == 0 and ty == 0 and tz == 0):
                        continue
                    best, bd, bk = F32(-1), F32(0), -1
                    for k in range(len(ov)):
                        if not ex[k, v]:
                            continue
                        d = F32(F32(F32(tx * ov[k][0, v]) + F32(ty * ov[k][1, v])) + F32(tz * ov[k][2, v]))
                        if np.abs(d) > best:
                            best, bd, bk = np.abs(d), d, k
                    if bk < 0:
                        continue
                    tt = F32(F32(F32(tx * tx) + F32(ty * ty)) + F32(tz * tz))
                    if F32(bd * bd) >= F32(cos2 * tt):
                        ids[o + i] = bk * nvox + v
                        got += 1
            lines_without += got == 0
            o += n
    return ids, int((ids < 0).sum()), int(lines_without)


def quantise(ovec, f, mask, f_thresh, shape):
    """(Aq uint64 [nvec * nvox], a_scale float64, sum Aq)"""
    _, fs = _planar(ovec, f, shape)
    ex = exists(ovec, f, mask, f_thresh, shape)
    fall = np.stack(fs)
    if not ex.any():
        return np.zeros(fall.size, np.uint64), 0.0, 0
    a_scale = np.float64(2.0 ** 30) / np.float64(fall[ex].max())
    aq = np.zeros(fall.shape, np.uint64)
    aq[ex] = np.rint(fall[ex].astype(np.float64) * a_scale).astype(np.uint64)
    return aq.reshape(-1), float(a_scale), int(aq.sum(dtype=np.uint64))


def track_density(ids, npts, q, nfix):
    """TDq uint64 [nfix]"""
    npts = np.asarray(npts, np.int64).reshape(-1)
    w = np.repeat(np.asarray(q, np.uint64), npts)
    td = np.zeros(nfix, np.uint64)
    ok = ids >= 0
    np.add.at(td, ids[ok], w[ok])
    return td


def line_sums(ids, npts, values):
    """uint64 [nlines]: the sum of values[ids] over every line's assigned points; and the number of those points"""
    npts = np.asarray(npts, np.int64).reshape(-1)
    line = np.repeat(np.arange(npts.size), npts)
    ok = ids >= 0
    s = np.zeros(npts.size, np.uint64)
    np.add.at(s, line[ok], values[ids[ok]])
    return s, np.bincount(line[ok], minlength=npts.size)


def cost_terms(aq, td, mu, a_scale):
    x = np.float64(mu) * (td.astype(np.float64) * 2.0 ** -20)
    with np.errstate(invalid="ignore", divide="ignore"):
        y = np.where(aq > 0, aq.astype(np.float64) / np.float64(a_scale), 0.0)
    r = x - y
    return r * r


def weights(xyz, npts, shape, ovec, f, mask=None, f_thresh=0.03, cos2=None, niter=50, q0=None):
    """the whole fit: a dict with ids, q, weights, td [nvec, nvox], mu, a_scale, cost (math.fsum: the exact sum rounded once),
    cost_bound (n * 2^-53 * sum|t| per entry), counts (the five of the header) and tdq"""
    cos2 = cos2_of(45) if cos2 is None else F32(cos2)
    npts = np.asarray(npts, np.int64).reshape(-1)
    nvec = len(ovec)
    nvox = int(shape[0]) * int(shape[1]) * int(shape[2])
    nfix = nvec * nvox
    ids, n_un, n_without = assign(xyz, npts, shape, ovec, f, mask, f_thresh, cos2)
    aq, a_scale, sum_aq = quantise(ovec, f, mask, f_thresh, shape)
    q = np.full(npts.size, Q_ONE, np.uint32) if q0 is None else np.asarray(q0, np.uint32).copy()
    td = track_density(ids, npts, q, nfix)
    sum_td0 = int(td.sum(dtype=np.uint64))
    mu = 0.0
    if a_scale > 0 and sum_td0:
        mu = float((np.float64(sum_aq) / np.float64(a_scale)) / (np.float64(sum_td0) * 2.0 ** -20))
    cost, bound = [], []

    def add_cost():
        t = cost_terms(aq, td, mu, a_scale)
        cost.append(math.fsum(t))
        bound.append(t.size * 2.0 ** -53 * float(np.abs(t).sum()))

    add_cost()
    N, nassigned = line_sums(ids, npts, aq)
    overflow = 0
    for _ in range(int(niter)):
        D, _n = line_sums(ids, npts, td)
        overflow += int((td[ids[ids >= 0]] >= np.uint64(TD_LIMIT)).sum())
        live = (nassigned > 0) & (D != 0)
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            w = q.astype(np.float64) * 2.0 ** -20
            A = N.astype(np.float64) / np.float64(a_scale)
            B = D.astype(np.float64) * 2.0 ** -20
            C = np.float64(mu) * B
            wn = (w * A) / C
            qn = np.rint(np.minimum(wn, 4096.0 - 2.0 ** -20) * 2.0 ** 20)
        q = np.where(live, qn, 0.0).astype(np.uint32)
        td = track_density(ids, npts, q, nfix)
        add_cost()
    out_td = ((td.astype(np.float64) * 2.0 ** -20) * np.float64(mu)).astype(F32).reshape(nvec, nvox)
    counts = (n_un, n_without, int((q == Q_CLAMP).sum()), int((q == 0).sum()), overflow)
    return dict(ids=ids, q=q, weights=(q.astype(F32) * F32(2.0 ** -20)), td=out_td, mu=mu, a_scale=a_scale, cost=np.array(cost), cost_bound=np.array(bound),
                counts=counts, tdq=td, aq=aq)


def connectome_loop(assign_pairs, w, nnodes):
    """the weighted matrix, one line after the other"""
    W = np.zeros((nnodes + 1, nnodes + 1), np.float64)
    for (a, b), x in zip(np.asarray(assign_pairs).reshape(-1, 2), np.asarray(w, np.float64)):
        i, j = min(int(a), int(b)), max(int(a), int(b))
        W[i, j] += x
        if i != j:
            W[j, i] += x
    return W
