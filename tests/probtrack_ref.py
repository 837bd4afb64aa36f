"""NumPy restatement of probabilistic ODF tracking (include/fibers_hip.h, "Probabilistic tracking"): the weight table,
the cone, the generator and the lines.  Python integers for the generator, np.float32 with one rounding per operation elsewhere, integer
sums.  `trace` runs all lines side by side, one step of every live line per iteration; tests/test_probtrack_ref.py holds it to a scalar
transcription of the definition.  `mutant` switches in one deliberate error (the mutants of DESIGN.md §5), for the tests of the tests."""
import numpy as np

M64 = (1 << 64) - 1
F32 = np.float32
MUTANTS = ("fma", "floor", "draw_first", "allow_gt", "same_row")


def splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def h32(rng_seed, line, k):
    """h(line, k) >> 32 in Python integers"""
    return splitmix64((rng_seed & M64) ^ splitmix64((line * 0xD1342543DE82EF95 + k) & M64)) >> 32


def _splitmix64_v(x):
    x = x + np.uint64(0x9E3779B97F4A7C15)
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def h32_v(rng_seed, line, k):
    """h32 for arrays of lines and draw counters (uint64 arithmetic wraps like the definition's)"""
    with np.errstate(over="ignore"):
        x = np.asarray(line, np.uint64) * np.uint64(0xD1342543DE82EF95) + np.asarray(k, np.uint64)
        return _splitmix64_v(np.uint64(rng_seed & M64) ^ _splitmix64_v(x)) >> np.uint64(32)


def row_pitch(nvert):
    return 64 * ((nvert + 63) // 64)


def table(odf, mask=None, subtract_min=True, pmf_thresh=0.1):
    """odf float32 [nvert, nvox] planar, mask [nvox] or None -> uint16 [nvox, pitch]"""
    o = np.asarray(odf, F32)
    nvert, nvox = o.shape
    with np.errstate(all="ignore"):
        m = np.fmin.reduce(o, axis=0) if subtract_min else np.zeros(nvox, F32)      # (fmin drops a NaN)
        w = o - m[None, :]
        w = np.where(w > 0, w, F32(0)).astype(F32)
        wmax = w.max(axis=0)
        live = (wmax > 0) & np.isfinite(wmax)
        if mask is not None:
            live &= np.asarray(mask).reshape(-1) != 0
        t = (w / wmax[None, :]).astype(F32)
        q = np.floor(t * F32(65535.0))
        q = np.where(t < F32(pmf_thresh), 0, q)
        q = np.where(live[None, :], q, 0)
    out = np.zeros((nvox, row_pitch(nvert)), np.uint16)
    out[:, :nvert] = q.T.astype(np.uint16)
    return out


def cone(U, cosang_thresh, mutant=None):
    """(allow, same) bool [nvert, nvert]"""
    U = np.asarray(U, F32)
    x, y, z = U[:, 0], U[:, 1], U[:, 2]
    c = (x[:, None] * x[None, :] + y[:, None] * y[None, :]) + z[:, None] * z[None, :]
    assert c.dtype == np.float32
    a = np.abs(c)
    allow = a > F32(cosang_thresh) if mutant == "allow_gt" else a >= F32(cosang_thresh)
    return allow, c > 0


def step_point(pos, vec, step, mutant=None):
    """nxt = pos + vec * step: multiply, then add, each rounded to float32"""
    if mutant == "fma":
        return (pos.astype(np.float64) + vec.astype(np.float64) * np.float64(F32(step))).astype(F32)
    return pos + vec * F32(step)


def voxel_of(nxt, mutant=None):
    with np.errstate(invalid="ignore"):
        return np.floor(nxt + F32(0.5)) if mutant == "floor" else np.rint(nxt)


def draw(q, u):
    """q int64 [n, nvert] with positive row sums, u uint64 [n] -> the picks"""
    cs = np.cumsum(q, axis=1)
    r = (u * cs[:, -1].astype(np.uint64)) >> np.uint64(32)
    return np.argmax(cs > r.astype(np.int64)[:, None], axis=1)


def trace(tab, U, cosang_thresh, shape, seeds, sublist, len_min=3, len_max=None, step_size=0.5, rng_seed=0, mutant=None):
    """-> dict(npts int32 [nlines], seed_index int64 [nlines], xyz float32 [npoints, 3], all_counts int32 [nseed * nsub, 2])"""
    if not F32(cosang_thresh) > 0:
        raise ValueError("cosang_thresh must be > 0 (an angle below 90 degrees)")
    U = np.asarray(U, F32)
    nvert = U.shape[0]
    nx, ny, nz = (int(v) for v in shape)
    nvox = nx * ny * nz
    len_max = max(shape) if len_max is None else int(len_max)
    allow, same = cone(U, cosang_thresh, mutant)
    W = np.asarray(tab)[:, :nvert].astype(np.int64)
    seeds = np.asarray(seeds, np.int64).reshape(-1)
    sub = np.asarray(sublist, F32).reshape(-1, 3)
    nsub, nl = sub.shape[0], seeds.size * sub.shape[0]
    line = np.arange(nl, dtype=np.int64)
    sd = seeds[line // nsub]
    inside = (sd >= 0) & (sd < nvox)
    sdc = np.where(inside, sd, 0)
    sv = np.stack([sdc % nx + 1, (sdc // nx) % ny + 1, sdc // (nx * ny) + 1], axis=1).astype(F32)
    pos0 = sv + sub[line % nsub]
    alive = inside & (W[sdc].sum(axis=1) > 0)
    j0 = np.zeros(nl, np.int64)
    ia = np.nonzero(alive)[0]
    if ia.size:
        j0[ia] = draw(W[sdc[ia]], h32_v(rng_seed, ia, 0))
    k = np.ones(nl, np.int64)
    npts = np.zeros(nl, np.int64)
    pts = [np.zeros((nl, len_max + 2, 3), F32), np.zeros((nl, len_max + 2, 3), F32)]
    cnt = [np.zeros(nl, np.int64), np.zeros(nl, np.int64)]
    for d, s0 in enumerate((1.0, -1.0)):
        pos, j, s, act = pos0.copy(), j0.copy(), np.full(nl, s0, F32), alive.copy()
        while act.any():
            ia = np.nonzero(act)[0]
            vec = s[ia, None] * U[j[ia]]
            nxt = step_point(pos[ia], vec, step_size, mutant)
            v = voxel_of(nxt, mutant)
            with np.errstate(invalid="ignore"):
                ok = np.isfinite(nxt).all(axis=1) & (v >= 1).all(axis=1) & (v[:, 0] <= nx) & (v[:, 1] <= ny) & (v[:, 2] <= nz)
            act[ia[~ok]] = False
            ia, nxt, v = ia[ok], nxt[ok], v[ok].astype(np.int64)
            lin = (v[:, 0] - 1) + nx * ((v[:, 1] - 1) + ny * (v[:, 2] - 1))
            q = W[lin] * allow[j[ia]]
            if mutant == "draw_first":
                k[ia] += 1
            has = q.sum(axis=1) > 0
            act[ia[~has]] = False
            ia, nxt, q = ia[has], nxt[has], q[has]
            if not ia.size:
                continue
            kk = k[ia] - 1 if mutant == "draw_first" else k[ia]
            pick = draw(q, h32_v(rng_seed, ia, kk))
            if mutant != "draw_first":
                k[ia] += 1
            keep = same[pick, pick] if mutant == "same_row" else same[j[ia], pick]
            s[ia] = np.where(keep, s[ia], -s[ia])
            j[ia] = pick
            pts[d][ia, cnt[d][ia]] = pos[ia]
            cnt[d][ia] += 1
            npts[ia] += 1
            act[ia[npts[ia] > len_max]] = False
            pos[ia] = nxt
    kept = np.nonzero(npts >= len_min)[0]
    xyz = []
    for i in kept:
        xyz.append(pts[0][i, :cnt[0][i]][::-1])
        xyz.append(pts[1][i, :cnt[1][i]])
    return dict(npts=npts[kept].astype(np.int32), seed_index=kept.astype(np.int64),
                xyz=np.concatenate(xyz).astype(F32) if xyz else np.zeros((0, 3), F32),
                all_counts=np.stack([cnt[0], cnt[1]], axis=1).astype(np.int32))
