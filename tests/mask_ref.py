"""NumPy restatement of the brain mask section of include/fibers_hip.h (dwi_mask, vol_median, mask_components), for the tests.
Volumes are NumPy arrays indexed [x, y, z] (the linear index x + nx (y + ny z) is Fortran order).  Everything is key-based: the median
is a sort of stacked clamped-shift views of the keys, Otsu is the int64 form, components are a flood fill."""
import numpy as np

KEEP_LARGEST, FILL_HOLES = 1, 2


def key(a):
    """float32 array -> the ordered-uint key of each bit pattern"""
    b = np.ascontiguousarray(a, np.float32).view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def unkey(k):
    k = np.ascontiguousarray(k, np.uint32)
    return np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32).view(np.float32)


def mean_frames(vol4, frames):
    """float64 sequential sum in the list's order, one division, one rounding"""
    acc = np.zeros(vol4.shape[:3], np.float64)
    for f in frames:
        acc = acc + vol4[..., int(f)].astype(np.float64)
    return (acc / np.float64(len(frames))).astype(np.float32)


def _shifted(a, axis, d):
    n = a.shape[axis]
    return np.take(a, np.clip(np.arange(n) + d, 0, n - 1), axis=axis)


def median(vol, radius, numpass=1):
    k = key(vol)
    w = range(-radius, radius + 1)
    for _ in range(numpass):
        views = [_shifted(_shifted(_shifted(k, 0, dx), 1, dy), 2, dz) for dz in w for dy in w for dx in w]
        k = np.sort(np.stack(views), axis=0)[len(views) // 2]
    return unkey(k).reshape(vol.shape)


def finite_range(vol):
    """(lo, hi) as float32 scalars chosen by key among the finite values, or None"""
    v = np.asarray(vol, np.float32).reshape(-1)
    v = v[np.isfinite(v)]
    if v.size == 0:
        return None
    k = key(v)
    return unkey(k.min().reshape(1))[0], unkey(k.max().reshape(1))[0]


def bins(vol, lo, hi):
    """bin of every voxel (-1: non-finite)"""
    v = np.asarray(vol, np.float32)
    fin = np.isfinite(v)
    with np.errstate(invalid="ignore", over="ignore"):
        t = (v.astype(np.float64) - np.float64(lo)) / (np.float64(hi) - np.float64(lo)) * 256.0
        b = np.minimum(255, np.floor(np.where(fin, t, 0.0)).astype(np.int64))
    return np.where(fin, b, -1)


def otsu(h):
    """k* (the first maximum of the int64 criterion) of 256 counts, or -1 when no candidate exists"""
    h = np.asarray(h, np.int64)
    j = np.arange(256, dtype=np.int64)
    c0, s0 = np.cumsum(h)[:255], np.cumsum(j * h)[:255]
    c1, s1 = h.sum() - c0, (j * h).sum() - s0
    ok = (c0 > 0) & (c1 > 0)
    if not ok.any():
        return -1
    d = s0 * c1 - s1 * c0
    with np.errstate(invalid="ignore", divide="ignore"):
        crit = (d.astype(np.float64) * d.astype(np.float64)) / (c0.astype(np.float64) * c1.astype(np.float64))
    crit = np.where(ok, crit, -1.0)
    return int(np.argmax(crit))                              # (argmax: the first maximum)


def components(m):
    """int32 canonical labels (1 + smallest linear index, x fastest) of the 6-connected components of m != 0: a flood fill in the
    order of the linear index, so the first voxel met of a component is its smallest"""
    m = np.asarray(m) != 0
    nx, ny, nz = m.shape
    flat_m = m.reshape(-1, order="F")
    flat_l = np.zeros(flat_m.size, np.int32)
    p = nx * ny
    for i in np.flatnonzero(flat_m):
        if flat_l[i]:
            continue
        flat_l[i] = i + 1
        stack = [int(i)]
        while stack:
            c = stack.pop()
            x, y, z = c % nx, (c // nx) % ny, c // p
            for ok, nb in ((x > 0, c - 1), (x < nx - 1, c + 1), (y > 0, c - nx), (y < ny - 1, c + nx), (z > 0, c - p), (z < nz - 1, c + p)):
                if ok and flat_m[nb] and not flat_l[nb]:
                    flat_l[nb] = i + 1
                    stack.append(nb)
    return flat_l.reshape(m.shape, order="F")


def largest(lab):
    """the label of the component of most voxels, ties to the smaller label; 0 when there is none"""
    u, c = np.unique(lab[lab != 0], return_counts=True)
    return int(u[np.argmax(c)]) if u.size else 0             # (unique sorts ascending, argmax takes the first)


def holes(m):
    """the voxels fill_holes adds: components of the complement without a voxel on a face"""
    m = np.asarray(m) != 0
    lab = components(~m)
    face = np.zeros(m.shape, bool)
    face[0], face[-1], face[:, 0], face[:, -1], face[:, :, 0], face[:, :, -1] = True, True, True, True, True, True
    touching = np.unique(lab[face & (lab != 0)])
    return (lab != 0) & ~np.isin(lab, touching)


def dilate(m, passes):
    m = np.asarray(m) != 0
    for _ in range(passes):
        o = m.copy()
        o[1:] |= m[:-1]; o[:-1] |= m[1:]
        o[:, 1:] |= m[:, :-1]; o[:, :-1] |= m[:, 1:]
        o[:, :, 1:] |= m[:, :, :-1]; o[:, :, :-1] |= m[:, :, 1:]
        m = o
    return m


def select_fill(m, flags):
    """(result mask bool, info counters) of the component stage on a mask"""
    m = np.asarray(m) != 0
    lab = components(m)
    ncomp = int(np.unique(lab[lab != 0]).size)
    sel = (lab == largest(lab)) & m if flags & KEEP_LARGEST else m.copy()
    n_kept = int(sel.sum())
    n_filled = 0
    if flags & FILL_HOLES:
        h = holes(sel)
        n_filled = int(h.sum())
        sel = sel | h
    return sel, dict(n_above=int(m.sum()), n_components=ncomp, n_kept=n_kept, n_filled=n_filled)


def mask_components(m, flags=0):
    """(int32 canonical labels of the result's components, result mask uint8, info)"""
    sel, info = select_fill(m, flags)
    info = dict(status=0, kstar=0, lo=np.float32(0), hi=np.float32(0), threshold=0.0, **info, n_mask=int(sel.sum()))
    return components(sel), sel.astype(np.uint8), info


def mask_from_b0(b0, radius=2, numpass=4, flags=KEEP_LARGEST | FILL_HOLES, dilate_passes=0):
    """(mask uint8, info) of everything after the mean"""
    v = median(b0, radius, numpass) if numpass > 0 else np.asarray(b0, np.float32)
    r = finite_range(v)
    zero = dict(n_above=0, n_components=0, n_kept=0, n_filled=0, n_mask=0)
    if r is None:
        return np.zeros(v.shape, np.uint8), dict(status=1, kstar=-1, lo=np.float32(0), hi=np.float32(0), threshold=0.0, **zero)
    lo, hi = r
    if hi == lo:
        return np.zeros(v.shape, np.uint8), dict(status=1, kstar=-1, lo=lo, hi=hi, threshold=0.0, **zero)
    b = bins(v, lo, hi)
    k = otsu(np.bincount(b[b >= 0].reshape(-1), minlength=256))
    above = b > k
    sel, info = select_fill(above, flags)
    out = dilate(sel, dilate_passes)
    thr = np.float64(lo) + np.float64(k + 1) * (np.float64(hi) - np.float64(lo)) / 256.0
    return out.astype(np.uint8), dict(status=0, kstar=k, lo=lo, hi=hi, threshold=float(thr), **info, n_mask=int(out.sum()))


def dwi_mask(vol4, frames, radius=2, numpass=4, flags=KEEP_LARGEST | FILL_HOLES, dilate_passes=0):
    """(mask uint8, b0 float32, info)"""
    b0 = mean_frames(vol4, frames)
    m, info = mask_from_b0(b0, radius, numpass, flags, dilate_passes)
    return m, b0, info


def info_equal(got, want):
    """every field bit for bit: the integers equal, lo / hi by float32 bits, threshold by float64 bits"""
    bad = []
    for k, w in want.items():
        g = got[k]
        if k in ("lo", "hi"):
            same = np.float32(g).view(np.uint32) == np.float32(w).view(np.uint32)
        elif k == "threshold":
            same = np.float64(g).view(np.uint64) == np.float64(w).view(np.uint64)
        else:
            same = int(g) == int(w)
        if not same:
            bad.append((k, g, w))
    return bad


# ---- the known answer: a ball with a dark cavity and bright islands outside ------------------------------------------------------------
def ball_phantom(shape=(24, 24, 24), seed=0, nframes=3):
    """(dwi float32 [nx,ny,nz,nframes], the true ball bool): U(800, 1200) inside a ball of radius 8.5 / 24 of the smallest edge about the
    centre, |N(0, 20)| outside, a dark cavity of radius 2 inside, two bright 5^3 islands in corners outside (one where the volume is
    too small for two).  The frames are the ball times (1, 0.98, 1.02, ...) plus a little noise of their own."""
    rng = np.random.default_rng(seed)
    nx, ny, nz = shape
    c = (np.array(shape) - 1) / 2.0
    rad = 8.5 * min(shape) / 24.0
    x, y, z = np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij")
    r2 = (x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2
    ball = r2 <= rad * rad
    img = np.where(ball, rng.uniform(800, 1200, shape), np.abs(rng.normal(0, 20, shape)))
    cav = (x - (c[0] + rad / 3)) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2 <= 4.0
    img[cav & ball] = np.abs(rng.normal(0, 20, shape))[cav & ball]
    isl = np.zeros(shape, bool)
    isl[:5, :5, :5] = True
    if min(shape) >= 20:
        isl[-5:, -5:, :5] = True
    isl &= ~ball
    img[isl] = rng.uniform(800, 1200, shape)[isl]
    scale = 1.0 + 0.02 * np.array([((-1) ** f) * ((f + 1) // 2) for f in range(nframes)])
    dwi = img[..., None] * scale + rng.normal(0, 1, shape + (nframes,))
    return np.asfortranarray(dwi.astype(np.float32)), ball


def dice(a, b):
    a, b = np.asarray(a) != 0, np.asarray(b) != 0
    return 2.0 * (a & b).sum() / (a.sum() + b.sum())
