"""NumPy float64 restatement of dwi_degibbs (include/fibers_hip.h "Gibbs-ringing removal"), by two routes:
  A  the filter and the shifted rows with numpy.fft (phase ramp e^{+2 pi i k s / n} over signed k, the Nyquist bin zeroed for j >= 1);
  B  the filter as a direct DFT from a twiddle table, the shifted rows as products with the circulant of the cosine sum D(t).
TEST INFRASTRUCTURE, NumPy only: the kernels are held to route A with a tolerance made of the routes' own difference."""
import functools

import numpy as np

LIMIT = 256                           # FIB_DEGIBBS_MAX_SIZE


# ---- the pieces of the definition -----------------------------------------------------------------------------------------------------
def shifts(K):
    """s_j, j = 0 .. 2K: 0, then j / J, then -j / J"""
    J = 2 * K + 1
    return np.array([0.0] + [j / J for j in range(1, K + 1)] + [-j / J for j in range(1, K + 1)])


def weights(n):
    """c[p] = 1 + cos(2 pi p / n), exactly 0 where 2 p == n"""
    c = 1.0 + np.cos(2.0 * np.pi * np.arange(n) / n)
    if n % 2 == 0:
        c[n // 2] = 0.0
    return c


def gains(nu, nv):
    """Gu, Gv [nu, nv]; both 0 in the bin where 2p == nu and 2q == nv (the integer test)"""
    cu, cv = weights(nu)[:, None], weights(nv)[None, :]
    den = cu + cv
    corner = (2 * np.arange(nu)[:, None] == nu) & (2 * np.arange(nv)[None, :] == nv)
    den = np.where(corner, 1.0, den)
    return np.where(corner, 0.0, cv / den), np.where(corner, 0.0, cu / den)


def dft_matrix(n):
    """e^{-2 pi i p u / n} with the product reduced mod n: the twiddle table a direct DFT reads"""
    k = np.outer(np.arange(n), np.arange(n)) % n
    return np.exp(-2j * np.pi * k / n)


def filter_a(a):
    Gu, Gv = gains(*a.shape)
    A = np.fft.fft2(a)
    return np.fft.ifft2(A * Gu).real, np.fft.ifft2(A * Gv).real


def filter_b(a):
    nu, nv = a.shape
    Gu, Gv = gains(nu, nv)
    Fu, Fv = dft_matrix(nu), dft_matrix(nv)
    A = Fu @ a @ Fv.T
    inv = lambda X: (Fu.conj() @ X @ Fv.conj().T).real / (nu * nv)     # noqa: E731
    return inv(A * Gu), inv(A * Gv)


def table_b(n, K):
    """route B's D as the library lays its table out: [2K, n], [j - 1, t] = D(t + s_j), D(t) = (1 / n) (1 + 2 sum_{k=1..h} cos(2 pi k t /
    n)), h = floor((n - 1) / 2), summed in ascending k.  t + s_j = a / J with an integer a, and k a is reduced mod n J in integers, so
    every cosine is taken of an angle in [0, 2 pi) that carries one rounding: plain float64 angles of up to 2 pi h n lose the 2^-50"""
    J = 2 * K + 1
    i = np.array([j for j in range(1, K + 1)] + [-j for j in range(1, K + 1)], np.int64)     # s_j in units of 1 / J
    a = (np.arange(n, dtype=np.int64)[None, :] * J + i[:, None]) % (n * J)
    acc = np.zeros(a.shape)
    for k in range(1, (n - 1) // 2 + 1):
        acc = acc + np.cos(2.0 * np.pi * ((a * k) % (n * J)) / (n * J))
    return (1.0 + 2.0 * acc) / n


def candidates_a(r, K):
    """r [R, n] -> r_j [2K + 1, R, n] with numpy.fft"""
    n = r.shape[1]
    k = np.fft.fftfreq(n) * n                                        # signed bins
    F = np.fft.fft(r, axis=1)
    out = [r]
    for s in shifts(K)[1:]:
        ph = np.exp(2j * np.pi * k * s / n)
        if n % 2 == 0:
            ph[n // 2] = 0.0
        out.append(np.fft.ifft(F * ph[None, :], axis=1).real)
    return np.stack(out)


def candidates_b(r, K):
    """the same as circulant products with D(l - m + s_j)"""
    n = r.shape[1]
    lm = (np.arange(n)[:, None] - np.arange(n)[None, :]) % n         # (l - m) mod n: D has period n
    return np.stack([r] + [r @ Dj[lm].T for Dj in table_b(n, K)])


def unring(r, K, minW, maxW, candidates):
    """rows r [R, n] -> (output [R, n], j* [R, n], t [2K + 1, R, n])"""
    c = candidates(r, K)
    d = np.abs(np.roll(c, -1, axis=2) - c)                           # d_j[l] = |r_j[l+1] - r_j[l]|
    L, Rr = np.zeros_like(d), np.zeros_like(d)
    for w in range(minW, maxW + 1):                                  # sequential in ascending w
        L = L + np.roll(d, w + 1, axis=2)                            # d_j[l - w - 1]
        Rr = Rr + np.roll(d, -w, axis=2)                             # d_j[l + w]
    t = np.minimum(L, Rr)
    js = np.argmin(t, axis=0)                                        # the first j that attains the minimum
    pick = lambda x: np.take_along_axis(x, js[None], axis=0)[0]      # noqa: E731
    s = shifts(K)[js]
    cur, prev, nxt = pick(c), pick(np.roll(c, 1, axis=2)), pick(np.roll(c, -1, axis=2))
    out = np.where(s > 0, cur * (1 - s) + prev * s, cur * (1 + s) - nxt * s)
    return out, js, t


def degibbs_slice(a, K, minW, maxW, route):
    """one slice a[u][v] (float64) -> dict(out, ju, jv, tu, tv, au, av)"""
    au, av = (filter_a if route == "A" else filter_b)(a)
    cand = candidates_a if route == "A" else candidates_b
    ou, ju, tu = unring(au.T, K, minW, maxW, cand)                   # rows along u: one per v
    ov, jv, tv = unring(av, K, minW, maxW, cand)                     # rows along v: one per u
    return dict(out=ou.T + ov, ju=ju.T, jv=jv, tu=np.transpose(tu, (0, 2, 1)), tv=tv, au=au, av=av)


def _gap(t):
    s = np.sort(t, axis=0)
    return s[1] - s[0]


def degibbs(vol, slice_axis=2, K=20, minW=1, maxW=3):
    """vol [nx, ny, nz, N] (float32 samples) -> dict: out float64, ju, jv int (all of vol's shape), d = the largest difference of the two
    routes' outputs, e_t = the largest difference of their t_j[l], gap_u / gap_v = the second smallest minus the smallest t_j[l] of
    route A per pixel, same_pick = the routes chose the same j* everywhere"""
    vol = np.asarray(vol, np.float64)
    if min(vol.shape[a] for a in range(3) if a != slice_axis) < 2 * maxW + 3:
        raise ValueError("in-plane sizes below 2 maxW + 3")
    res = dict(out=np.zeros(vol.shape), ju=np.zeros(vol.shape, np.int64), jv=np.zeros(vol.shape, np.int64), gap_u=np.zeros(vol.shape),
               gap_v=np.zeros(vol.shape), d=0.0, e_t=0.0, same_pick=True)
    for f in range(vol.shape[3]):
        for s in range(vol.shape[slice_axis]):
            ix = [slice(None)] * 3 + [f]
            ix[slice_axis] = s
            ix = tuple(ix)
            A, B = degibbs_slice(vol[ix], K, minW, maxW, "A"), degibbs_slice(vol[ix], K, minW, maxW, "B")
            res["out"][ix], res["ju"][ix], res["jv"][ix] = A["out"], A["ju"], A["jv"]
            res["gap_u"][ix], res["gap_v"][ix] = _gap(A["tu"]), _gap(A["tv"])
            res["d"] = max(res["d"], np.abs(A["out"] - B["out"]).max())
            res["e_t"] = max(res["e_t"], np.abs(A["tu"] - B["tu"]).max(), np.abs(A["tv"] - B["tv"]).max())
            res["same_pick"] &= bool(np.array_equal(A["ju"], B["ju"]) and np.array_equal(A["jv"], B["jv"]))
    return res


def total_variation(vol, slice_axis):
    """the anisotropic total variation of every slice, circular, summed"""
    ua, va = [a for a in range(3) if a != slice_axis]
    v = np.asarray(vol, np.float64)
    return np.abs(np.roll(v, -1, axis=ua) - v).sum() + np.abs(np.roll(v, -1, axis=va) - v).sum()


# ---- the phantom and the cases --------------------------------------------------------------------------------------------------------
def phantom_slice(nu, nv, rng):
    """box in box (300 around 1000) drawn at 4x the resolution, its centred k-space cut to nu x nv (real ringing), plus noise of sigma 5
    in every pixel (no two candidates tie)"""
    hu, hv = 4 * nu, 4 * nv
    hi = np.zeros((hu, hv))
    jit = lambda n: int(rng.integers(-n // 16 - 1, n // 16 + 2))     # noqa: E731
    u0, u1, v0, v1 = hu // 6 + jit(hu), hu - hu // 6 + jit(hu), hv // 6 + jit(hv), hv - hv // 6 + jit(hv)
    hi[u0:u1, v0:v1] = 300.0
    hi[hu // 3 + jit(hu):hu - hu // 3 + jit(hu), hv // 3 + jit(hv):hv - hv // 3 + jit(hv)] = 1000.0
    F = np.fft.fftshift(np.fft.fft2(hi))
    cu, cv = hu // 2 - nu // 2, hv // 2 - nv // 2
    lo = np.fft.ifft2(np.fft.ifftshift(F[cu:cu + nu, cv:cv + nv])).real * (nu * nv) / (hu * hv)
    return lo + rng.normal(0.0, 5.0, (nu, nv))


def phantom(shape, N, slice_axis, seed):
    vol = np.zeros(tuple(shape) + (N,), np.float32)
    rng = np.random.default_rng(seed)
    nu, nv = [shape[a] for a in range(3) if a != slice_axis]
    for f in range(N):
        for s in range(shape[slice_axis]):
            ix = [slice(None)] * 3 + [f]
            ix[slice_axis] = s
            vol[tuple(ix)] = phantom_slice(nu, nv, rng)
    return np.asfortranarray(vol)


# (shape, N, slice_axis, K, minW, maxW, seed)
CASES = [
    ((9, 9, 2), 1, 2, 20, 1, 3, 1),            # the minimum at maxW = 3
    ((12, 9, 3), 2, 2, 20, 1, 3, 2),           # even and odd
    ((16, 16, 2), 2, 2, 20, 1, 3, 3),          # both even: the zeroed corner bin
    ((15, 14, 2), 3, 2, 20, 1, 3, 4),
    ((64, 9, 1), 1, 2, 20, 1, 3, 5),           # a row of exactly one wave
    ((65, 10, 1), 1, 2, 20, 1, 3, 6),          # and one past it
    ((5, 9, 12), 2, 0, 20, 1, 3, 7),           # 9 x 12 in plane, 5 slices across x (as 9 x 12 x 5 the planes would be 12 x 5: refused)
    ((9, 5, 12), 2, 1, 20, 1, 3, 8),           # 9 x 12 in plane, 5 slices across y
    ((LIMIT, 9, 1), 1, 2, 20, 1, 3, 9),        # the in-plane limit in one axis
    ((15, 14, 2), 3, 2, 1, 1, 3, 10),          # nshifts 1
    ((15, 14, 2), 3, 2, 32, 1, 3, 11),         # nshifts 32
    ((15, 14, 2), 3, 2, 20, 1, 1, 12),         # windows (1, 1)
    ((15, 15, 2), 3, 2, 20, 2, 6, 13),         # windows (2, 6): 15 x 14 is below 2 maxW + 3 = 15 and refused (test_degibbs_ref.py)
]
# the minimum at maxW = 1: the 22 samples a thread reads around its own wrap round the row more than once.  A kernel path, not a
# phantom: on 5 x 6 pixels the method has nothing to remove, so the total-variation property is not asked of it
EDGE = [((5, 6, 1), 1, 2, 20, 1, 1, 14)]
PHANTOMS, CASES = list(CASES), CASES + EDGE


def case_id(case):
    shape, N, axis, K, minW, maxW, _ = case
    return "%dx%dx%dx%d-a%d-K%d-w%d%d" % (shape + (N, axis, K, minW, maxW))


@functools.lru_cache(maxsize=None)
def case_volume(case):
    shape, N, axis, *_ = case
    v = phantom(shape, N, axis, case[6])
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def case_reference(case):
    """degibbs() of the case's volume, computed once and shared (read-only)"""
    _, _, axis, K, minW, maxW, _ = case
    r = degibbs(case_volume(case), axis, K, minW, maxW)
    for v in r.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return r
