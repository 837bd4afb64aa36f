"""Bundle tools on the GPU (csrc/bundle.hip through the C ABI: fibd_str_* on device tensors, fib_str_* on host arrays, and the Python
layer on top) against the NumPy restatement of the header's definitions (tests/bundle_ref.py, pinned by tests/test_bundle_ref.py).

RESAMPLE: rows 0 and K-1, every row of lines with n <= 1 and the NaN rows are compared BIT FOR BIT.  The order of the additions behind
the cumulative lengths is free on the device, so every other component is held to the bound derived from that freedom:
|gpu - ref| <= ulp32(|ref|) + n * 2^-50 * T / min(r) + 2^-50 * max|p|  (each any-order float64 prefix sum is within (n-1) * 2^-53 * T
of the exact one; a position moves by at most four times the difference of two such sums in mm, a polyline being 1-Lipschitz in its
own arc length, and a voxel is at least min(r) mm; the last two terms are the interpolation's and the final rounding's).
ASSIGN: label, dist, flip and dist_all are BIT-IDENTICAL to the restatement (sequential float64 sums, the file is compiled with
contraction off).  CENTROIDS: counts bit-identical, |sums_gpu - sums_ref| <= (N_b - 1) * 2^-52 * sum|t| per cell."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bundle_ref as bd  # noqa: E402

pytestmark = pytest.mark.gpu
FIB_ERR_INVALID, FIB_ERR_UNSUPPORTED = -1, -7
LENGTHS = (0, 1, 2, 15, 16, 17, 63, 64, 65, 255, 256, 257, 300)
SENTINEL = 0x5A5A5A5A
RES = (1.25, 0.5, 2.0)
SHAPE = (9, 8, 7)
KS = (2, 3, 12, 20, 64, 65, 256)


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def _np(t):
    return t.cpu().numpy()


def _to_dev(dev, xyz, npts):
    import torch
    return torch.from_numpy(np.ascontiguousarray(xyz, np.float32)).to(dev), torch.from_numpy(np.ascontiguousarray(npts, np.int32)).to(dev)


def _t(dev, a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).to(dev)                    # (a copy: the shared references are read-only)


def _walks(rng, lengths, shape, step=0.35, wild=0.01, margin=0.1):
    """random walks folded back into a box a little larger than the volume; every line longer than 4 repeats some of its points (the
    tracer emits the seed twice); a few points replaced by NaN / Inf / 1e30"""
    out = []
    lo = 0.5 - margin
    w = np.array(shape, np.float64) + 2 * margin
    for n in lengths:
        if n == 0:
            continue
        d = rng.standard_normal((n, 3))
        d = np.cumsum(0.7 * d / np.linalg.norm(d, axis=1, keepdims=True) * step + 0.3 * step * rng.standard_normal(3), axis=0)
        p = rng.uniform(lo, lo + w, 3) + d
        p = lo + w - np.abs(np.mod(p - lo, 2 * w) - w)
        if n > 4:
            at = rng.integers(1, n, max(1, n // 40))
            p[at] = p[at - 1]
            p[1] = p[0]
            if n % 2:
                p[n - 1] = p[n - 2]
        out.append(p)
    xyz = (np.concatenate(out) if out else np.zeros((0, 3))).astype(np.float32)
    bad = rng.random(xyz.shape[0]) < wild
    xyz[bad, rng.integers(0, 3, int(bad.sum()))] = rng.choice(np.array([np.nan, np.inf, -np.inf, 1e30, -1e30], np.float32), int(bad.sum()))
    return xyz


class Case:
    """257 random walks (a partial last group and workgroup), lengths from LENGTHS, one line of 100 000 points, about 1 % wild points;
    `clean`: the same lines with every wild point put at (3, 3, 3); the restatement's answers, computed once per K"""

    def __init__(self, seed=51):
        rng = np.random.default_rng(seed)
        n = np.concatenate([np.array(LENGTHS), rng.choice(np.array(LENGTHS), 257 - len(LENGTHS))]).astype(np.int32)
        rng.shuffle(n)
        n[100] = 100000
        self.npts = n
        self.xyz = _walks(rng, n, SHAPE)
        with np.errstate(invalid="ignore"):
            self.clean = np.where(np.abs(self.xyz) < 1e29, self.xyz, np.float32(3.0)).astype(np.float32)
        self.off = np.concatenate([[0], np.cumsum(n.astype(np.int64))])
        self.bound = {"wild": bd.resample_bound(self.xyz, n, RES), "clean": bd.resample_bound(self.clean, n, RES)}
        self._ref = {}

    def points(self, which):
        return self.xyz if which == "wild" else self.clean

    def ref(self, which, K):
        if (which, K) not in self._ref:
            r = bd.resample(self.points(which), self.npts, RES, K)
            r.setflags(write=False)
            self._ref[(which, K)] = r
        return self._ref[(which, K)]


@pytest.fixture(scope="module")
def case():
    return Case()


def _check_resample(c, which, K, got, flip=None, what=""):
    """the header's rules for one result [nlines, K, 3] against the restatement"""
    ref = c.ref(which, K)
    if flip is not None:
        ref = np.where(np.asarray(flip, bool)[:, None, None], ref[:, ::-1], ref)
    assert got.dtype == np.float32 and got.shape == ref.shape
    gu, ru = got.view(np.uint32), ref.view(np.uint32)
    nanline = np.isnan(ref).all(axis=(1, 2))
    exact = nanline | (c.npts <= 1)
    assert np.array_equal(gu[exact], ru[exact]), (what, K)                  # NaN rows (0x7FC00000) and copies, bit for bit
    assert np.array_equal(gu[:, [0, K - 1]], ru[:, [0, K - 1]]), (what, K)   # the two ends
    rest = ~exact
    assert rest.sum() > 100 and nanline.sum() > (10 if which == "wild" else 0) and not np.isnan(ref[rest]).any()
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    with np.errstate(invalid="ignore", over="ignore"):
        err = np.abs(got[rest].astype(np.float64) - ref[rest].astype(np.float64))
        tol = bd.ulp32(ref[rest]) + c.bound[which][rest][:, None, None]
    print("resample %s K=%d %s: %d of %d components differ from the restatement, largest error / tolerance %.3g"
          % (which, K, what, int((gu[rest] != ru[rest]).sum()), gu[rest].size, float((err / tol).max())))
    assert (err <= tol).all(), (what, K, np.argwhere(err > tol)[:5])


# ---- resample ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", KS)
def test_resample_on_random_walks(fj, dev, case, K):
    import torch
    c = case
    for which in ("wild", "clean"):
        x, n = _to_dev(dev, c.points(which), c.npts)
        out, status = fj.str_resample_device(x, n, RES, K)
        got = _np(out)
        assert int(status.item()) == c.npts.size
        _check_resample(c, which, K, got)
        ones = torch.ones(c.npts.size, dtype=torch.uint8, device=dev)
        flipped = _np(fj.str_resample_device(x, n, RES, K, flip=ones)[0])
        assert np.array_equal(flipped.view(np.uint32), got[:, ::-1].view(np.uint32))          # all-ones flip: the rows reversed, bit for bit
        again = _np(fj.str_resample_device(x, n, RES, K)[0])
        assert np.array_equal(again.view(np.uint32), got.view(np.uint32))                      # two runs: the same bytes
    # mixed flags, and the bool spelling
    fl = (np.arange(c.npts.size) % 3 == 0)
    mixed = _np(fj.str_resample_device(x, n, RES, K, flip=_t(dev, fl))[0])
    _check_resample(c, "clean", K, mixed, flip=fl, what="mixed flip")
    assert np.array_equal(mixed.view(np.uint32), np.where(fl[:, None, None], got[:, ::-1], got).view(np.uint32))


def test_resample_does_not_depend_on_the_order_of_the_lines(fj, dev, case):
    c = case
    K = 20
    x, n = _to_dev(dev, c.xyz, c.npts)
    base = _np(fj.str_resample_device(x, n, RES, K)[0])
    perm = np.random.default_rng(5).permutation(c.npts.size)
    xyz = np.concatenate([c.xyz[c.off[l]:c.off[l + 1]] for l in perm])
    x2, n2 = _to_dev(dev, xyz, c.npts[perm])
    got = _np(fj.str_resample_device(x2, n2, RES, K)[0])
    assert np.array_equal(got.view(np.uint32), base[perm].view(np.uint32))
    # a line alone, and on a 4-byte aligned view on a side stream
    import torch
    l = 100
    one = _np(fj.str_resample_device(*_to_dev(dev, c.xyz[c.off[l]:c.off[l + 1]], c.npts[l:l + 1]), RES, K)[0])
    assert np.array_equal(one[0].view(np.uint32), base[l].view(np.uint32))
    buf = torch.zeros(c.xyz.size + 8, dtype=torch.float32, device=dev)
    view = buf[1:1 + c.xyz.size].view(-1, 3)
    view.copy_(x)
    assert view.data_ptr() % 16 == 4
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        got = fj.str_resample_device(view, n, RES, K, stream=side)[0]
    side.synchronize()
    assert np.array_equal(_np(got).view(np.uint32), base.view(np.uint32))


def test_resample_refusals_and_host_form(fj, dev, case):
    import torch
    c = case
    L = fj.lib()
    nl, npnt = c.npts.size, c.xyz.shape[0]
    x, n = _to_dev(dev, c.xyz, c.npts)
    res = (C.c_float * 3)(*RES)
    work = torch.empty(fj.str_work_size(nl) // 8 + 1, dtype=torch.int64, device=dev)
    out = torch.full((nl, 20, 3), SENTINEL, dtype=torch.int32, device=dev)
    status = torch.full((1,), 99, dtype=torch.int64, device=dev)
    args = (x.data_ptr(), n.data_ptr(), nl, npnt, res)
    tail = (None, out.data_ptr(), status.data_ptr(), work.data_ptr(), work.numel() * 8, None)
    for K in (1, 257, 0, -3):
        assert L.fibd_str_resample(*args, K, *tail) == FIB_ERR_UNSUPPORTED
        assert L.fib_str_resample(0, c.xyz.ctypes.data, c.npts.ctypes.data, nl, npnt, res, K, None, None) == FIB_ERR_UNSUPPORTED
    assert L.fibd_str_resample(*args, 20, None, out.data_ptr(), status.data_ptr(), work.data_ptr(), 64, None) == FIB_ERR_INVALID    # work too small
    short = c.npts.copy(); short[200] = max(0, short[200] - 1); short[3] += 2                          # sum != npoints
    neg = c.npts.copy(); neg[256] = -3; neg[0] += 3 + c.npts[256]                                       # a negative count, the sum still right
    assert short.sum() != c.npts.sum() and neg.sum() == c.npts.sum()
    for bad in (short, neg):
        nb = torch.from_numpy(bad).to(dev)
        assert L.fibd_str_resample(x.data_ptr(), nb.data_ptr(), nl, npnt, res, 20, *tail) == 0
        torch.cuda.synchronize()
        assert int(status.item()) == -1 and (_np(out) == SENTINEL).all()                                # nothing is written
        status.fill_(99)
        hout = np.full((nl, 20, 3), SENTINEL, np.uint32)
        assert L.fib_str_resample(0, c.xyz.ctypes.data, bad.ctypes.data, nl, npnt, res, 20, None, hout.ctypes.data) == FIB_ERR_INVALID
        assert (hout == SENTINEL).all()
    assert L.fibd_str_resample(*args, 20, *tail) == 0
    torch.cuda.synchronize()
    assert int(status.item()) == nl
    # no lines at all
    assert L.fibd_str_resample(x.data_ptr(), n.data_ptr(), 0, 0, res, 20, *tail) == 0
    torch.cuda.synchronize()
    assert int(status.item()) == 0
    # the host form equals the device form, with and without flags
    fl = (np.arange(nl) % 2).astype(np.uint8)
    for K, flags in ((20, None), (65, fl)):
        want = _np(fj.str_resample_device(x, n, RES, K, flip=None if flags is None else _t(dev, flags))[0])
        hout = np.empty((nl, K, 3), np.float32)
        assert L.fib_str_resample(0, c.xyz.ctypes.data, c.npts.ctypes.data, nl, npnt, res, K, None if flags is None else flags.ctypes.data,
                                  hout.ctypes.data) == 0
        assert np.array_equal(hout.view(np.uint32), want.view(np.uint32))
    assert L.fib_str_resample(-1, c.xyz.ctypes.data, c.npts.ctypes.data, nl, npnt, res, 20, None, hout.ctypes.data) == FIB_ERR_UNSUPPORTED
    fj.trim()


# ---- assign ------------------------------------------------------------------------------------------------------------------------
def _models(rng, lines, nclean, nmodels):
    """models from three sources -- the lines themselves (wild ones, all NaN, among them from the fourth model on), reversed copies,
    noise -- and the last a duplicate of the first"""
    K = lines.shape[1]
    real = np.flatnonzero(~np.isnan(lines[:nclean]).any(axis=(1, 2)))
    m = np.empty((nmodels, K, 3), np.float32)
    for i in range(nmodels):
        src = lines[rng.choice(real)] if i < 3 or rng.random() < 0.9 else lines[rng.integers(nclean, lines.shape[0])]
        if i % 3 == 0:
            m[i] = src
        elif i % 3 == 1:
            m[i] = src[::-1]
        else:
            m[i] = src + rng.standard_normal((K, 3)).astype(np.float32)
    if nmodels >= 2:
        m[nmodels - 1] = m[0]
    return m


@pytest.mark.parametrize("K,nmodels", [(2, 1), (12, 2), (20, 63), (20, 64), (20, 65), (100, 700)])
def test_assign_is_bit_identical_to_the_restatement(fj, dev, case, K, nmodels):
    c = case
    rng = np.random.default_rng(K * 1000 + nmodels)
    lines = np.concatenate([c.ref("clean", K), c.ref("wild", K)])            # 514 lines: two full workgroups and two lines
    nclean = c.npts.size
    models = _models(rng, lines, nclean, nmodels)
    pairs = bd.mdf(lines, models, RES)
    a, m = _t(dev, lines), _t(dev, models)
    rl, rd, rf, rall = bd.assign(lines, models, RES, np.inf, pairs)
    assert np.isnan(rd).sum() > 10 and (rd == 0).sum() >= 1 and (nmodels <= 2 or rf.any())
    if nmodels >= 2:
        assert (rl == nmodels - 1).sum() == 0 and (rl == 0).sum() >= 1       # the duplicate of model 0 never wins
    own = float(rd[np.flatnonzero(rd > 0)[0]])                                # a threshold equal to a line's own distance (as float32: the
                                                                              # float64 d may lie on either side of it; thresh 0 is the exact tie)
    for thresh in (np.inf, 0.0, own):
        rl, rd, rf, rall = bd.assign(lines, models, RES, thresh, pairs)
        got = fj.str_assign_device(a, m, RES, thresh, dist_all=True)
        assert np.array_equal(_np(got["label"]), rl), (thresh, np.flatnonzero(_np(got["label"]) != rl)[:5])
        assert np.array_equal(_np(got["dist"]).view(np.uint32), rd.view(np.uint32))
        assert np.array_equal(_np(got["flip"]), rf) and _np(got["flip"]).dtype == np.uint8
        assert np.array_equal(_np(got["dist_all"]).view(np.uint32), rall.view(np.uint32))
        if thresh == own:
            assert (rl == -1).any() and (rl >= 0).any()
        if thresh == 0.0:
            assert ((rl >= 0) == (rd == 0)).all()
    none = fj.str_assign_device(a, m, RES, 1.0)                               # without dist_all
    assert none["dist_all"] is None and np.array_equal(_np(none["dist"]).view(np.uint32), rd.view(np.uint32))
    # the host form equals the device form
    L = fj.lib()
    nl = lines.shape[0]
    hl, hd, hf, hall = np.empty(nl, np.int32), np.empty(nl, np.float32), np.empty(nl, np.uint8), np.empty((nl, nmodels), np.float32)
    assert L.fib_str_assign(0, lines.ctypes.data, nl, K, models.ctypes.data, nmodels, (C.c_float * 3)(*RES), own, hl.ctypes.data, hd.ctypes.data,
                            hf.ctypes.data, hall.ctypes.data) == 0
    assert np.array_equal(hl, rl) and np.array_equal(hd.view(np.uint32), rd.view(np.uint32)) and np.array_equal(hf, rf)
    assert np.array_equal(hall.view(np.uint32), rall.view(np.uint32))


def test_assign_refusals(fj, dev, case):
    L = fj.lib()
    lines = _t(dev, case.ref("clean", 12))
    nl = lines.shape[0]
    res = (C.c_float * 3)(*RES)
    import torch
    lab, dist, fl = torch.zeros(nl, dtype=torch.int32, device=dev), torch.zeros(nl, dtype=torch.float32, device=dev), torch.zeros(nl, dtype=torch.uint8, device=dev)
    outs = (lab.data_ptr(), dist.data_ptr(), fl.data_ptr(), None, None)
    assert L.fibd_str_assign(lines.data_ptr(), nl, 12, lines.data_ptr(), 0, res, 1.0, *outs) == FIB_ERR_INVALID
    assert L.fibd_str_assign(lines.data_ptr(), nl, 12, lines.data_ptr(), 1 << 24, res, 1.0, *outs) == FIB_ERR_INVALID
    assert L.fibd_str_assign(lines.data_ptr(), nl, 257, lines.data_ptr(), 1, res, 1.0, *outs) == FIB_ERR_UNSUPPORTED
    assert L.fibd_str_assign(lines.data_ptr(), nl, 12, None, 1, res, 1.0, *outs) == FIB_ERR_INVALID
    assert L.fibd_str_centroids(lines.data_ptr(), nl, 12, lab.data_ptr(), None, 1, 1, dist.data_ptr(), lab.data_ptr(), None) == FIB_ERR_INVALID   # flags
    torch.cuda.synchronize()


# ---- centroids ---------------------------------------------------------------------------------------------------------------------
def _sums_close(got, ref, bound):
    return np.abs(got - ref) <= bound


@pytest.mark.parametrize("K,nmodels", [(20, 3), (20, 250), (20, 2000), (100, 32), (2, 1), (64, 97)])
def test_centroids_on_random_labels(fj, dev, case, K, nmodels):
    """K = 20: one LDS window holds 102 bundles, so 3 bundles are one window, 250 three, and 2 000 go to the kernel without LDS;
    K = 100 holds 20 bundles per window; 2 580 lines are three workgroups"""
    import torch
    c = case
    rng = np.random.default_rng(K + nmodels)
    lines = np.tile(np.nan_to_num(c.ref("clean", K)), (10, 1, 1))            # (the rows of the lines without points are NaN: 0 here)
    nl = lines.shape[0]
    lines = lines + rng.standard_normal((nl, 1, 3)).astype(np.float32)
    label = rng.integers(-2, nmodels + 3, nl).astype(np.int32)               # -2, -1, nmodels, nmodels + 1, nmodels + 2: no bundle
    label[:5] = [-1, nmodels, nmodels + 1, 2 ** 31 - 1, -2 ** 31]
    if nmodels > 2:
        label[label == 1] = 0                                                 # bundle 1 holds no line
    flip = rng.integers(0, 2, nl).astype(np.uint8)
    a, lb, fl = _t(dev, lines), _t(dev, label), _t(dev, flip)
    S, N, bound = bd.centroids(lines, label, flip, nmodels)
    sums, counts = fj.str_centroids_device(a, lb, fl, nmodels)
    gs, gn = _np(sums), _np(counts)
    assert gn.dtype == np.uint32 and np.array_equal(gn, N) and gs.dtype == np.float64 and gs.shape == (nmodels, K, 3)
    ok = _sums_close(gs, S, bound)
    assert ok.all(), (np.argwhere(~ok)[:5], gs[~ok][:5], S[~ok][:5])
    assert not gs[N == 0].any() and (nmodels <= 2 or N[1] == 0)              # empty bundles are exactly 0
    # two halves with ACCUMULATE: the same counts, sums within the same bound
    h = nl // 2 + 7
    acc = fj.str_centroids_device(a[:h].contiguous(), lb[:h].contiguous(), fl[:h].contiguous(), nmodels)
    acc = fj.str_centroids_device(a[h:].contiguous(), lb[h:].contiguous(), fl[h:].contiguous(), nmodels, out=acc)
    assert np.array_equal(_np(acc[1]), N) and _sums_close(_np(acc[0]), S, bound).all()
    # flip = NULL is all zeros; one bundle holds every line
    every = np.full(nl, nmodels - 1, np.int32)
    S1, N1, b1 = bd.centroids(lines, every, None, nmodels)
    s1, n1 = fj.str_centroids_device(a, _t(dev, every), None, nmodels)
    assert np.array_equal(_np(n1), N1) and N1[nmodels - 1] == nl and _sums_close(_np(s1), S1, b1).all() and not _np(s1)[:nmodels - 1].any()
    # the host form: counts equal, sums within the bound
    hs, hn = np.full((nmodels, K, 3), 7.0), np.full(nmodels, 7, np.uint32)
    L = fj.lib()
    assert L.fib_str_centroids(0, lines.ctypes.data, nl, K, label.ctypes.data, flip.ctypes.data, nmodels, 0, hs.ctypes.data, hn.ctypes.data) == 0
    assert np.array_equal(hn, N) and _sums_close(hs, S, bound).all()
    assert L.fib_str_centroids(0, lines.ctypes.data, nl, K, label.ctypes.data, flip.ctypes.data, nmodels, 0x100, hs.ctypes.data, hn.ctypes.data) == 0
    # (2 N_b terms of sum 2 sum|t|: (2 N_b - 1) * 2^-52 * 2 sum|t| <= 6 * bound for N_b >= 2, and S + S is exact for N_b = 1)
    assert np.array_equal(hn, 2 * N) and _sums_close(hs, 2 * S, 6 * bound).all()


def test_host_forms_over_several_chunks_equal_the_device_forms(fj, dev):
    """more points than one chunk of the host forms holds (2^22, cut at line boundaries; 2^22 / K lines for the equal-length forms; the
    limit is a constant: the cuts themselves are checked at small limits on the CPU, tests/host_tier_check.cpp): resample and assign byte for byte, centroid counts exactly and sums within the bound"""
    import torch
    rng = np.random.default_rng(43)
    L = fj.lib()
    res = (C.c_float * 3)(*RES)
    npts = np.concatenate([[0, 1], rng.integers(0, 4000, 2300), [0]]).astype(np.int32)
    npnt = int(npts.sum())
    assert npnt > (1 << 22)
    xyz = np.cumsum(rng.standard_normal((npnt, 3)).astype(np.float32) * np.float32(0.3), axis=0, dtype=np.float32)
    flip = rng.integers(0, 2, npts.size).astype(np.uint8)
    K = 12
    want = _np(fj.str_resample_device(*_to_dev(dev, xyz, npts), RES, K, flip=_t(dev, flip))[0])
    got = np.empty((npts.size, K, 3), np.float32)
    assert L.fib_str_resample(0, xyz.ctypes.data, npts.ctypes.data, npts.size, npnt, res, K, flip.ctypes.data, got.ctypes.data) == 0
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)) and np.isnan(got[0]).all() and np.isfinite(got[1:-1]).all()
    K, nl, nm = 20, (1 << 22) // 20 + 5000, 3
    lines = rng.uniform(1, 9, (nl, K, 3)).astype(np.float32)
    models = lines[[7, nl // 2, nl - 1]][:, ::-1].copy()
    a, m = _t(dev, lines), _t(dev, models)
    r = fj.str_assign_device(a, m, RES, 4.0, dist_all=True)
    hl, hd, hf, hall = np.empty(nl, np.int32), np.empty(nl, np.float32), np.empty(nl, np.uint8), np.empty((nl, nm), np.float32)
    assert L.fib_str_assign(0, lines.ctypes.data, nl, K, models.ctypes.data, nm, res, 4.0, hl.ctypes.data, hd.ctypes.data, hf.ctypes.data, hall.ctypes.data) == 0
    assert np.array_equal(hl, _np(r["label"])) and np.array_equal(hd.view(np.uint32), _np(r["dist"]).view(np.uint32)) and np.array_equal(hf, _np(r["flip"]))
    assert np.array_equal(hall.view(np.uint32), _np(r["dist_all"]).view(np.uint32))
    assert hl[nl - 1] == 2 and hf[nl - 1] == 1 and hd[nl - 1] == 0 and (hl == -1).any() and (hl >= 0).sum() > 3
    sums, counts = fj.str_centroids_device(a, r["label"], r["flip"], nm)
    hs, hn = np.empty((nm, K, 3)), np.empty(nm, np.uint32)
    assert L.fib_str_centroids(0, lines.ctypes.data, nl, K, hl.ctypes.data, hf.ctypes.data, nm, 0, hs.ctypes.data, hn.ctypes.data) == 0
    assert np.array_equal(hn, _np(counts)) and int(hn.sum()) == int((hl >= 0).sum())
    # both are any-order sums of the same N_b terms, each within (N_b - 1) * 2^-52 * sum|t| of the sequential one; sum|t| <= 9 N_b here
    nb = hn.astype(np.float64)[:, None, None]
    assert (np.abs(hs - _np(sums)) <= 2 * np.maximum(nb - 1, 0) * 2.0 ** -52 * 9 * nb).all()
    fj.trim()


def test_resample_host_form_cut_by_lines_equals_the_device_form(fj, dev):
    """K = 256: a chunk of the host form holds 2^22 / 256 = 16 384 lines whatever their points, so 16 384 + 37 lines of 0 to 3 points are
    cut by the line limit and not by the point limit (about 25 000 points in all); byte for byte against the device form"""
    rng = np.random.default_rng(47)
    K, nl = 256, (1 << 22) // 256 + 37
    npts = rng.integers(0, 4, nl).astype(np.int32)
    npnt = int(npts.sum())
    assert nl == 16384 + 37 and npnt < (1 << 22) and all((npts == n).any() for n in range(4))
    xyz = (rng.uniform(1, 8, (npnt, 3)) + np.cumsum(rng.standard_normal((npnt, 3)) * 0.3, axis=0) % 1.0).astype(np.float32)
    flip = rng.integers(0, 2, nl).astype(np.uint8)
    want = _np(fj.str_resample_device(*_to_dev(dev, xyz, npts), RES, K, flip=_t(dev, flip))[0])
    got = np.full((nl, K, 3), SENTINEL, np.uint32).view(np.float32)
    assert fj.lib().fib_str_resample(0, xyz.ctypes.data, npts.ctypes.data, nl, npnt, (C.c_float * 3)(*RES), K, flip.ctypes.data, got.ctypes.data) == 0
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.isnan(got[npts == 0]).all() and np.isfinite(got[npts > 0]).all()     # (every line was written, the last 37 included)
    fj.trim()


# ---- Python tier -------------------------------------------------------------------------------------------------------------------
def _two_bundles(rng, nper=40):
    """straight lines along x (bundle 0) and along y (bundle 1) with uneven point spacing, half of them stored reversed"""
    lines, truth, rev = [], [], []
    for b in range(2):
        for i in range(nper):
            n = int(rng.integers(5, 40))
            s = np.sort(np.concatenate([[0.0, 1.0], rng.random(n - 2)]))
            p = np.empty((n, 3))
            p[:, b] = 3.0 + 20.0 * s
            p[:, 1 - b] = 12.0 + rng.uniform(-0.5, 0.5)
            p[:, 2] = 6.0 + rng.uniform(-0.5, 0.5)
            r = i % 2 == 1
            lines.append(p[::-1] if r else p)
            truth.append(b)
            rev.append(int(r))
    return lines, np.array(truth), np.array(rev)


def test_str_bundles_centroids_and_profile_on_two_analytic_bundles(fj, dev):
    rng = np.random.default_rng(9)
    lines, truth, rev = _two_bundles(rng)
    shape = (26, 26, 12)
    npts = np.array([p.shape[0] for p in lines], np.int32)
    tr = fj.Tract(np.concatenate(lines).astype(np.float32), npts, seed_index=np.arange(npts.size, dtype=np.int64), volsize=shape, volres=(1.0, 1.0, 2.0),
                  scalars=np.zeros(int(npts.sum()), np.float32), properties=np.arange(npts.size, dtype=np.float32))
    mx = np.array([[3, 12, 6], [23, 12, 6]], np.float32)                      # two-point models: resampled by the same kernel
    my = np.array([[12, 3, 6], [12, 23, 6]], np.float32)
    far = np.array([[3, 3, 60], [23, 23, 60]], np.float32)
    models = fj.Tract(np.concatenate([mx, my, far]), np.array([2, 2, 2], np.int32), volsize=shape, volres=(1.0, 1.0, 2.0))
    rs = fj.str_resample(tr, 20)
    assert rs.nstr == tr.nstr and (rs.npts == 20).all() and rs.scalars is None
    assert np.array_equal(rs.seed_index, tr.seed_index) and np.array_equal(rs.properties, tr.properties)
    assert np.array_equal(rs.xyz.reshape(-1, 20, 3), bd.resample(tr.xyz, npts, tr.volres, 20))
    b = fj.str_bundles(tr, models, thresh_mm=5.0, npoints=20)
    assert np.array_equal(b.label, truth) and np.array_equal(b.flip, rev) and b.npoints == 20
    assert list(b.counts) == [40, 40, 0] and int(b.counts.sum()) == tr.nstr and (b.dist < 1.5).all()
    assert np.array_equal(fj.str_bundles(rs, models, 5.0, 20).dist, b.dist)  # lines that have 20 points already go in as they are
    tight = fj.str_bundles(tr, models, thresh_mm=0.0, npoints=20)
    assert (tight.label == -1).all() and not tight.counts.any() and np.array_equal(tight.dist, b.dist)
    cen = fj.str_centroids(tr, b)
    assert cen.nstr == 3 and (cen.npts == 20).all() and list(cen.properties) == [40, 40, 0]
    cx = cen.xyz.reshape(3, 20, 3)
    ramp = 3.0 + 20.0 * np.arange(20) / 19.0
    assert np.allclose(cx[0, :, 0], ramp, atol=1e-4) and np.allclose(cx[1, :, 1], ramp, atol=1e-4) and np.isnan(cx[2]).all()
    assert np.abs(cx[0, :, 1] - 12).max() < 0.5 and np.abs(cx[1, :, 0] - 12).max() < 0.5
    # a volume that equals the x coordinate: the profile of the x bundle is the ramp (nearest voxel), that of the y bundle is flat
    vol = (np.arange(1, 27, dtype=np.float32)[:, None, None] + np.zeros(shape, np.float32))
    prof = fj.str_profile(tr, fj.MRI(vol), models, thresh_mm=5.0, npoints=20)
    assert prof.shape == (3, 20, 1) and prof.dtype == np.float32
    assert np.abs(prof[0, :, 0] - ramp).max() <= 0.5 + 1e-3 and (np.diff(prof[0, :, 0]) > 0).all()
    assert np.abs(prof[1, :, 0] - 12).max() <= 0.5 + 1e-3 and np.isnan(prof[2]).all()
    # the device tier in a refinement loop: assign -> centroids -> assign keeps the labels
    import torch
    a = torch.from_numpy(b.lines).to(dev)
    m = torch.from_numpy(np.stack([bd.resample(q, [2], tr.volres, 20)[0] for q in (mx, my, far)])).to(dev)
    r1 = fj.str_assign_device(a, m, tr.volres, 5.0)
    sums, counts = fj.str_centroids_device(a, r1["label"], r1["flip"], 3)
    m2 = (sums / counts.view(torch.int32).to(torch.float64)[:, None, None]).to(torch.float32)
    m2[2] = m[2]
    r2 = fj.str_assign_device(a, m2.contiguous(), tr.volres, 5.0)
    assert np.array_equal(_np(r2["label"]), truth) and np.array_equal(_np(r2["flip"]), rev) and (_np(r2["dist"]) <= _np(r1["dist"]).max()).all()
    fj.trim()
