"""Tract selection and connectomes on the GPU (csrc/tractsel.hip through the C ABI: fibd_str_* on device tensors, fib_str_* on host
arrays, and the Python layer on top) against the NumPy restatement of the header's definitions (tests/tractsel_ref.py, pinned by
tests/test_tractsel_ref.py).  Everything integer or copied -- keep, hits, counts, every output of the gather, C, assign, n_lines --
is compared BIT FOR BIT over every line.  W is a float64 sum whose order is free on the device: it is held to the bound derived in
the header, |W_gpu - W_ref| <= (n_max + m) * 2^-52 * W_ref per cell against the sequential float64 sums (the file is compiled with
contraction off, so every term is the same IEEE float64 value on both sides); cells with C == 0 must be exactly 0."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stream_rk_ref as rk  # noqa: E402
import tractmap_ref as tm  # noqa: E402
import tractsel_ref as ts  # noqa: E402

pytestmark = pytest.mark.gpu
FIB_ERR_INVALID, FIB_ERR_UNSUPPORTED = -1, -7
SHAPES = ((7, 6, 5), (9, 8, 7))
LENGTHS = (0, 1, 2, 15, 16, 17, 63, 64, 65, 255, 256, 257, 300)
B31 = 0x80000000
SENTINEL = 0x5A5A5A5A


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def _np(t):
    return t.cpu().numpy()


def _u32(dev, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.uint32).view(np.int32)).to(dev).view(torch.uint32)


def _to_dev(dev, xyz, npts):
    import torch
    return torch.from_numpy(np.ascontiguousarray(xyz, np.float32)).to(dev), torch.from_numpy(np.ascontiguousarray(npts, np.int32)).to(dev)


def _walks(rng, lengths, shape, step=0.35, wild=0.01, margin=0.1):
    """random walks folded back into a box `margin` larger than the volume on every face (about 10 % of the points are outside at 0.1),
    a few points replaced by NaN / Inf / 1e30"""
    out = []
    lo = 0.5 - margin
    w = np.array(shape, np.float64) + 2 * margin
    for n in lengths:
        if n == 0:
            continue
        d = rng.standard_normal((n, 3))
        d = np.cumsum(0.7 * d / np.linalg.norm(d, axis=1, keepdims=True) * step + 0.3 * step * rng.standard_normal(3), axis=0)
        p = rng.uniform(lo, lo + w, 3) + d
        out.append(lo + w - np.abs(np.mod(p - lo, 2 * w) - w))
    xyz = (np.concatenate(out) if out else np.zeros((0, 3))).astype(np.float32)
    bad = rng.random(xyz.shape[0]) < wild
    xyz[bad, rng.integers(0, 3, int(bad.sum()))] = rng.choice(np.array([np.nan, np.inf, -np.inf, 1e30, -1e30], np.float32), int(bad.sum()))
    return xyz


def _nodes_of_voxels(lab, remap, L):
    y = lab.astype(np.int64)
    if remap is not None:
        y = np.where((y >= 0) & (y < len(remap)), np.asarray(remap, np.int64)[np.clip(y, 0, len(remap) - 1)], 0)
    return np.where((y >= 1) & (y <= L), y, 0)


class Case:
    """257 random walks (a partial last group and workgroup), lengths from LENGTHS, one line of 100 000 points; 32 ROIs of byte values
    0 / 1 / 2 / 255; a label volume with negative labels and labels beyond remap; the restatement's answers, computed once"""

    def __init__(self, shape, seed):
        rng = np.random.default_rng(seed)
        self.shape = shape
        self.nvox = shape[0] * shape[1] * shape[2]
        n = np.concatenate([np.array(LENGTHS), rng.choice(np.array(LENGTHS), 257 - len(LENGTHS))]).astype(np.int32)
        rng.shuffle(n)
        n[100] = 100000
        self.npts = n
        self.xyz = _walks(rng, n, shape)
        with np.errstate(invalid="ignore"):                                   # the same lines with every wild point put at (3, 3, 3): all lengths finite
            self.clean = np.where(np.abs(self.xyz) < 1e29, self.xyz, np.float32(3.0)).astype(np.float32)
        self.rois = rng.choice(np.array([0, 0, 0, 0, 0, 0, 0, 1, 2, 255], np.uint8), (32, self.nvox))
        self.bits = ts.roi_pack(self.rois)
        self.hits = ts.hits(self.xyz, n, shape, self.bits)
        self.labels = rng.choice(np.array([-3, 0, 1, 2, 3, 4, 5, 6, 7, 9, 11, 1000], np.int32), self.nvox)
        self.remap = np.array([0, 3, 1, 2, 0, 6, 9, 5, 4, -2], np.int32)     # labels 9, 11, 1000, -3: beyond remap; 6 -> 9 > L; 9 -> -2
        self.L = 6
        self.volres = (1.25, 0.5, 2.0)
        assert abs(float((tm.voxel(self.xyz, shape) < 0).mean()) - 0.1) < 0.06


@pytest.fixture(scope="module")
def cases():
    return {s: Case(s, 21 + i) for i, s in enumerate(SHAPES)}


def _rules(nroi):
    top = 1 << (nroi - 1)                                                    # bit 31 when nroi = 32
    rs = [dict(), dict(visit_all=1), dict(visit_none=1), dict(visit_all=top), dict(visit_none=top), dict(end_any=top), dict(end_both=top),
          dict(end_any=1, min_npts=2), dict(min_npts=16, max_npts=64), dict(min_npts=257), dict(max_npts=1)]
    if nroi >= 5:
        rs += [dict(visit_all=0b00101, visit_none=0b01000, end_any=0b00001), dict(end_any=0b10001), dict(end_both=0b00011, max_npts=300)]
    if nroi == 32:
        rs += [dict(visit_all=B31 | 1, visit_none=1 << 17), dict(end_any=B31 | (1 << 30)), dict(visit_all=0xFFFFFFFF), dict(visit_none=0xFFFFFFFF)]
    return rs


def _select(fj, x, n, shape, bits, **kw):
    keep, hits, counts = fj.str_select_device(x, n, shape, bits, **kw)
    return _np(keep), _np(hits), [int(v) for v in _np(counts)]


# ---- ROI bits and selection --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("nroi", [1, 5, 32])
def test_roi_pack_and_select_on_random_walks(fj, dev, cases, shape, nroi):
    import torch
    c = cases[shape]
    bits = fj.str_roi_pack_device(torch.from_numpy(c.rois[:nroi].copy()).to(dev))
    ref_bits = c.bits & np.uint32((1 << nroi) - 1)
    assert set(np.unique(c.rois[:nroi])) == {0, 1, 2, 255}
    assert _np(bits).dtype == np.uint32 and np.array_equal(_np(bits), ref_bits) and np.array_equal(ref_bits, ts.roi_pack(c.rois[:nroi]))
    if nroi == 32:
        assert (ref_bits & np.uint32(B31)).any()
    x, n = _to_dev(dev, c.xyz, c.npts)
    ref_hits = c.hits & np.uint32((1 << nroi) - 1)
    for kw in _rules(nroi):
        keep, hits, counts = _select(fj, x, n, shape, bits, **kw)
        ref = ts.rule(ref_hits, c.npts, **kw)
        assert keep.dtype == np.uint8 and np.array_equal(keep, ref), (kw, np.flatnonzero(keep != ref)[:5])
        assert hits.dtype == np.uint32 and np.array_equal(hits, ref_hits), (kw, np.argwhere(hits != ref_hits)[:5])
        assert counts == [int(ref.sum()), int(c.npts[ref != 0].astype(np.int64).sum())], kw
    for r in (1, 1 << (nroi - 1)):                                            # keep(visit_all = r) + keep(visit_none = r) == 1 per line
        a = _select(fj, x, n, shape, bits, visit_all=r)[0]
        b = _select(fj, x, n, shape, bits, visit_none=r)[0]
        assert (a.astype(int) + b == 1).all() and 0 < a.sum() < a.size
    # no ROIs at all: every line is kept, the empty ones too
    keep, hits, counts = fj.str_select_device(x, n, shape, None)
    assert _np(keep).all() and not _np(hits).any() and [int(v) for v in _np(counts)] == [c.npts.size, int(c.npts.sum())]


def test_select_on_a_4_byte_aligned_view_and_a_side_stream(fj, dev, cases):
    import torch
    c = cases[SHAPES[1]]
    bits = _u32(dev, c.bits)
    base = torch.zeros(c.xyz.size + 8, dtype=torch.float32, device=dev)
    assert base.data_ptr() % 16 == 0
    view = base[1:1 + c.xyz.size].view(-1, 3)                                 # offset by one float
    view.copy_(torch.from_numpy(c.xyz).to(dev))
    assert view.data_ptr() % 16 == 4
    n = torch.from_numpy(c.npts).to(dev)
    kw = dict(visit_all=5, end_any=B31)
    ref = ts.rule(c.hits, c.npts, **kw)
    keep, hits, _ = _select(fj, view, n, c.shape, bits, **kw)
    assert np.array_equal(keep, ref) and np.array_equal(hits, c.hits)
    g = fj.str_gather_device(view, n, torch.from_numpy(ref).to(dev))
    rx, rn, ri, _ = ts.gather(c.xyz, c.npts, ref)
    nk, npk, status = (int(v) for v in _np(g["counts"]))
    assert (nk, npk, status) == (rn.size, rx.shape[0], 0)
    assert np.array_equal(_np(g["xyz"])[:npk].view(np.uint32), rx.view(np.uint32)) and np.array_equal(_np(g["npts"])[:nk], rn)
    lab = torch.from_numpy(c.labels).to(dev)
    r = fj.str_connectome_device(view, n, c.shape, lab, 11)
    assert np.array_equal(_np(r["counts"]), ts.connectome(c.xyz, c.npts, c.shape, c.labels, 11)[0])
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        keep, hits, counts = fj.str_select_device(view, n, c.shape, bits, stream=side, **kw)
        g = fj.str_gather_device(view, n, keep, stream=side)
    side.synchronize()
    assert np.array_equal(_np(keep), ref) and int(_np(g["counts"])[1]) == rx.shape[0]
    assert np.array_equal(_np(g["xyz"])[:npk].view(np.uint32), rx.view(np.uint32)) and np.array_equal(_np(g["index"])[:nk], ri)


def test_the_tracers_own_output_without_a_copy(fj, dev):
    """the circular field of tests/stream_rk_ref.py, RK4, from every voxel: selection by an ROI on the circle, and the connectome of a
    two-label split of the volume"""
    import torch
    nx, ny, nz = rk.CIRCLE_SHAPE
    ov = rk.circle_field()
    planar = torch.from_numpy(np.ascontiguousarray(ov.reshape(nx * ny * nz, 3, order="F").T)).to(dev)
    field, mout = fj.stream_field_device([planar], mask=torch.ones(nx * ny * nz, dtype=torch.uint8, device=dev))
    seeds = torch.nonzero(mout).flatten()
    r = fj.stream_device_run(field, rk.CIRCLE_SHAPE, seeds, torch.from_numpy(rk.CIRCLE_SUB).to(dev), len_max=200, smooth_coeff=0.0,
                             interp="trilinear", integrator="rk4")
    x, n = r["xyz"], r["npts"]
    hx, hn = _np(x).reshape(-1, 3), _np(n)
    assert hn.size > 1000
    X, Y, Z = np.meshgrid(np.arange(1, nx + 1), np.arange(1, ny + 1), np.arange(1, nz + 1), indexing="ij")
    rad = np.hypot(X - rk.CIRCLE_C, Y - rk.CIRCLE_C)
    rois = np.stack([r.reshape(-1, order="F") for r in ((rad > 10) & (rad < 12) & (X > 30), (rad > 10) & (rad < 12) & (X < 18), rad < 6)]).astype(np.uint8)
    bits = fj.str_roi_pack_device(torch.from_numpy(rois).to(dev))
    assert np.array_equal(_np(bits), ts.roi_pack(rois))
    ref_hits = ts.hits(hx, hn, rk.CIRCLE_SHAPE, _np(bits))
    for kw in (dict(visit_all=3), dict(visit_all=1, visit_none=4), dict(end_any=1), dict(end_both=4, min_npts=100), dict(visit_none=7)):
        keep, hits, counts = _select(fj, x, n, rk.CIRCLE_SHAPE, bits, **kw)
        ref = ts.rule(ref_hits, hn, **kw)
        assert np.array_equal(keep, ref) and np.array_equal(hits, ref_hits) and counts == [int(ref.sum()), int(hn[ref != 0].sum())]
        assert 0 < ref.sum() < ref.size, kw
    lab = np.where(X <= 24, 1, 2).astype(np.int32).reshape(-1, order="F")
    got = fj.str_connectome_device(x, n, rk.CIRCLE_SHAPE, torch.from_numpy(lab).to(dev), 2, volres=(1.0, 1.0, 2.0))
    Cr, Wr, ar, nr, bound = ts.connectome(hx, hn, rk.CIRCLE_SHAPE, lab, 2, volres=(1.0, 1.0, 2.0))
    assert np.array_equal(_np(got["counts"]), Cr) and np.array_equal(_np(got["assign"]), ar) and int(got["n_lines"].item()) == nr
    assert Cr[1, 2] > 0 and Cr[1, 1] > 0 and Cr[2, 2] > 0
    assert ts.weights_close(_np(got["lengths"]), Wr, bound, Cr).all()


# ---- gather ------------------------------------------------------------------------------------------------------------------------
def _check_gather(fj, dev, xyz, npts, flags, sc=None, what=""):
    import torch
    x, n = _to_dev(dev, xyz, npts)
    k = torch.from_numpy(np.ascontiguousarray(flags)).to(dev)
    s = None if sc is None else torch.from_numpy(sc).to(dev)
    g = fj.str_gather_device(x, n, k, s)
    rx, rn, ri, rs = ts.gather(xyz, npts, flags, sc)
    nk, npk, status = (int(v) for v in _np(g["counts"]))
    assert (nk, npk, status) == (rn.size, rx.shape[0], 0), what
    assert np.array_equal(_np(g["xyz"])[:npk].view(np.uint32), rx.view(np.uint32)), what                   # the bytes, NaN payloads included
    assert np.array_equal(_np(g["npts"])[:nk], rn) and np.array_equal(_np(g["index"])[:nk], ri), what
    if sc is not None:
        assert np.array_equal(_np(g["scalars"])[:npk].view(np.uint32), rs.view(np.uint32)), what
    return g, rx, rn


@pytest.mark.parametrize("shape", SHAPES)
def test_gather_with_given_flags(fj, dev, cases, shape):
    c = cases[shape]
    rng = np.random.default_rng(31)
    xyz = c.xyz.copy()
    xyz.view(np.uint32)[5, 1] = 0x7FC12345                                    # a NaN with a payload, a signalling-pattern NaN, -0.0
    xyz.view(np.uint32)[6, 0] = 0xFFA00001
    xyz[7, 2] = -0.0
    sc = rng.standard_normal((xyz.shape[0], 2)).astype(np.float32)
    sc.view(np.uint32)[9, 1] = 0x7F800001
    nl = c.npts.size
    g, rx, _ = _check_gather(fj, dev, xyz, c.npts, np.ones(nl, np.uint8), sc, "all")
    assert np.array_equal(_np(g["xyz"]).view(np.uint32), xyz.view(np.uint32)) and np.array_equal(_np(g["npts"]), c.npts)
    assert np.array_equal(_np(g["scalars"]).view(np.uint32), sc.view(np.uint32)) and _np(g["xyz"]).view(np.uint32)[5, 1] == 0x7FC12345
    _check_gather(fj, dev, xyz, c.npts, np.zeros(nl, np.uint8), sc, "none")
    _check_gather(fj, dev, xyz, c.npts, (np.arange(nl) % 2).astype(np.uint8), sc, "alternate")
    _check_gather(fj, dev, xyz, c.npts, (np.arange(nl) % 2 == 0), None, "alternate, bool, no scalars")
    flags = rng.choice(np.array([0, 0, 1, 3, 128, 255], np.uint8), nl)       # flags that no select made: any non-zero byte keeps
    flags[100] = 0
    _check_gather(fj, dev, xyz, c.npts, flags, sc[:, :1].copy(), "free flags without the long line")
    flags[100] = 7
    g, rx, rn = _check_gather(fj, dev, xyz, c.npts, flags, sc, "free flags")
    # the LINES density of the gathered lines equals the restatement's
    nk, npk = int(_np(g["counts"])[0]), int(_np(g["counts"])[1])
    d, nout = fj.str_density_device(g["xyz"][:npk], g["npts"][:nk], shape, "lines")
    ref, rout = tm.density(rx, rn, shape, tm.LINES)
    assert np.array_equal(_np(d), ref) and int(nout.item()) == rout


def test_gather_capacities(fj, dev, cases):
    import torch
    c = cases[SHAPES[0]]
    x, n = _to_dev(dev, c.xyz, c.npts)
    flags = (np.arange(c.npts.size) % 3 != 0).astype(np.uint8)
    rx, rn, ri, _ = ts.gather(c.xyz, c.npts, flags)
    sc = torch.arange(c.xyz.shape[0], dtype=torch.float32, device=dev).view(-1, 1)
    k = torch.from_numpy(flags).to(dev)

    def outputs(cl, cp):
        return dict(xyz=torch.full((cp, 3), SENTINEL, dtype=torch.int32, device=dev).view(torch.float32), npts=torch.full((cl,), SENTINEL, dtype=torch.int32, device=dev),
                    index=torch.full((cl,), SENTINEL, dtype=torch.int64, device=dev), scalars=torch.full((cp, 1), SENTINEL, dtype=torch.int32, device=dev).view(torch.float32),
                    counts=torch.full((3,), 99, dtype=torch.int64, device=dev))

    for cl, cp in ((rn.size - 1, rx.shape[0]), (rn.size, rx.shape[0] - 1), (0, 0)):
        out = outputs(cl, cp)
        g = fj.str_gather_device(x, n, k, sc, out=out)
        assert [int(v) for v in _np(g["counts"])] == [rn.size, rx.shape[0], -1]                            # the true totals, status -1
        for name in ("xyz", "npts", "scalars"):
            assert (_np(out[name]).view(np.uint32) == SENTINEL).all(), (cl, cp, name)                      # nothing is changed
        assert (_np(out["index"]) == SENTINEL).all()
    out = outputs(rn.size, rx.shape[0])                                       # exactly enough
    g = fj.str_gather_device(x, n, k, sc, out=out)
    assert [int(v) for v in _np(g["counts"])] == [rn.size, rx.shape[0], 0]
    assert np.array_equal(_np(out["xyz"]).view(np.uint32), rx.view(np.uint32)) and np.array_equal(_np(out["npts"]), rn) and np.array_equal(_np(out["index"]), ri)


# ---- connectome --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_connectome_on_random_walks(fj, dev, cases, shape):
    import torch
    c = cases[shape]
    x, n = _to_dev(dev, c.xyz, c.npts)
    lab = torch.from_numpy(c.labels).to(dev)
    ends = _np(fj.str_density_device(x, n, shape, "endpoints")[0]).astype(np.int64)
    for L, remap in ((c.L, c.remap), (11, None), (4, None), (9, c.remap)):
        rm = None if remap is None else torch.from_numpy(remap).to(dev)
        Cr, Wr, ar, nr, bound = ts.connectome(c.xyz, c.npts, shape, c.labels, L, remap, volres=c.volres)
        # W of the lines with their wild points made finite: every cell is finite, the line of 100 000 points sets the bound of its cell
        Cc, Wc, _, _, bc = ts.connectome(c.clean, c.npts, shape, c.labels, L, remap, volres=c.volres)
        gc = fj.str_connectome_device(_to_dev(dev, c.clean, c.npts)[0], n, shape, lab, L, remap=rm, volres=c.volres)
        assert np.isfinite(Wc).all() and np.array_equal(_np(gc["counts"]), Cc)
        ok = ts.weights_close(_np(gc["lengths"]), Wc, bc, Cc)
        assert ok.all(), (L, np.argwhere(~ok)[:5], _np(gc["lengths"])[~ok][:5], Wc[~ok][:5])
        for volres in (None, c.volres):
            got = fj.str_connectome_device(x, n, shape, lab, L, remap=rm, volres=volres)
            Cg = _np(got["counts"])
            assert Cg.dtype == np.uint32 and Cg.shape == (L + 1, L + 1) and np.array_equal(Cg, Cr), (L, np.argwhere(Cg != Cr)[:5])
            assert np.array_equal(_np(got["assign"]), ar) and int(got["n_lines"].item()) == nr == int((c.npts >= 1).sum())
            if volres is None:
                assert got["lengths"] is None
                continue
            Wg = _np(got["lengths"])
            ok = ts.weights_close(Wg, Wr, bound, Cr)
            assert ok.all(), (L, np.argwhere(~ok)[:5], Wg[~ok][:5], Wr[~ok][:5])
            assert (Wg[Cr == 0] == 0).all() and np.isfinite(Wr[Cr > 0]).any()
        # identities on the GPU result: symmetric; the upper triangle with the diagonal counts every non-empty line once; a node's row
        # counts the line ends in its voxels, which the ENDPOINTS density of the same lines counts too
        Ci = Cg.astype(np.int64)
        assert np.array_equal(Cg, Cg.T) and int(np.triu(Ci).sum()) == int((c.npts >= 1).sum())
        nodes = _nodes_of_voxels(c.labels, remap, L)
        for i in range(1, L + 1):
            assert Ci[i, i] + Ci[i].sum() == int(ends[nodes == i].sum()), (L, i)
    assert fj.str_connectome_device(x, n, shape, lab, 3, assign=False)["assign"] is None


def test_connectome_in_batches_and_composition_with_gather(fj, dev, cases):
    import torch
    c = cases[SHAPES[1]]
    x, n = _to_dev(dev, c.xyz, c.npts)
    lab, rm = torch.from_numpy(c.labels).to(dev), torch.from_numpy(c.remap).to(dev)
    whole = fj.str_connectome_device(x, n, c.shape, lab, c.L, remap=rm, volres=c.volres)
    Cr, Wr, ar, nr, bound = ts.connectome(c.xyz, c.npts, c.shape, c.labels, c.L, c.remap, volres=c.volres)
    assert np.array_equal(_np(whole["counts"]), Cr)
    off = np.concatenate([[0], np.cumsum(c.npts.astype(np.int64))])
    cuts = [(0, 90), (90, 101), (101, c.npts.size)]
    for order in ((0, 1, 2), (2, 0, 1)):
        acc, total = None, 0
        for b in order:
            l0, l1 = cuts[b]
            acc = fj.str_connectome_device(x[off[l0]:off[l1]], n[l0:l1], c.shape, lab, c.L, remap=rm, volres=c.volres, out=acc)
            total += int(acc["n_lines"].item())
            assert np.array_equal(_np(acc["assign"]), ar[l0:l1])
        assert np.array_equal(_np(acc["counts"]).view(np.uint8), _np(whole["counts"]).view(np.uint8)) and total == nr          # the same bytes as one call
        assert ts.weights_close(_np(acc["lengths"]), Wr, bound, Cr).all()
    # the bundle between nodes 2 and 5: flags made from `assign` with torch, through the gather
    a = whole["assign"]
    flags = ((a[:, 0] == 2) & (a[:, 1] == 5)) | ((a[:, 0] == 5) & (a[:, 1] == 2))
    g = fj.str_gather_device(x, n, flags)
    ref_flags = np.array([{int(p), int(q)} == {2, 5} for p, q in ar])
    rx, rn, ri, _ = ts.gather(c.xyz, c.npts, ref_flags)
    nk, npk, status = (int(v) for v in _np(g["counts"]))
    assert nk == rn.size == int(Cr[2, 5]) > 0 and npk == rx.shape[0] and status == 0
    assert np.array_equal(_np(g["xyz"])[:npk].view(np.uint32), rx.view(np.uint32)) and np.array_equal(_np(g["npts"])[:nk], rn)
    assert np.array_equal(_np(g["index"])[:nk], ri)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def test_invalid_counts_are_refused(fj, dev, cases):
    import torch
    c = cases[SHAPES[0]]
    x, _ = _to_dev(dev, c.xyz, c.npts)
    short = c.npts.copy(); short[200] = max(0, short[200] - 1); short[3] += 2                        # sum != npoints
    neg = c.npts.copy(); neg[256] = -3; neg[0] += 3 + c.npts[256]                                     # a negative count, the sum still right
    assert short.sum() != c.npts.sum() and neg.sum() == c.npts.sum()
    bits, lab = _u32(dev, c.bits), torch.from_numpy(c.labels).to(dev)
    L = fj.lib()
    nl = c.npts.size
    rois = [np.ascontiguousarray(r) for r in c.rois[:2]]
    ptrs = (C.c_void_p * 2)(*[r.ctypes.data for r in rois])
    res = (C.c_float * 3)(1, 1, 1)
    for bad in (short, neg):
        n = torch.from_numpy(bad).to(dev)
        work = torch.empty(fj.str_select_work_size(nl) // 8 + 1, dtype=torch.int64, device=dev)
        keep = torch.full((nl,), 9, dtype=torch.uint8, device=dev)
        hits = torch.full((nl, 3), SENTINEL, dtype=torch.int32, device=dev)
        counts = torch.full((2,), 99, dtype=torch.int64, device=dev)
        assert L.fibd_str_select(x.data_ptr(), n.data_ptr(), nl, c.xyz.shape[0], *c.shape, bits.data_ptr(), 1, 0, 0, 0, 0, 0, keep.data_ptr(),
                                 hits.data_ptr(), counts.data_ptr(), work.data_ptr(), work.numel() * 8, None) == 0
        torch.cuda.synchronize()
        assert not _np(keep).any() and (_np(hits).view(np.uint32) == SENTINEL).all() and list(_np(counts)) == [-1, -1]   # keep zero-filled, hits untouched
        out = dict(xyz=torch.full((c.xyz.shape[0], 3), SENTINEL, dtype=torch.int32, device=dev).view(torch.float32),
                   npts=torch.full((nl,), SENTINEL, dtype=torch.int32, device=dev), index=torch.full((nl,), SENTINEL, dtype=torch.int64, device=dev),
                   counts=torch.full((3,), 99, dtype=torch.int64, device=dev))
        g = fj.str_gather_device(x, n, torch.ones(nl, dtype=torch.uint8, device=dev), out=out)
        assert list(_np(g["counts"]))[:2] == [-1, -1]
        assert (_np(out["xyz"]).view(np.uint32) == SENTINEL).all() and (_np(out["npts"]) == SENTINEL).all() and (_np(out["index"]) == SENTINEL).all()
        got = fj.str_connectome_device(x, n, c.shape, lab, 11, volres=(1, 1, 1))
        assert int(got["n_lines"].item()) == -1 and not _np(got["counts"]).any() and not _np(got["lengths"]).any()       # zero-filled, nothing added
        before = dict(counts=_u32(dev, np.arange(144, dtype=np.uint32).reshape(12, 12)), lengths=torch.full((12, 12), 2.5, dtype=torch.float64, device=dev))
        got = fj.str_connectome_device(x, n, c.shape, lab, 11, volres=(1, 1, 1), out=before)
        assert int(got["n_lines"].item()) == -1 and np.array_equal(_np(got["counts"]).reshape(-1), np.arange(144)) and (_np(got["lengths"]) == 2.5).all()
        # host forms: FIB_ERR_INVALID, outputs untouched
        hk, hh, hc = np.full(nl, 9, np.uint8), np.full((nl, 3), SENTINEL, np.uint32), (C.c_int64 * 2)(77, 77)
        assert L.fib_str_select(0, c.xyz.ctypes.data, bad.ctypes.data, nl, c.xyz.shape[0], *c.shape, ptrs, 2, 1, 2, 0, 0, 0, 0, hk.ctypes.data,
                                hh.ctypes.data, hc) == FIB_ERR_INVALID
        assert (hk == 9).all() and (hh == SENTINEL).all() and list(hc) == [77, 77]
        hC, hW, ha, hn = np.full((12, 12), 7, np.uint32), np.full((12, 12), 2.5), np.full((nl, 2), 7, np.int32), C.c_int64(77)
        assert L.fib_str_connectome(0, c.xyz.ctypes.data, bad.ctypes.data, nl, c.xyz.shape[0], *c.shape, res, c.labels.ctypes.data, None, 0, 11, 0,
                                    hC.ctypes.data, hW.ctypes.data, ha.ctypes.data, C.byref(hn)) == FIB_ERR_INVALID
        assert (hC == 7).all() and (hW == 2.5).all() and (ha == 7).all() and hn.value == 77
    # arguments the host can judge
    n = torch.from_numpy(c.npts).to(dev)
    work = torch.empty(fj.str_select_work_size(nl) // 8 + 1, dtype=torch.int64, device=dev)
    keep, counts = torch.zeros(nl, dtype=torch.uint8, device=dev), torch.zeros(3, dtype=torch.int64, device=dev)
    args = (x.data_ptr(), n.data_ptr(), nl, c.xyz.shape[0], *c.shape, bits.data_ptr())
    assert L.fibd_str_select(*args, 1 << 32, 0, 0, 0, 0, 0, keep.data_ptr(), None, counts.data_ptr(), work.data_ptr(), work.numel() * 8, None) == FIB_ERR_INVALID
    assert L.fibd_str_select(*args, 1, 0, 0, 0, 0, 0, keep.data_ptr(), None, counts.data_ptr(), work.data_ptr(), 64, None) == FIB_ERR_INVALID       # work too small
    assert L.fibd_str_roi_pack(bits.data_ptr(), 33, c.nvox, bits.data_ptr(), None) == FIB_ERR_INVALID
    torch.cuda.synchronize()


# ---- host forms and the Python layer -----------------------------------------------------------------------------------------------
def test_host_forms_and_python_layer_over_several_chunks(fj, dev):
    """more points than one chunk of the host forms holds (2^22, cut at line boundaries; there is no hook to make it smaller), as a
    `Tract` with scalars, properties and seed_index"""
    rng = np.random.default_rng(41)
    shape = (24, 20, 16)
    nvox = 24 * 20 * 16
    npts = np.concatenate([[0, 1], rng.integers(0, 4000, 2300), [0]]).astype(np.int32)
    npnt = int(npts.sum())
    assert npnt > (1 << 22)
    xyz = (rng.random((npnt, 3), dtype=np.float32) * (np.array(shape, np.float32) + 1.0)).astype(np.float32)
    short = np.flatnonzero(npts < 4000)                                       # most lines visit everything: make some lines local
    off = np.concatenate([[0], np.cumsum(npts.astype(np.int64))])
    for l in short[::2]:
        xyz[off[l]:off[l + 1]] = (rng.uniform(1, np.array(shape)) + rng.uniform(-1.5, 1.5, (npts[l], 3))).astype(np.float32)
    X = np.arange(1, 25)[:, None, None] + np.zeros(shape, int)
    Zc = np.arange(1, 17)[None, None, :] + np.zeros(shape, int)
    Yc = np.arange(1, 21)[None, :, None] + np.zeros(shape, int)
    roi_a, roi_b, roi_c = (X <= 8).astype(np.uint8), ((Yc > 10) * 200).astype(np.uint8), (Zc > 12).astype(np.float32)
    tr = fj.Tract(xyz, npts, seed_index=np.arange(npts.size, dtype=np.int64)[::-1].copy(), volsize=shape, volres=(1.0, 2.0, 0.5),
                  scalars=rng.standard_normal((npnt, 2)).astype(np.float32), properties=rng.standard_normal((npts.size, 3)).astype(np.float32))
    out = fj.str_select(tr, include=[fj.MRI(roi_a)], exclude=roi_c, end_in=[roi_b], min_npts=3, max_npts=3500)
    rois = np.stack([roi_a.reshape(-1, order="F"), (roi_c != 0).astype(np.uint8).reshape(-1, order="F"), roi_b.reshape(-1, order="F")])
    keep, hits, counts = ts.select(xyz, npts, shape, ts.roi_pack(rois), visit_all=1, visit_none=2, end_any=4, min_npts=3, max_npts=3500)
    rx, rn, ri, rs = ts.gather(xyz, npts, keep, tr.scalars)
    assert 0 < counts[0] < npts.size and out.nstr == counts[0]
    assert np.array_equal(out.xyz.view(np.uint32), rx.view(np.uint32)) and np.array_equal(out.npts, rn) and np.array_equal(out.index, ri)
    assert np.array_equal(out.scalars, rs) and np.array_equal(out.properties, tr.properties[ri]) and np.array_equal(out.seed_index, tr.seed_index[ri])
    assert np.array_equal(out.hits, hits[keep != 0]) and tuple(out.volsize) == shape and tr.nstr == npts.size
    # the C entry point itself: keep and hits of every line, the counts
    L = fj.lib()
    hk, hh, hc = np.zeros(npts.size, np.uint8), np.zeros((npts.size, 3), np.uint32), (C.c_int64 * 2)()
    planes = [np.ascontiguousarray(r) for r in rois]
    ptrs = (C.c_void_p * 33)(*([p.ctypes.data for p in planes] + [planes[0].ctypes.data] * 30))
    args = (xyz.ctypes.data, npts.ctypes.data, npts.size, npnt, *shape, ptrs)
    assert L.fib_str_select(0, *args, 3, 1, 2, 4, 0, 3, 3500, hk.ctypes.data, hh.ctypes.data, hc) == 0
    assert np.array_equal(hk, keep) and np.array_equal(hh, hits) and list(hc) == counts
    assert L.fib_str_select(-1, *args, 3, 1, 2, 4, 0, 3, 3500, hk.ctypes.data, hh.ctypes.data, hc) == FIB_ERR_UNSUPPORTED       # FIB_DEVICE_ALL
    assert b"FIB_DEVICE_ALL" in L.fib_last_error()
    assert L.fib_str_select(0, *args, 33, 1, 2, 4, 0, 3, 3500, hk.ctypes.data, hh.ctypes.data, hc) == FIB_ERR_INVALID
    assert b"32" in L.fib_last_error()
    # connectome: ids default to the sorted unique positive labels
    lab = (rng.integers(0, 9, shape) * 10).astype(np.int32)
    lab[0, 0, 0] = -5
    con = fj.str_connectome(tr, fj.MRI(lab))
    assert list(con.ids) == [10, 20, 30, 40, 50, 60, 70, 80]
    remap = np.zeros(81, np.int32)
    remap[con.ids] = np.arange(1, 9)
    Cr, Wr, ar, nr, bound = ts.connectome(xyz, npts, shape, lab.reshape(-1, order="F"), 8, remap, volres=tr.volres)
    assert con.counts.dtype == np.uint32 and np.array_equal(con.counts, Cr) and np.array_equal(con.assign, ar) and con.n_lines == nr
    assert ts.weights_close(con.total_length, Wr, bound, Cr).all()
    assert np.array_equal(con.mean_length, ts.mean_length(Cr, con.total_length)) and con.mean_length.dtype == np.float64
    sub = fj.str_connectome(tr, lab, ids=[30, 10], lengths=False)
    Cs = ts.connectome(xyz, npts, shape, lab.reshape(-1, order="F"), 2, np.array([0] * 10 + [2] + [0] * 19 + [1], np.int32))[0]
    assert sub.mean_length is None and np.array_equal(sub.counts, Cs)
    hC, hn = np.zeros((9, 9), np.uint32), C.c_int64(0)
    labf = np.ascontiguousarray(lab.reshape(-1, order="F"))
    cargs = (xyz.ctypes.data, npts.ctypes.data, npts.size, npnt, *shape, None, labf.ctypes.data, remap.ctypes.data, 81, 8)
    assert L.fib_str_connectome(-1, *cargs, 0, hC.ctypes.data, None, None, C.byref(hn)) == FIB_ERR_UNSUPPORTED
    hC[:] = Cr
    assert L.fib_str_connectome(0, *cargs, 0x100, hC.ctypes.data, None, None, C.byref(hn)) == 0                                  # ACCUMULATE
    assert np.array_equal(hC, 2 * Cr) and hn.value == nr
    fj.trim()
