"""Tract maps on the GPU (csrc/tractmap.hip through the C ABI: fibd_str_* on device tensors, fib_str_* on host arrays, and the Python
layer on top) against the NumPy restatement of the header's definitions (tests/tractmap_ref.py, pinned by
tests/test_tractmap_ref.py).  Counts are integers and a sample is a gather, so maps and samples are compared BIT FOR BIT, over every
voxel / point of every input.  The statistics are float64 sums whose order is free on the device: they are held to the tolerance
derived in the header, |gpu - ref| <= ulp32(ref) + n * 2^-52 * sum|t_i| / d, against the sequential float64 result (the file is
compiled with contraction off, so every term is the same IEEE float64 value on both sides)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stream_rk_ref as rk  # noqa: E402
import tractmap_ref as tm  # noqa: E402
from test_tractmap_ref import SHAPE as WSHAPE, witnesses  # noqa: E402

pytestmark = pytest.mark.gpu
FIB_ERR_INVALID, FIB_ERR_UNSUPPORTED = -1, -7
ACC = 0x100
MODES = (("points", tm.POINTS), ("lines", tm.LINES), ("endpoints", tm.ENDPOINTS))


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def _np(t):
    return t.cpu().numpy()


def _check_density(fj, xyz, npts, shape, what=""):
    """the three modes of the device form on device tensors, every voxel, and n_outside, against the restatement; returns the maps"""
    hx, hn = _np(xyz).reshape(-1, 3), _np(npts)
    maps = {}
    for name, code in MODES:
        d, nout = fj.str_density_device(xyz, npts, shape, name)
        ref, rout = tm.density(hx, hn, shape, code)
        got = _np(d)
        assert got.dtype == np.uint32 and np.array_equal(got, ref), (what, name, int((got != ref).sum()))
        assert int(nout.item()) == rout, (what, name, int(nout.item()), rout)
        maps[name] = got
    assert int(maps["points"].sum(dtype=np.int64)) + tm.density(hx, hn, shape, tm.POINTS)[1] == hx.shape[0]
    assert (maps["lines"] <= maps["points"]).all()
    return maps


def _check_sample_and_stats(fj, xyz, npts, shape, volres, rng, what="", frames=(1, 3)):
    import torch
    hx, hn = _np(xyz).reshape(-1, 3), _np(npts)
    nvox = shape[0] * shape[1] * shape[2]
    last = None
    for nf in frames:
        vol = rng.standard_normal((nf, nvox)).astype(np.float32)
        s = fj.str_sample_device(xyz, torch.from_numpy(vol).to(xyz.device), shape, outside=float("nan"))
        ref = tm.sample(hx, vol, shape, outside=np.nan)
        assert s.shape == (hx.shape[0], nf) and np.array_equal(_np(s), ref, equal_nan=True), (what, nf)
        last = s
    for sc in (None, last):
        p = fj.str_stats_device(xyz, npts, volres, sc)
        ref, bound = tm.stats(hx, hn, volres, None if sc is None else _np(sc))
        got = _np(p)
        assert got.shape == ref.shape
        ok = tm.stats_close(got, ref, bound)
        assert ok.all(), (what, np.argwhere(~ok)[:5], got[~ok][:5], ref[~ok][:5])


# ---- the tracer's own output, fed to the device forms without a copy ---------------------------------------------------------------
def _circle_lines(fj, dev, len_max):
    import torch
    nx, ny, nz = rk.CIRCLE_SHAPE
    ov = rk.circle_field()
    planar = torch.from_numpy(np.ascontiguousarray(ov.reshape(nx * ny * nz, 3, order="F").T)).to(dev)
    field, mout = fj.stream_field_device([planar], mask=torch.ones(nx * ny * nz, dtype=torch.uint8, device=dev))
    seeds = torch.nonzero(mout).flatten()
    sub = torch.from_numpy(rk.CIRCLE_SUB).to(dev)
    return fj.stream_device_run(field, rk.CIRCLE_SHAPE, seeds, sub, len_max=len_max, smooth_coeff=0.0, interp="trilinear", integrator="rk4")


@pytest.mark.parametrize("len_max", [200, 600])
def test_lines_that_come_back_to_voxels_they_have_left(fj, dev, len_max):
    """the circular field of tests/test_gpu_stream_rk.py, RK4, from every voxel: 100 (300) voxels of arc on circles of 3 to 150 voxels
    of circumference -- lines go round several times.  len_max 200: every line fits the LDS tile of mode 1; 600: most do not"""
    r = _circle_lines(fj, dev, len_max)
    n = _np(r["npts"])
    assert n.size > 1000 and n.max() == len_max + 2 and ((n > 256).any() == (len_max > 254))
    maps = _check_density(fj, r["xyz"], r["npts"], rk.CIRCLE_SHAPE, "circle")
    # re-entries are what this case is about: more runs of equal voxels (what merging consecutive points leaves) than (line, voxel) pairs
    lin = tm.voxel(_np(r["xyz"]), rk.CIRCLE_SHAPE)
    first = np.zeros(lin.size, bool)
    first[np.concatenate([[0], np.cumsum(n.astype(np.int64))[:-1]])] = True
    runs = int((first | (lin != np.roll(lin, 1))).sum())
    pairs = int(maps["lines"].sum(dtype=np.int64))
    print("circle len_max %d: %d lines, %d points, %d runs, %d (line, voxel) pairs" % (len_max, n.size, lin.size, runs, pairs))
    assert runs > pairs
    _check_sample_and_stats(fj, r["xyz"], r["npts"], rk.CIRCLE_SHAPE, (1.0, 1.0, 2.0), np.random.default_rng(len_max), "circle")


@pytest.mark.parametrize("nvec", [1, 3])
def test_bundle_phantom_lines(fj, dev, nvec):
    import torch
    from fibers_jl_amd import phantom
    shape = (40, 36, 32)
    ovs, mask = [], None
    for k in range(nvec):
        ov, m = phantom.bundle_field_torch(shape, dev, seed=7 + k, cell=9.0)
        ovs.append(ov)
        mask = m if mask is None else (mask | m)
    field, mout = fj.stream_field_device(ovs, mask=mask)
    seeds = torch.nonzero(mout).flatten()
    sub = torch.tensor([[0.1, -0.2, 0.3], [-0.3, 0.25, 0.0]], dtype=torch.float32, device=dev)
    r = fj.stream_device_run(field, shape, seeds, sub)
    assert r["npts"].numel() > 5000
    _check_density(fj, r["xyz"], r["npts"], shape, "bundle%d" % nvec)
    _check_sample_and_stats(fj, r["xyz"], r["npts"], shape, (1.25, 1.25, 2.5), np.random.default_rng(nvec), "bundle%d" % nvec)
    # a map of another size than the volume the lines were traced in: points beyond it are outside
    small = (20, 36, 16)
    _check_density(fj, r["xyz"], r["npts"], small, "bundle%d small" % nvec)


# ---- synthetic lines ---------------------------------------------------------------------------------------------------------------
def _walks(rng, lengths, shape, step=0.35, wild=0.01):
    """random walks (so that consecutive points share voxels and lines cross themselves), folded back into a box a little larger than the volume, a few
    points replaced by NaN / Inf / 1e30"""
    out = []
    hi = np.array(shape, np.float64) + 1.2
    for n in lengths:
        if n == 0:
            continue
        d = rng.standard_normal((n, 3))
        d = np.cumsum(0.7 * d / np.linalg.norm(d, axis=1, keepdims=True) * step + 0.3 * step * rng.standard_normal(3), axis=0)
        p = rng.uniform(0.3, hi, 3) + d
        w = hi - 0.2                                                          # folded back and forth between 0.2 and a little beyond the far faces
        p = 0.2 + w - np.abs(np.mod(p - 0.2, 2 * w) - w)
        out.append(p)
    xyz = (np.concatenate(out) if out else np.zeros((0, 3))).astype(np.float32)
    bad = rng.random(xyz.shape[0]) < wild
    xyz[bad, rng.integers(0, 3, int(bad.sum()))] = rng.choice(np.array([np.nan, np.inf, -np.inf, 1e30, -1e30], np.float32), int(bad.sum()))
    return xyz


def _to_dev(dev, xyz, npts):
    import torch
    return torch.from_numpy(np.ascontiguousarray(xyz, np.float32)).to(dev), torch.from_numpy(np.asarray(npts, np.int32)).to(dev)


def test_random_lines_with_empty_lines(fj, dev):
    rng = np.random.default_rng(11)
    shape = (14, 9, 11)
    lengths = np.concatenate([[0, 0, 0], rng.integers(0, 300, 700), [0] * 9, rng.integers(0, 8, 300), [1, 0, 2, 0, 0]]).astype(np.int32)
    xyz = _walks(rng, lengths, shape)
    x, n = _to_dev(dev, xyz, lengths)
    _check_density(fj, x, n, shape, "random")
    _check_sample_and_stats(fj, x, n, shape, (0.5, 2.0, 1.0), rng, "random", frames=(1, 3, 7))


def test_one_line_of_100000_points(fj, dev):
    """the slow path of mode 1 (a bitmap over the voxels the line spans), alone and between short lines; 30^3 voxels, so the line
    visits most voxels many times"""
    rng = np.random.default_rng(12)
    shape = (30, 30, 30)
    long_line = _walks(rng, [100000], shape, step=0.5, wild=0.0005)
    x, n = _to_dev(dev, long_line, [100000])
    maps = _check_density(fj, x, n, shape, "long")
    assert maps["lines"].max() == 1 and maps["lines"].sum() > 1000
    _check_sample_and_stats(fj, x, n, shape, (1.0, 1.0, 1.0), rng, "long", frames=(1,))
    lengths = np.concatenate([rng.integers(0, 260, 40), [100000], rng.integers(0, 260, 40), [257, 256, 255, 0]]).astype(np.int32)
    xyz = np.concatenate([_walks(rng, lengths[:40], shape), long_line, _walks(rng, lengths[41:], shape)])
    x, n = _to_dev(dev, xyz, lengths)
    _check_density(fj, x, n, shape, "long between short")
    _check_sample_and_stats(fj, x, n, shape, (1.0, 0.5, 1.0), rng, "long between short", frames=(3,))


def test_tie_and_outside_witnesses_on_the_device(fj, dev):
    xyz, want = witnesses()
    x, n = _to_dev(dev, xyz, [len(xyz)])
    maps = _check_density(fj, x, n, WSHAPE, "witnesses")
    ref = np.bincount(want[want >= 0], minlength=maps["points"].size)
    assert np.array_equal(maps["points"], ref)                               # the hand-counted voxels, not only the restatement
    _check_sample_and_stats(fj, x, n, WSHAPE, (1.0, 1.0, 1.0), np.random.default_rng(1), "witnesses", frames=(1, 3, 7))
    # each witness as a line of its own
    x, n = _to_dev(dev, xyz, [1] * len(xyz))
    maps = _check_density(fj, x, n, WSHAPE, "witness lines")
    assert np.array_equal(maps["endpoints"], 2 * ref)


def test_views_side_stream_and_no_lines(fj, dev):
    import torch
    rng = np.random.default_rng(13)
    shape = (12, 12, 12)
    lengths = rng.integers(0, 120, 500).astype(np.int32)
    xyz = _walks(rng, lengths, shape)
    side = torch.cuda.Stream(device=dev)
    for shift in (1, 3):                                                      # 4 and 12 bytes off a 16-byte boundary
        base = torch.zeros(xyz.size + 8, dtype=torch.float32, device=dev)
        assert base.data_ptr() % 16 == 0
        view = base[shift:shift + xyz.size].view(-1, 3)
        view.copy_(torch.from_numpy(xyz).to(dev))
        assert view.data_ptr() % 16 == 4 * shift
        n = torch.from_numpy(lengths).to(dev)
        _check_density(fj, view, n, shape, "shift %d" % shift)
        _check_sample_and_stats(fj, view, n, shape, (1.0, 1.0, 1.0), rng, "shift %d" % shift)
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            d, nout = fj.str_density_device(view, n, shape, "lines", stream=side)
            s = fj.str_sample_device(view, torch.ones(12 ** 3, device=dev), shape, outside=-1.0, stream=side)
            p = fj.str_stats_device(view, n, (1.0, 1.0, 1.0), s, stream=side)
        side.synchronize()
        ref, rout = tm.density(xyz, lengths, shape, tm.LINES)
        assert np.array_equal(_np(d), ref) and int(nout.item()) == rout
        assert np.array_equal(_np(s), tm.sample(xyz, np.ones((1, 12 ** 3), np.float32), shape, outside=-1.0))
        rp, rb = tm.stats(xyz, lengths, (1, 1, 1), _np(s))
        assert tm.stats_close(_np(p), rp, rb).all()
    # no lines / no points: the map is still zero-filled, n_outside 0; lines that are all empty
    e = torch.zeros((0, 3), dtype=torch.float32, device=dev)
    for npts in (torch.zeros(0, dtype=torch.int32, device=dev), torch.zeros(5, dtype=torch.int32, device=dev)):
        for name, code in MODES:
            junk = torch.full((12 ** 3,), 7, dtype=torch.int32, device=dev).view(torch.uint32)
            d, nout = fj.str_density_device(e, npts, shape, name)
            assert int(_np(d).sum()) == 0 and int(nout.item()) == 0
            L = fj.lib()
            work = torch.empty(fj.str_work_size(npts.numel()) // 8 + 1, dtype=torch.int64, device=dev)
            no = torch.full((1,), 99, dtype=torch.int64, device=dev)
            assert L.fibd_str_density(None, npts.data_ptr() if npts.numel() else None, npts.numel(), 0, 12, 12, 12, code,
                                      junk.data_ptr(), no.data_ptr(), work.data_ptr(), work.numel() * 8, None) == 0
            torch.cuda.synchronize()
            assert int(_np(junk).sum()) == 0 and int(no.item()) == 0
        assert fj.str_sample_device(e, torch.ones(12 ** 3, device=dev), shape).shape == (0, 1)
        p = fj.str_stats_device(e, npts, (1, 1, 1))
        assert p.shape == (npts.numel(), 1) and (_np(p) == 0).all()


def test_accumulate_and_repeatability(fj, dev):
    rng = np.random.default_rng(14)
    shape = (16, 16, 10)
    lengths = rng.integers(0, 200, 2000).astype(np.int32)
    xyz = _walks(rng, lengths, shape)
    x, n = _to_dev(dev, xyz, lengths)
    half = 1000
    ph = int(lengths[:half].sum())
    for name, code in MODES:
        whole, wout = fj.str_density_device(x, n, shape, name)
        again, _ = fj.str_density_device(x, n, shape, name)
        assert np.array_equal(_np(whole).view(np.uint8), _np(again).view(np.uint8))               # identical bytes
        a, ao = fj.str_density_device(x[:ph], n[:half], shape, name)
        ao = int(ao.item())
        b, bo = fj.str_density_device(x[ph:], n[half:], shape, name, out=a)
        assert b.data_ptr() == a.data_ptr() and np.array_equal(_np(b), _np(whole)) and ao + int(bo.item()) == int(wout.item())
        # the other order of the batches
        c, _ = fj.str_density_device(x[ph:], n[half:], shape, name)
        c, _ = fj.str_density_device(x[:ph], n[:half], shape, name, out=c)
        assert np.array_equal(_np(c).view(np.uint8), _np(whole).view(np.uint8))
        assert np.array_equal(_np(whole), tm.density(xyz, lengths, shape, code)[0])


def test_invalid_counts_are_refused(fj, dev):
    import torch
    rng = np.random.default_rng(15)
    shape = (10, 10, 10)
    lengths = rng.integers(1, 50, 3000).astype(np.int32)
    xyz = _walks(rng, lengths, shape)
    x, _ = _to_dev(dev, xyz, lengths)
    short = lengths.copy(); short[1500] -= 1                                  # sum != npoints
    neg = lengths.copy(); neg[2999] = -3; neg[0] += 3                          # a negative count, the sum still right
    L = fj.lib()
    for bad in (short, neg):
        n = torch.from_numpy(bad).to(dev)
        for name, code in MODES:
            d, nout = fj.str_density_device(x, n, shape, name)
            assert int(nout.item()) == -1 and int(_np(d).sum()) == 0                               # zero-filled, nothing counted
            keep = torch.from_numpy(rng.integers(0, 2 ** 31, 1000).astype(np.int32)).to(dev).view(torch.uint32)
            before = _np(keep).copy()
            d, nout = fj.str_density_device(x, n, shape, name, out=keep)
            assert int(nout.item()) == -1 and np.array_equal(_np(keep), before)                    # ACCUMULATE: D keeps its bytes
            # host form: FIB_ERR_INVALID, outputs untouched
            hd = before.copy()
            ho = C.c_int64(77)
            assert L.fib_str_density(0, xyz.ctypes.data, bad.ctypes.data, bad.size, xyz.shape[0], 10, 10, 10, code, hd.ctypes.data, C.byref(ho)) == FIB_ERR_INVALID
            assert np.array_equal(hd, before) and ho.value == 77
        p = torch.full((bad.size, 1), 5.0, device=dev)
        fj.str_stats_device(x, n, (1, 1, 1), out=p)
        assert (_np(p) == 5.0).all()                                                               # no row is written
        hp = np.full((bad.size, 1), 5.0, np.float32)
        res = (C.c_float * 3)(1, 1, 1)
        assert L.fib_str_stats(0, xyz.ctypes.data, bad.ctypes.data, bad.size, xyz.shape[0], res, None, 0, hp.ctypes.data) == FIB_ERR_INVALID
        assert (hp == 5.0).all()
    n = torch.from_numpy(lengths).to(dev)
    work = torch.empty(fj.str_work_size(lengths.size) // 8 + 1, dtype=torch.int64, device=dev)
    d = torch.zeros(1000, dtype=torch.int32, device=dev)
    no = torch.zeros(1, dtype=torch.int64, device=dev)
    args = (x.data_ptr(), n.data_ptr(), lengths.size, xyz.shape[0], 10, 10, 10)
    assert L.fibd_str_density(*args, 3, d.data_ptr(), no.data_ptr(), work.data_ptr(), work.numel() * 8, None) == FIB_ERR_INVALID      # mode
    assert L.fibd_str_density(*args, 1, d.data_ptr(), no.data_ptr(), work.data_ptr(), 64, None) == FIB_ERR_INVALID                    # work too small
    assert L.fibd_str_density(x.data_ptr(), n.data_ptr(), lengths.size, xyz.shape[0], 10, 0, 10, 1, d.data_ptr(), no.data_ptr(), work.data_ptr(),
                              work.numel() * 8, None) == FIB_ERR_INVALID
    assert L.fibd_str_sample(x.data_ptr(), xyz.shape[0], d.data_ptr(), 10, 10, 10, 0, 0.0, d.data_ptr(), None) == FIB_ERR_INVALID
    torch.cuda.synchronize()


def test_host_forms_equal_the_device_forms(fj, dev):
    rng = np.random.default_rng(16)
    shape = (20, 18, 16)
    nvox = 20 * 18 * 16
    lengths = np.concatenate([[0], rng.integers(0, 400, 1500), [0, 0]]).astype(np.int32)
    xyz = _walks(rng, lengths, shape)
    x, n = _to_dev(dev, xyz, lengths)
    L = fj.lib()
    res = (C.c_float * 3)(0.7, 1.1, 2.0)
    for name, code in MODES:
        d, nout = fj.str_density_device(x, n, shape, name)
        hd = np.full(nvox, 9, np.uint32)
        ho = C.c_int64(-5)
        assert L.fib_str_density(0, xyz.ctypes.data, lengths.ctypes.data, lengths.size, xyz.shape[0], 20, 18, 16, code, hd.ctypes.data, C.byref(ho)) == 0
        assert np.array_equal(hd, _np(d)) and ho.value == int(nout.item())
        assert L.fib_str_density(0, xyz.ctypes.data, lengths.ctypes.data, lengths.size, xyz.shape[0], 20, 18, 16, code | ACC, hd.ctypes.data, C.byref(ho)) == 0
        assert np.array_equal(hd, 2 * _np(d)) and ho.value == int(nout.item())
        assert L.fib_str_density(-1, xyz.ctypes.data, lengths.ctypes.data, lengths.size, xyz.shape[0], 20, 18, 16, code, hd.ctypes.data,
                                 C.byref(ho)) == FIB_ERR_UNSUPPORTED
    import torch
    vol = rng.standard_normal((3, nvox)).astype(np.float32)
    s = fj.str_sample_device(x, torch.from_numpy(vol).to(dev), shape, outside=2.5)
    hs = np.zeros((xyz.shape[0], 3), np.float32)
    assert L.fib_str_sample(0, xyz.ctypes.data, xyz.shape[0], vol.ctypes.data, 20, 18, 16, 3, 2.5, hs.ctypes.data) == 0
    assert np.array_equal(hs, _np(s)) and np.array_equal(hs, tm.sample(xyz, vol, shape, 2.5))
    assert L.fib_str_sample(-1, xyz.ctypes.data, xyz.shape[0], vol.ctypes.data, 20, 18, 16, 3, 2.5, hs.ctypes.data) == FIB_ERR_UNSUPPORTED
    p = fj.str_stats_device(x, n, (0.7, 1.1, 2.0), s)
    hp = np.zeros((lengths.size, 4), np.float32)
    assert L.fib_str_stats(0, xyz.ctypes.data, lengths.ctypes.data, lengths.size, xyz.shape[0], res, hs.ctypes.data, 3, hp.ctypes.data) == 0
    assert np.array_equal(hp, _np(p), equal_nan=True)                          # the same kernel on the same lines: the same sums
    rp, rb = tm.stats(xyz, lengths, (0.7, 1.1, 2.0), hs)
    assert tm.stats_close(hp, rp, rb).all()
    assert L.fib_str_stats(-1, xyz.ctypes.data, lengths.ctypes.data, lengths.size, xyz.shape[0], res, hs.ctypes.data, 3, hp.ctypes.data) == FIB_ERR_UNSUPPORTED
    fj.trim()                                                                  # gives the workers' buffers back; the next call re-allocates
    ho = C.c_int64(0)
    hd = np.zeros(nvox, np.uint32)
    assert L.fib_str_density(0, xyz.ctypes.data, lengths.ctypes.data, lengths.size, xyz.shape[0], 20, 18, 16, 1, hd.ctypes.data, C.byref(ho)) == 0
    assert np.array_equal(hd, tm.density(xyz, lengths, shape, tm.LINES)[0])
    fj.trim()


def test_host_form_cuts_chunks_at_line_boundaries(fj):
    """more points than one chunk of the host form (2^22) holds, with a line longer than a chunk among them"""
    rng = np.random.default_rng(17)
    shape = (24, 24, 24)
    lengths = np.concatenate([rng.integers(0, 3000, 2500), [5_000_000], rng.integers(0, 3000, 500)]).astype(np.int32)
    npnt = int(lengths.sum())
    xyz = (rng.random((npnt, 3), dtype=np.float32) * 26.0).astype(np.float32)
    L = fj.lib()
    for _, code in MODES:
        hd = np.zeros(24 ** 3, np.uint32)
        ho = C.c_int64(0)
        assert L.fib_str_density(0, xyz.ctypes.data, lengths.ctypes.data, lengths.size, npnt, 24, 24, 24, code, hd.ctypes.data, C.byref(ho)) == 0
        ref, rout = tm.density(xyz, lengths, shape, code)
        assert np.array_equal(hd, ref) and ho.value == rout
    res = (C.c_float * 3)(1, 1, 1)
    sc = rng.standard_normal((npnt, 1)).astype(np.float32)
    hp = np.zeros((lengths.size, 2), np.float32)
    assert L.fib_str_stats(0, xyz.ctypes.data, lengths.ctypes.data, lengths.size, npnt, res, sc.ctypes.data, 1, hp.ctypes.data) == 0
    rp, rb = tm.stats(xyz, lengths, (1, 1, 1), sc)
    assert tm.stats_close(hp, rp, rb).all()
    fj.trim()


def test_python_layer_end_to_end(fj, tmp_path):
    from fibers_jl_amd import phantom
    shape = (14, 14, 14)
    ov = np.asfortranarray(phantom.fibre_field(*shape).astype(np.float32))
    rng = np.random.default_rng(18)
    fa = fj.MRI(rng.random(shape, dtype=np.float32), volres=(2.0, 2.0, 2.5))
    md = fj.MRI(rng.random(shape + (2,), dtype=np.float32), volres=(2.0, 2.0, 2.5))
    tr = fj.stream(fj.MRI(ov, volres=(2.0, 2.0, 2.5)), mask=fj.MRI(np.ones(shape, np.uint8)), sublist=np.array([[0.1, -0.2, 0.3]], np.float32))
    assert tr.nstr > 1000 and tuple(tr.volsize) == shape
    ts = fj.str_sample(tr, fa)
    assert ts.scalars.shape == (tr.xyz.shape[0], 1) and tr.scalars is None
    assert np.array_equal(ts.scalars, tm.sample(tr.xyz, fa.vol.reshape(-1, order="F")[None], shape))
    tp = fj.str_stats(ts)
    assert tp.properties.shape == (tr.nstr, 2)
    rp, rb = tm.stats(tr.xyz, tr.npts, tr.volres, ts.scalars)
    assert tm.stats_close(tp.properties, rp, rb).all()
    out = str(tmp_path / "maps.trk")
    assert not fj.trk_write(tp, out)
    back = fj.trk_read(out)
    assert back.n_scalars == 1 and back.n_properties == 2
    assert np.array_equal(np.asarray(back.scalars).reshape(-1, 1), ts.scalars) and np.array_equal(np.asarray(back.properties).reshape(-1, 2), tp.properties)
    # columns are appended: a list of volumes, after the column that is there
    t3 = fj.str_sample(ts, [fa, md], outside=np.nan)
    assert t3.scalars.shape[1] == 4 and np.array_equal(t3.scalars[:, 0], ts.scalars[:, 0]) and np.array_equal(t3.scalars[:, 1], ts.scalars[:, 0])
    planar = np.concatenate([fa.vol, md.vol], axis=3).reshape(-1, 3, order="F").T
    assert np.array_equal(t3.scalars[:, 1:], tm.sample(tr.xyz, planar, shape, np.nan), equal_nan=True)
    t4 = fj.str_stats(fj.str_stats(t3))
    assert t4.properties.shape == (tr.nstr, 10) and np.array_equal(t4.properties[:, :5], t4.properties[:, 5:], equal_nan=True)
    # density -> NIfTI -> density
    for name, code in MODES:
        d = fj.str_density(tr, name)
        ref, rout = tm.density(tr.xyz, tr.npts, shape, code)
        assert d.vol.dtype == np.uint32 and d.vol.shape == shape + (1,) and tuple(d.volres) == tuple(tr.volres) and d.n_outside == rout
        assert np.array_equal(d.vol.reshape(-1, order="F"), ref)
        f = str(tmp_path / ("density_%s.nii.gz" % name))
        assert not fj.mri_write(d, f)
        rd = fj.mri_read(f)
        assert rd.vol.dtype == np.uint32 and np.array_equal(rd.vol.reshape(shape + (-1,), order="F"), d.vol)
        d2 = fj.str_density(tr, name, out=d)
        assert d2 is d and np.array_equal(d.vol.reshape(-1, order="F"), 2 * ref) and d.n_outside == 2 * rout
    big = fj.str_density(tr, "points", shape=(20, 20, 3))
    assert big.vol.shape == (20, 20, 3, 1) and big.n_outside == tm.density(tr.xyz, tr.npts, (20, 20, 3), tm.POINTS)[1] > 0
    with pytest.raises(ValueError):
        fj.str_density(tr, "visits")


# ---- full size, once ---------------------------------------------------------------------------------------------------------------
def test_c4_lines_full_size(fj, dev):
    """C4's lines as tests/test_gpu_fullsize.py makes them (140^3, ~1 M seeds, ~129 M points): mode 0 against np.bincount over ALL points;
    mode 1 against the restatement on a seeded subset of 100 000 lines traced again into a map of their own; the identities on the whole set"""
    import torch
    from fibers_jl_amd import phantom
    shape = (140, 140, 140)
    nvox = 140 ** 3
    bval, bvec = phantom.scheme_dti(60, 4, 1000.0, seed=2)
    dwi, _ = phantom.make_dwi_torch(shape, bval, bvec, seed=2, device=dev, nfib=1)
    ones = torch.ones(nvox, dtype=torch.uint8, device=dev)
    o = fj.dti_fit_device(fj.DtiPlan(bval, bvec, device=0), dwi, ones)
    del dwi
    bm = phantom.ball_mask_torch(shape, dev)
    field, mout = fj.stream_field_device([o["eigvec1"]], fa=o["fa"], fa_thresh=0.1, mask=bm)
    seeds = torch.nonzero(mout).flatten()
    sub = torch.tensor([[0.1, -0.2, 0.3]], dtype=torch.float32, device=dev)
    r = fj.stream_device_run(field, shape, seeds, sub, buffers=fj.StreamBuffers(dev))
    xyz, npts = r["xyz"], r["npts"]
    nl, npnt = npts.numel(), xyz.shape[0]
    assert nl > 9.0e5 and npnt > 1.0e8
    maps, outs = {}, {}
    for name, _ in MODES:
        d, nout = fj.str_density_device(xyz, npts, shape, name)
        maps[name], outs[name] = _np(d), int(nout.item())
    hx = _np(xyz)
    lin = tm.voxel(hx, shape)
    assert (lin >= 0).all() and outs["points"] == 0 and outs["lines"] == 0 and outs["endpoints"] == 0      # the tracer stays inside
    assert np.array_equal(maps["points"], np.bincount(lin, minlength=nvox).astype(np.uint32))
    assert int(maps["points"].sum(dtype=np.int64)) == npnt and int(maps["endpoints"].sum(dtype=np.int64)) == 2 * nl
    assert (maps["lines"] <= maps["points"]).all() and (maps["lines"] <= nl).all()
    assert np.array_equal(maps["lines"] > 0, maps["points"] > 0)
    hn = _np(npts)
    off = np.concatenate([[0], np.cumsum(hn.astype(np.int64))])
    assert np.array_equal(maps["endpoints"], np.bincount(np.concatenate([lin[off[:-1]], lin[off[1:] - 1]]), minlength=nvox).astype(np.uint32))
    # a seeded subset of 100 000 lines, traced again, into a map of its own
    pick = np.sort(np.random.default_rng(19).choice(int(seeds.numel()), 100000, replace=False))
    rs = fj.stream_device_run(field, shape, seeds[torch.from_numpy(pick).to(dev)], sub, buffers=fj.StreamBuffers(dev))
    d, nout = fj.str_density_device(rs["xyz"], rs["npts"], shape, "lines")
    ref, rout = tm.density(_np(rs["xyz"]), _np(rs["npts"]), shape, tm.LINES)
    assert rs["npts"].numel() > 90000 and np.array_equal(_np(d), ref) and int(nout.item()) == rout
    # the sample of one map along all points, and the statistics of a seeded subset of lines
    s = fj.str_sample_device(xyz, o["fa"], shape)
    fa = _np(o["fa"]).reshape(-1)
    assert np.array_equal(_np(s)[:, 0], fa[lin])
    ss = fj.str_sample_device(rs["xyz"], o["fa"], shape)
    p = fj.str_stats_device(rs["xyz"], rs["npts"], (1.25, 1.25, 1.25), ss)
    rp, rb = tm.stats(_np(rs["xyz"]), _np(rs["npts"]), (1.25, 1.25, 1.25), _np(ss))
    assert tm.stats_close(_np(p), rp, rb).all()
