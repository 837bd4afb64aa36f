"""The exclusive scan over packed lines (csrc/line_scan.inc) at its own boundaries, through the public device-tier entries of its three
users: the offset scan of the tract maps and of the selection (1 sum per line), the gather (3 sums), prob_stream (2 sums).  A workgroup
takes 1024 lines; the totals kernel gives each of its 256 lanes ceil(blocks / 256) block totals, so more than 262 144 lines make a lane
walk several of them (263 169 lines: 258 blocks, 2 per lane; 525 315 lines: 514 blocks, 3 per lane, lane 171 gets one, the rest none).
Everything is compared BIT FOR BIT with the NumPy restatements (tractmap_ref, tractsel_ref, probtrack_ref); nothing reads the work area."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import probtrack_ref as pr  # noqa: E402
import tractmap_ref as tm  # noqa: E402
import tractsel_ref as ts  # noqa: E402
from test_gpu_probtrack import SHAPE as PROB_SHAPE, _sublist, lattice_case  # noqa: E402

pytestmark = pytest.mark.gpu
FIB_ERR_CAPACITY = -9
SIZES = (0, 1, 1023, 1024, 1025, 4097, 263169, 525315)
BIG = 525315
SHAPE = (7, 6, 5)
NVOX = 7 * 6 * 5
SENTINEL = 0x5A5A5A5A
MODES = (("points", tm.POINTS), ("lines", tm.LINES), ("endpoints", tm.ENDPOINTS))


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def _np(t):
    return t.cpu().numpy()


def _t(dev, a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).to(dev)                    # (a copy: the shared inputs are read-only)


def _u32(dev, a):
    import torch
    return _t(dev, np.asarray(a, np.uint32).view(np.int32)).view(torch.uint32)


@functools.lru_cache(maxsize=None)
def lines(n):
    """n lines of 0 to 5 points (under a million points at the largest n), the lines at the workgroup's edges set by hand with an empty
    one at 1024; points uniform in [0, shape + 1), so that some are outside; a 60 % keep"""
    rng = np.random.default_rng(1000 + n)
    npts = rng.choice(np.array([0, 0, 1, 2, 3, 5], np.int32), n)
    for at, c in ((n - 1, 2), (0, 3), (1023, 5), (1024, 0)):
        if 0 <= at < n:
            npts[at] = c
    xyz = (rng.random((int(npts.sum()), 3), dtype=np.float32) * (np.array(SHAPE, np.float32) + 1.0)).astype(np.float32)
    keep = (rng.random(n) < 0.6).astype(np.uint8)
    for a in (npts, xyz, keep):
        a.setflags(write=False)
    return xyz, npts, keep


# ---- offsets: one sum per line -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_offsets_through_the_density_maps(fj, dev, n):
    xyz, npts, _ = lines(n)
    x, c = _t(dev, xyz), _t(dev, npts)
    assert n < 1025 or (npts[1024] == 0 and npts[1023] == 5)
    for name, code in MODES:
        d, nout = fj.str_density_device(x, c, SHAPE, name)
        ref, rout = tm.density(xyz, npts, SHAPE, code)
        assert np.array_equal(_np(d), ref) and int(nout.item()) == rout, name
        assert n < 1023 or (rout > 0 and ref.any())


@pytest.mark.parametrize("n", (1025, BIG))
def test_offsets_through_the_selection(fj, dev, n):
    """hits is per line: one wrong offset anywhere shows"""
    xyz, npts, _ = lines(n)
    rois = np.random.default_rng(5).choice(np.array([0, 1], np.uint8), (5, NVOX))
    bits = ts.roi_pack(rois)
    kw = dict(visit_all=1, min_npts=1)
    rkeep, rhits, rcounts = ts.select(xyz, npts, SHAPE, bits, **kw)
    assert 0 < rcounts[0] < n
    keep, hits, counts = fj.str_select_device(_t(dev, xyz), _t(dev, npts), SHAPE, _u32(dev, bits), **kw)
    assert np.array_equal(_np(keep), rkeep) and np.array_equal(_np(hits), rhits) and [int(v) for v in _np(counts)] == rcounts


# ---- gather: three sums per line ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def gather_ref(n):
    """the restatement's gather of lines(n) with its random keep"""
    return ts.gather(*lines(n))


def _check_gather(fj, dev, xyz, npts, keep, sc=None, ref=None):
    g = fj.str_gather_device(_t(dev, xyz), _t(dev, npts), _t(dev, keep), None if sc is None else _t(dev, sc))
    rx, rn, ri, rs = ref or ts.gather(xyz, npts, keep, sc)
    nk, npk, status = (int(v) for v in _np(g["counts"]))
    assert (nk, npk, status) == (rn.size, rx.shape[0], 0)
    assert np.array_equal(_np(g["xyz"])[:npk].view(np.uint32), rx.view(np.uint32))
    assert np.array_equal(_np(g["npts"])[:nk], rn) and np.array_equal(_np(g["index"])[:nk], ri)
    if sc is not None:
        assert np.array_equal(_np(g["scalars"])[:npk].view(np.uint32), rs.view(np.uint32))


@pytest.mark.parametrize("n", SIZES)
def test_gather_of_a_random_keep(fj, dev, n):
    _check_gather(fj, dev, *lines(n), ref=gather_ref(n))


def test_gather_of_all_of_none_and_with_scalars(fj, dev):
    xyz, npts, keep = lines(1025)
    _check_gather(fj, dev, xyz, npts, np.ones(1025, np.uint8))
    _check_gather(fj, dev, xyz, npts, np.zeros(1025, np.uint8))
    _check_gather(fj, dev, xyz, npts, keep, np.random.default_rng(6).standard_normal((xyz.shape[0], 2)).astype(np.float32))


def test_gather_refusals_at_three_blocks_per_lane(fj, dev):
    """a capacity one short, a negative count in a later lane's range of the totals kernel, npoints one too large: the counts say so
    and every output keeps its sentinel"""
    import torch
    xyz, npts, keep = lines(BIG)
    rx, rn, _, _ = gather_ref(BIG)
    nk, npk = rn.size, rx.shape[0]
    k = _t(dev, keep)

    def run(x, c, cl, cp):
        out = dict(xyz=torch.full((cp, 3), SENTINEL, dtype=torch.int32, device=dev).view(torch.float32),
                   npts=torch.full((cl,), SENTINEL, dtype=torch.int32, device=dev), index=torch.full((cl,), SENTINEL, dtype=torch.int64, device=dev),
                   counts=torch.full((3,), 99, dtype=torch.int64, device=dev))
        g = fj.str_gather_device(x, c, k, out=out)
        for name in ("xyz", "npts"):
            assert (_np(out[name]).view(np.uint32) == SENTINEL).all(), name
        assert (_np(out["index"]) == SENTINEL).all()
        return [int(v) for v in _np(g["counts"])]

    x, c = _t(dev, xyz), _t(dev, npts)
    assert run(x, c, nk - 1, npk) == [nk, npk, -1]
    assert run(x, c, nk, npk - 1) == [nk, npk, -1]
    neg = npts.copy()
    neg[0] += 1 + neg[300000]                                                  # (the sum stays right: the negative count alone is refused)
    neg[300000] = -1
    assert neg.sum() == xyz.shape[0] and 300000 // 1024 >= 3
    assert run(x, _t(dev, neg), BIG, xyz.shape[0])[:2] == [-1, -1]
    longer = torch.cat([x, torch.ones((1, 3), dtype=torch.float32, device=dev)])
    assert run(longer, c, BIG, xyz.shape[0] + 1)[:2] == [-1, -1]


# ---- prob_stream: two sums per line ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", (2, 92, 183))
def test_prob_stream_offsets(fj, dev, k):
    """960 seeds tiled k times, 3 offsets: 5 760, 264 960 and 527 040 lines (6, 259, 515 blocks); len_min drops a sixth of the lines
    that have points, so that the kept-line sum differs from the line number"""
    import torch
    U, thr, tab, _, _ = lattice_case()
    seeds, sub = np.tile(np.arange(960, dtype=np.int64), k), _sublist(3)
    nl = seeds.size * 3
    assert -(-nl // 1024) == {2: 6, 92: 259, 183: 515}[k]
    want = pr.trace(tab, U, thr, PROB_SHAPE, seeds, sub, 3, 4, 1.0, rng_seed=17)
    n = want["all_counts"].sum(axis=1)
    has, dropped = int((n > 0).sum()), int(((n > 0) & (n < 3)).sum())
    assert 0.10 * has <= dropped <= 0.30 * has and want["npts"].size == has - dropped
    plan = fj.ProbPlan(U, device=0, cosang_thresh=thr)
    dtab, dseeds, dsub = _t(dev, tab), _t(dev, seeds), _t(dev, sub)
    got = fj.probtrack.prob_stream_device(plan, dtab, PROB_SHAPE, dseeds, dsub, 3, 4, 1.0, rng_seed=17)
    assert np.array_equal(_np(got["npts"]), want["npts"]) and np.array_equal(_np(got["seed_index"]), want["seed_index"])
    assert _np(got["xyz"]).tobytes() == want["xyz"].tobytes() and np.array_equal(_np(got["all_counts"]), want["all_counts"])
    if k != 183:
        return
    # lines_cap one short: FIB_ERR_CAPACITY, the true totals, nothing written
    lines_want, points_want = want["npts"].size, want["xyz"].shape[0]
    wb = fj.prob_work_size(nl)
    work = torch.empty(wb // 8, dtype=torch.int64, device=dev)
    npts = torch.full((lines_want,), -7, dtype=torch.int32, device=dev)
    sidx = torch.full((lines_want,), -7, dtype=torch.int64, device=dev)
    xyz = torch.full((3 * points_want,), -7.0, dtype=torch.float32, device=dev)
    a, b = C.c_int64(0), C.c_int64(0)
    torch.cuda.synchronize()
    rc = fj.lib().fibd_prob_run(plan._h, *PROB_SHAPE, 3, 4, 1.0, dtab.data_ptr(), dseeds.data_ptr(), dseeds.numel(), dsub.data_ptr(), 3, 17,
                                npts.data_ptr(), sidx.data_ptr(), lines_want - 1, xyz.data_ptr(), points_want, C.byref(a), C.byref(b),
                                work.data_ptr(), wb, None)
    assert rc == FIB_ERR_CAPACITY and (a.value, b.value) == (lines_want, points_want)
    assert (_np(npts) == -7).all() and (_np(sidx) == -7).all() and (_np(xyz) == -7.0).all()
