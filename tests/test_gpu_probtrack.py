"""Probabilistic ODF tracking on the GPU (csrc/probtrack.hip through the C ABI and the Python layer) against the NumPy restatement of the
header's definition (tests/probtrack_ref.py, pinned by tests/test_probtrack_ref.py).  Every sum of the definition is an integer sum and
every float operation is rounded on its own, so the weight table, npts, seed_index and every coordinate are compared BIT FOR BIT.
Volumes are 12 x 10 x 8 with a ball mask of radius 5.5 (608 seeds); the ODFs are GQI reconstructions of the phantom."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import probtrack_ref as R  # noqa: E402
import tractmap_ref as tm  # noqa: E402

pytestmark = pytest.mark.gpu
FIB_ERR_INVALID, FIB_ERR_UNSUPPORTED, FIB_ERR_CAPACITY = -1, -7, -9
SHAPE = (12, 10, 8)
NVOX = 12 * 10 * 8
SPHERES = {"sphere_362": False, "sphere_642": True, "sphere_724": False}       # name -> crossing fibres in the phantom
PLANTED = (413, 546, 532, 427, 534)                                             # NaN, +Inf, -Inf, all negative, constant: inside the ball
F32 = np.float32


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def _t(dev, a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).to(dev)                    # (a copy: the shared references are read-only)


def _np(t):
    return t.cpu().numpy()


@pytest.fixture(scope="module")
def mask(fj):
    from fibers_jl_amd import phantom
    m = phantom.ball_mask(*SHAPE, radius=5.5).reshape(-1, order="F")
    assert int(m.sum()) == 608
    m.setflags(write=False)
    return m


@pytest.fixture(scope="module")
def odfs(fj):
    """name -> (U float32 [nvert, 3], odf float32 [nvert, nvox] planar with the planted voxels, the GQI result's MRI); computed once"""
    from fibers_jl_amd import phantom
    bval, bvec = phantom.scheme_gqi()
    out = {}
    for name, crossing in SPHERES.items():
        sph = getattr(fj, name)
        dwi, _, _ = phantom.make_volume(SHAPE, bval, bvec, seed=11, crossing=crossing)
        g = fj.gqi_rec(fj.MRI(dwi, bval, bvec), fj.MRI(np.ones(SHAPE, np.uint8)), sph)
        o = np.ascontiguousarray(g.odf.vol.reshape(NVOX, sph.nvert, order="F").T)
        o[3, PLANTED[0]] = np.nan
        o[7, PLANTED[1]] = np.inf
        o[0, PLANTED[2]] = -np.inf
        o[:, PLANTED[3]] = -np.abs(o[:, PLANTED[3]]) - 1
        o[:, PLANTED[4]] = 0.25
        g.odf.vol[...] = o.T.reshape(SHAPE + (sph.nvert,), order="F")
        o.setflags(write=False)
        out[name] = (np.ascontiguousarray(sph.vertices[: sph.nvert], F32), o, g.odf)
    return out


_tables = {}


def ref_table(odfs, mask, name, masked, subtract_min=True, pmf=0.1):
    key = (name, masked, subtract_min, pmf)
    if key not in _tables:
        t = R.table(odfs[name][1], mask if masked else None, subtract_min, pmf)
        t.setflags(write=False)
        _tables[key] = t
    return _tables[key]


# ---- table -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("name", sorted(SPHERES))
def test_table_is_bit_identical(fj, dev, odfs, mask, name, masked):
    import torch
    U, o, _ = odfs[name]
    nvert, pitch = U.shape[0], R.row_pitch(U.shape[0])
    assert fj.prob_row_pitch(nvert) == pitch
    want = ref_table(odfs, mask, name, masked)
    assert not want[list(PLANTED[1:3]) + [PLANTED[4]]].any() and want[PLANTED[0]].any() and want[PLANTED[3]].any()
    got = fj.probtrack.prob_table_device(_t(dev, o), _t(dev, mask) if masked else None)
    assert got.dtype == torch.uint16 and tuple(got.shape) == (NVOX, pitch)
    assert _np(got).tobytes() == want.tobytes()
    # a voxel count that is no multiple of the tile, no subtraction, another threshold, a sentinel behind the buffer
    n = NVOX - 13
    buf = torch.full((n * pitch + 256,), 0xA5A5, dtype=torch.uint16, device=dev)
    cut = _t(dev, o[:, :n])
    fj.probtrack.prob_table_device(cut, _t(dev, mask[:n]) if masked else None, subtract_min=False, pmf_thresh=0.5, out=buf[: n * pitch].view(n, pitch))
    want2 = R.table(o[:, :n], mask[:n] if masked else None, False, 0.5)
    b = _np(buf)
    assert b[: n * pitch].tobytes() == want2.tobytes() and (b[n * pitch:] == 0xA5A5).all()


def test_table_of_a_wide_direction_set(fj, dev):
    """more than 480 directions take the 16-voxel tile"""
    rng = np.random.default_rng(2)
    o = rng.standard_normal((500, 83)).astype(F32)
    o[:, 4] = np.nan
    o[17, 9] = np.inf
    got = fj.probtrack.prob_table_device(_t(dev, o))
    assert tuple(got.shape) == (83, 512) and _np(got).tobytes() == R.table(o).tobytes()
    with pytest.raises(ValueError):
        fj.prob_row_pitch(513)


# ---- lines -----------------------------------------------------------------------------------------------------------------------
def _seeds(mask, nseed):
    s = np.flatnonzero(mask).astype(np.int64)
    return s if nseed is None else s[:: max(1, len(s) // nseed)][:nseed] if nseed > 1 else s[300:301]


def _sublist(nsub):
    return np.random.default_rng(9).uniform(-0.49, 0.49, (nsub, 3)).astype(F32)


def _same_lines(got, want):
    assert np.array_equal(_np(got["npts"]), want["npts"]), "npts differ"
    assert np.array_equal(_np(got["seed_index"]), want["seed_index"]), "seed_index differs"
    assert _np(got["xyz"]).tobytes() == want["xyz"].tobytes(), "coordinates differ"
    assert np.array_equal(_np(got["all_counts"]), want["all_counts"]), "per-line counts differ"


CASES = [
    # name, nsub, step, ang, len_max, len_min, pmf, nseed (None: all 608)
    ("sphere_362", 3, 0.5, 45, 140, 3, 0.1, None),
    ("sphere_642", 1, 1.0, 20, 12, 1, 0.5, 257),
    ("sphere_724", 1, 0.5, 80, 2, 1, 0.1, 1),
    ("sphere_642", 3, 0.5, 45, 140, 14, 0.1, None),                           # (len_min 14 drops 558 of the 1783 lines that have points)
    ("sphere_362", 1, 1.0, 45, 12, 3, 0.5, 257),
    ("sphere_724", 3, 0.5, 20, 140, 3, 0.1, 257),
    ("sphere_642", 3, 1.0, 80, 12, 1, 0.1, 1),
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(x) for x in c))
def test_lines_are_bit_identical(fj, dev, odfs, mask, case):
    name, nsub, step, ang, len_max, len_min, pmf, nseed = case
    U = odfs[name][0]
    tab = ref_table(odfs, mask, name, True, True, pmf)
    seeds, sub = _seeds(mask, nseed), _sublist(nsub)
    assert len(seeds) == (608 if nseed is None else nseed)
    plan = fj.ProbPlan(getattr(fj, name), ang, 0)
    want = R.trace(tab, U, plan.cosang_thresh, SHAPE, seeds, sub, len_min, len_max, step, rng_seed=1234 + nsub)
    got = fj.probtrack.prob_stream_device(plan, _t(dev, tab), SHAPE, _t(dev, seeds), _t(dev, sub), len_min, len_max, step, rng_seed=1234 + nsub)
    _same_lines(got, want)
    assert want["all_counts"].sum(axis=1).max() <= len_max + 2
    if len_min == 14:
        assert 0 < want["npts"].size < 0.75 * (want["all_counts"].sum(axis=1) > 0).sum()     # len_min drops a good part of the lines
    if len_max == 2:
        assert want["npts"].max() == 4


def test_lines_from_the_faces_zero_rows_and_outside(fj, dev, odfs, mask):
    """seeds on the volume's faces (table without a mask), seeds whose row is zero, seeds outside the volume"""
    name = "sphere_362"
    U = odfs[name][0]
    tab = ref_table(odfs, mask, name, False)
    lin = np.arange(NVOX)
    x, y, z = lin % 12, (lin // 12) % 10, lin // 120
    face = (x == 0) | (x == 11) | (y == 0) | (y == 9) | (z == 0) | (z == 7)
    seeds = np.concatenate([lin[face][::3], np.array(PLANTED[1:3] + (NVOX, -1), np.int64)]).astype(np.int64)
    sub = _sublist(3)
    plan = fj.ProbPlan(getattr(fj, name), 45, 0)
    want = R.trace(tab, U, plan.cosang_thresh, SHAPE, seeds, sub, 1, 140, 0.5, rng_seed=2 ** 63 + 1)
    assert (want["all_counts"][-12:] == 0).all() and want["npts"].size > 100
    got = fj.probtrack.prob_stream_device(plan, _t(dev, tab), SHAPE, _t(dev, seeds), _t(dev, sub), 1, 140, 0.5, rng_seed=2 ** 63 + 1)
    _same_lines(got, want)


def lattice_case():
    """13 directions (the half of the 26-neighbourhood: pitch 64, half of a line's 16 lanes hold nothing), a random table with empty
    voxels, and a cosang_thresh that EQUALS c(j, i) of every (axis, face diagonal) pair, so that >= and > give other lines"""
    d = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, -1, 0), (1, 0, 1), (1, 0, -1), (0, 1, 1), (0, 1, -1), (1, 1, 1), (1, 1, -1), (1, -1, 1),
         (1, -1, -1)]
    U = np.array(d, np.float64)
    U = (U / np.linalg.norm(U, axis=1)[:, None]).astype(F32)
    thr = float((U[0, 0] * U[3, 0] + U[0, 1] * U[3, 1]) + U[0, 2] * U[3, 2])    # 1 * float32(1 / sqrt 2)
    rng = np.random.default_rng(8)
    tab = np.zeros((NVOX, 64), np.uint16)
    tab[:, :13] = np.floor(rng.random((NVOX, 13)) ** 4 * 65535)
    tab[rng.random(NVOX) < 0.1] = 0
    return U, thr, tab, np.arange(NVOX, dtype=np.int64), _sublist(2)


def test_a_threshold_on_a_dot_product_and_a_small_direction_set(fj, dev):
    U, thr, tab, seeds, sub = lattice_case()
    plan = fj.ProbPlan(U, device=0, cosang_thresh=thr)
    assert plan.pitch == 64 and plan.cosang_thresh == thr
    want = R.trace(tab, U, thr, SHAPE, seeds, sub, 2, 20, 1.0, rng_seed=17)
    strict = R.trace(tab, U, thr, SHAPE, seeds, sub, 2, 20, 1.0, rng_seed=17, mutant="allow_gt")
    assert want["npts"].size > 500 and strict["xyz"].tobytes() != want["xyz"].tobytes()      # (the case tells >= from >)
    got = fj.probtrack.prob_stream_device(plan, _t(dev, tab), SHAPE, _t(dev, seeds), _t(dev, sub), 2, 20, 1.0, rng_seed=17)
    _same_lines(got, want)


def test_streams_and_repeats_give_the_same_bytes(fj, dev, odfs, mask):
    import torch
    name = "sphere_642"
    tab = _t(dev, ref_table(odfs, mask, name, True))
    seeds, sub = _t(dev, _seeds(mask, None)), _t(dev, _sublist(3))
    plan = fj.ProbPlan(getattr(fj, name), 45, 0)
    torch.cuda.synchronize()
    outs = []
    for st in (None, torch.cuda.Stream(dev), torch.cuda.Stream(dev), None):
        r = fj.probtrack.prob_stream_device(plan, tab, SHAPE, seeds, sub, rng_seed=7, stream=st)
        outs.append((_np(r["npts"]).tobytes(), _np(r["seed_index"]).tobytes(), _np(r["xyz"]).tobytes()))
    assert all(o == outs[0] for o in outs[1:]) and len(outs[0][2]) > 0
    other = fj.probtrack.prob_stream_device(plan, tab, SHAPE, seeds, sub, rng_seed=8)
    assert _np(other["xyz"]).tobytes() != outs[0][2]


def test_capacities(fj, dev, odfs, mask):
    import torch
    name = "sphere_362"
    U = odfs[name][0]
    tabn = ref_table(odfs, mask, name, True)
    seedsn, subn = _seeds(mask, 257), _sublist(3)
    plan = fj.ProbPlan(getattr(fj, name), 45, 0)
    want = R.trace(tabn, U, plan.cosang_thresh, SHAPE, seedsn, subn, 3, 140, 0.5, rng_seed=3)
    nl, npnt = want["npts"].size, want["xyz"].shape[0]
    tab, seeds, sub = _t(dev, tabn), _t(dev, seedsn), _t(dev, subn)
    L = fj.lib()
    wb = fj.prob_work_size(seedsn.size * 3)
    work = torch.empty(wb // 8, dtype=torch.int64, device=dev)
    pad = 64

    def run(lcap, pcap):
        npts = torch.full((lcap + pad,), -7, dtype=torch.int32, device=dev)
        sidx = torch.full((lcap + pad,), -7, dtype=torch.int64, device=dev)
        xyz = torch.full((3 * (pcap + pad),), -7.0, dtype=torch.float32, device=dev)
        a, b = C.c_int64(0), C.c_int64(0)
        torch.cuda.synchronize()
        rc = L.fibd_prob_run(plan._h, *SHAPE, 3, 140, 0.5, tab.data_ptr(), seeds.data_ptr(), seeds.numel(), sub.data_ptr(), 3, 3,
                             npts.data_ptr(), sidx.data_ptr(), lcap, xyz.data_ptr(), pcap, C.byref(a), C.byref(b), work.data_ptr(), wb, None)
        return rc, a.value, b.value, _np(npts), _np(sidx), _np(xyz)

    for lcap, pcap in ((nl - 1, npnt), (nl, npnt - 1), (0, 0)):
        rc, a, b, npts, sidx, xyz = run(lcap, pcap)
        assert rc == FIB_ERR_CAPACITY and (a, b) == (nl, npnt)
        assert (npts == -7).all() and (sidx == -7).all() and (xyz == -7.0).all()           # nothing was written
    rc, a, b, npts, sidx, xyz = run(nl, npnt)                                              # the reported sizes
    assert rc == 0 and (a, b) == (nl, npnt)
    assert np.array_equal(npts[:nl], want["npts"]) and np.array_equal(sidx[:nl], want["seed_index"])
    assert xyz[: 3 * npnt].tobytes() == want["xyz"].tobytes()
    assert (npts[nl:] == -7).all() and (sidx[nl:] == -7).all() and (xyz[3 * npnt:] == -7.0).all()
    # the Python layer grows a caller's buffers by itself
    buf = fj.StreamBuffers(dev, 4, 4)
    r = fj.probtrack.prob_stream_device(plan, tab, SHAPE, seeds, sub, 3, 140, 0.5, rng_seed=3, buffers=buf)
    _same_lines(r, want)
    assert r["buffers"] is buf and buf.npts.numel() >= nl


def test_output_goes_through_the_tract_maps(fj, dev, odfs, mask):
    name = "sphere_642"
    U = odfs[name][0]
    tabn = ref_table(odfs, mask, name, True)
    seedsn, subn = _seeds(mask, None), _sublist(1)
    plan = fj.ProbPlan(getattr(fj, name), 45, 0)
    want = R.trace(tabn, U, plan.cosang_thresh, SHAPE, seedsn, subn, 3, 140, 0.5, rng_seed=21)
    r = fj.probtrack.prob_stream_device(plan, _t(dev, tabn), SHAPE, _t(dev, seedsn), _t(dev, subn), 3, 140, 0.5, rng_seed=21)
    for mode, code in (("points", tm.POINTS), ("lines", tm.LINES), ("endpoints", tm.ENDPOINTS)):
        d, nout = fj.str_density_device(r["xyz"], r["npts"], SHAPE, mode)
        dr, noutr = tm.density(want["xyz"], want["npts"], SHAPE, code)
        assert np.array_equal(_np(d), dr) and int(_np(nout)[0]) == noutr
    res = (1.25, 0.5, 2.0)
    p = fj.str_stats_device(r["xyz"], r["npts"], res)
    pr, bound = tm.stats(want["xyz"], want["npts"], res)
    assert tm.stats_close(_np(p), pr, bound).all()


# ---- host form ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sphere_642", "sphere_362"])
def test_host_form_equals_the_device_tier(fj, dev, odfs, mask, name):
    U, o, odf_mri = odfs[name]
    sub = _sublist(3)
    m = fj.MRI(np.asfortranarray(mask.reshape(SHAPE, order="F")))
    tr = fj.prob_stream(odf_mri, getattr(fj, name), mask=m, sublist=sub, len_min=3, ang_thresh=45, step_size=0.5, pmf_thresh=0.1, rng_seed=99)
    plan = fj.ProbPlan(getattr(fj, name), 45, 0)
    tab = fj.probtrack.prob_table_device(_t(dev, o), _t(dev, mask))
    r = fj.probtrack.prob_stream_device(plan, tab, SHAPE, _t(dev, _seeds(mask, None)), _t(dev, sub), 3, None, 0.5, rng_seed=99)
    assert np.array_equal(tr.npts, _np(r["npts"])) and np.array_equal(tr.seed_index, _np(r["seed_index"]))
    assert np.asarray(tr.xyz, F32).tobytes() == _np(r["xyz"]).tobytes() and tr.xyz.shape[0] > 1000
    want = R.trace(ref_table(odfs, mask, name, True), U, plan.cosang_thresh, SHAPE, _seeds(mask, None), sub, 3, 12, 0.5, rng_seed=99)
    assert np.asarray(tr.xyz, F32).tobytes() == want["xyz"].tobytes()
    # a seed volume, and a GQI-like container
    sv = np.zeros(SHAPE, np.uint8, order="F")
    sv[5:7, 4:6, 3:5] = 1

    class G:
        odf = odf_mri
    tr2 = fj.prob_stream(G(), getattr(fj, name), mask=m, seed=fj.MRI(sv), sublist=sub[:1], rng_seed=99)
    s2 = np.flatnonzero(sv.reshape(-1, order="F")).astype(np.int64)
    want2 = R.trace(ref_table(odfs, mask, name, True), U, plan.cosang_thresh, SHAPE, s2, sub[:1], 3, 12, 0.5, rng_seed=99)
    assert np.array_equal(tr2.npts, want2["npts"]) and np.asarray(tr2.xyz, F32).tobytes() == want2["xyz"].tobytes()


def test_refusals(fj, dev, odfs, mask):
    import torch
    from fibers_jl_amd._dev import ArgError
    name = "sphere_362"
    U, o, odf_mri = odfs[name]
    with pytest.raises(fj.FibersError) as e:
        fj.ProbPlan(getattr(fj, name), 90, 0)
    assert e.value.code == FIB_ERR_INVALID
    with pytest.raises(ValueError):
        fj.ProbPlan(np.zeros((513, 3), F32), 45, 0)
    h = C.c_void_p()
    assert fj.lib().fib_prob_plan_create(0, np.zeros((513, 3), F32).ctypes.data, 513, 0.7, C.byref(h)) == FIB_ERR_UNSUPPORTED
    with pytest.raises(fj.FibersError) as e:
        fj.prob_stream(odf_mri, getattr(fj, name), sublist=_sublist(1), device=fj.DEVICE_ALL)
    assert e.value.code == FIB_ERR_UNSUPPORTED
    plan = fj.ProbPlan(getattr(fj, name), 45, 0)
    tab = _t(dev, ref_table(odfs, mask, name, True))
    seeds, sub = _t(dev, _seeds(mask, 257)), _t(dev, _sublist(3))
    ok = fj.probtrack.prob_stream_device(plan, tab, SHAPE, seeds, sub)
    assert ok["npts"].numel() > 0
    bad = [
        dict(table=tab.view(torch.int16)),                                      # wrong dtype
        dict(table=tab.cpu()),                                                  # wrong device
        dict(table=tab[:-1]),                                                   # a short table
        dict(table=tab[:, :128].contiguous()),                                  # another pitch
        dict(seeds=seeds.to(torch.int32)),
        dict(table=torch.zeros(tuple(tab.shape) + (2,), dtype=torch.uint16, device=dev)[..., 0]),   # a strided view
        dict(seeds=torch.zeros((seeds.numel(), 2), dtype=torch.int64, device=dev)[:, 0]),
        dict(sublist=torch.zeros((3, 3, 2), dtype=torch.float32, device=dev)[..., 0]),
        dict(sublist=sub.reshape(-1)),
        dict(work=torch.empty(fj.prob_work_size(257 * 3) // 8 - 1, dtype=torch.int64, device=dev)),   # a short work
        dict(work=torch.empty(fj.prob_work_size(257 * 3) // 8, dtype=torch.int64)),
    ]
    for kw in bad:
        args = dict(table=tab, seeds=seeds, sublist=sub)
        work = kw.pop("work", None)
        args.update(kw)
        with pytest.raises(ArgError):
            fj.probtrack.prob_stream_device(plan, args["table"], SHAPE, args["seeds"], args["sublist"], work=work)
    with pytest.raises(ArgError):
        fj.probtrack.prob_table_device(_t(dev, o).double())
    with pytest.raises(ArgError):
        fj.probtrack.prob_table_device(_t(dev, o), _t(dev, mask)[:-1])
    with pytest.raises(ArgError):
        fj.probtrack.prob_table_device(_t(dev, o), out=torch.empty((NVOX, 64), dtype=torch.uint16, device=dev))


def test_host_form_walks_voxel_chunks(fj):
    """more than 2^18 voxels: the host form builds the table from two chunks of the planar host ODF; seeds on both sides of the cut"""
    shape = (70, 64, 60)
    nvox = 70 * 64 * 60
    assert nvox > 2 ** 18
    sph = fj.sphere_362
    U = np.ascontiguousarray(sph.vertices[:181], F32)
    rng = np.random.default_rng(3)
    o = (rng.random((181, nvox), dtype=F32) ** 4).astype(F32)
    sv = np.zeros(nvox, np.uint8)
    sv[2 ** 18 - 40: 2 ** 18 + 40: 3] = 1
    sub = _sublist(2)
    vol = o.T.reshape(shape + (181,), order="F")
    tr = fj.prob_stream(fj.MRI(vol), sph, seed=fj.MRI(np.asfortranarray(sv.reshape(shape, order="F"))), sublist=sub, len_max=30, ang_thresh=30,
                        pmf_thresh=0.3, rng_seed=5)
    want = R.trace(R.table(o, None, True, 0.3), U, fj.ProbPlan(sph, 30, 0).cosang_thresh, shape, np.flatnonzero(sv), sub, 3, 30, 0.5, rng_seed=5)
    assert want["npts"].size > 40 and want["npts"].max() == 32
    assert np.array_equal(tr.npts, want["npts"]) and np.array_equal(tr.seed_index, want["seed_index"])
    assert np.asarray(tr.xyz, F32).tobytes() == want["xyz"].tobytes()


# ---- the host form on its worker: the lock, an empty result, what stays on the device ------------------------------------------------
def _host_args(fj, odfs, mask, name="sphere_362", seed=None, **kw):
    return dict(dict(odf=odfs[name][2], odf_dirs=getattr(fj, name), mask=fj.MRI(np.asfortranarray(mask.reshape(SHAPE, order="F"))), seed=seed,
                     sublist=_sublist(2), len_min=3, ang_thresh=45, step_size=0.5, pmf_thresh=0.1, rng_seed=31), **kw)


def _host_bytes(fj, args):
    a = dict(args)
    tr = fj.prob_stream(a.pop("odf"), a.pop("odf_dirs"), **a)
    return tr.npts.tobytes(), tr.seed_index.tobytes(), np.asarray(tr.xyz, F32).tobytes()


def test_host_form_calls_from_three_threads_with_trim_between_them(fj, odfs, mask):
    """Three threads make the same prob_stream call on device 0 while a fourth calls trim() between its own short sleeps: every result
    is byte-equal to that of a single call made before.  (The worker's lock cannot be seen from outside; this is what a caller sees.)"""
    import threading
    import time
    args = _host_args(fj, odfs, mask)
    want = _host_bytes(fj, args)
    assert len(want[2]) > 12 * 1000
    got, errors, done = [None] * 3, [], threading.Event()

    def call(i):
        try:
            got[i] = [_host_bytes(fj, args) for _ in range(3)]
        except Exception as e:                                                 # noqa: BLE001
            errors.append(e)

    def trimmer():
        try:
            while not done.is_set():
                time.sleep(0.002)
                fj.trim()
        except Exception as e:                                                 # noqa: BLE001
            errors.append(e)

    th = [threading.Thread(target=call, args=(i,)) for i in range(3)]
    tt = threading.Thread(target=trimmer)
    tt.start()
    for t in th:
        t.start()
    for t in th:
        t.join()
    done.set()
    tt.join()
    assert not errors, errors
    assert all(r == want for rs in got for r in rs)


def test_host_form_without_a_seed_returns_empty_arrays(fj, odfs, mask):
    """an all-zero seed volume: nlines = npoints = 0, the three arrays are there all the same, fib_tract_free takes them"""
    from fibers_jl_amd import _lib
    name = "sphere_362"
    U, _, odf_mri = odfs[name]
    vol = np.asfortranarray(odf_mri.vol, dtype=F32)
    m8 = np.ascontiguousarray(mask, np.uint8)
    s8 = np.zeros(NVOX, np.uint8)
    sub = _sublist(2)
    out = _lib.TractOut()
    L = fj.lib()
    rc = L.fib_prob_stream(0, *SHAPE, vol.ctypes.data, U.shape[0], U.ctypes.data, m8.ctypes.data, s8.ctypes.data, sub.ctypes.data, 2, 3, 12,
                           float(np.cos(np.deg2rad(F32(45)))), 0.5, 0.1, 1, 31, C.byref(out))
    assert rc == 0, L.fib_last_error()
    assert out.nlines == 0 and out.npoints == 0
    assert out.npts and out.seed_index and out.xyz and not out.flags
    L.fib_tract_free(C.byref(out))
    assert not out.npts and not out.seed_index and not out.xyz and not out.flags and out.nlines == 0 and out.npoints == 0
    tr = fj.prob_stream(odf_mri, getattr(fj, name), mask=fj.MRI(np.asfortranarray(mask.reshape(SHAPE, order="F"))),
                        seed=fj.MRI(np.zeros(SHAPE, np.uint8, order="F")), sublist=sub)
    assert tr.npts.size == 0 and tr.seed_index.size == 0 and tr.xyz.shape == (0, 3)


def test_host_form_keeps_no_device_memory_past_trim(fj, odfs, mask):
    """after a warm-up call and trim(), a call and trim() leave the free device memory where it was: the table, the result buffers and
    the output ring's mirror all go back"""
    import torch
    args = _host_args(fj, odfs, mask)
    _host_bytes(fj, args)
    fj.trim()
    torch.cuda.synchronize()
    before = torch.cuda.mem_get_info()[0]
    _host_bytes(fj, args)
    fj.trim()
    torch.cuda.synchronize()
    after = torch.cuda.mem_get_info()[0]
    print("free device memory before / after: %d / %d" % (before, after))
    assert after == before
