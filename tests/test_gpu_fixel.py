"""Tractogram weights on the GPU (csrc/fixel.hip through the C ABI: fibd_fixel_* / fibd_str_weights on device tensors, fib_str_weights on
host arrays with the points forced into several chunks, and `str_weights` on top) against the NumPy restatement of the header's
definitions (tests/fixel_ref.py, pinned by tests/test_fixel_ref.py).  Every sum that decides a weight is an integer sum, so fixel ids,
q, weights, td, mu and all counts are compared BIT FOR BIT.  cost is a float64 sum whose order is free: it is held to
n * 2^-53 * sum|t| around the exact sum of its terms (math.fsum in the restatement), the bound the header states.

Shapes: a 6 x 5 x 4 volume with nvec 1, 2 and 3; about 150 lines of 0 to 70 points and one line of 300.  One world of 48 x 40 x 24
voxels with nvec 3 takes fx_cost past two rounds of its fixed grid."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fixel_ref as fx  # noqa: E402
from test_fixel_ref import Field, pack, rules_case  # noqa: E402

pytestmark = pytest.mark.gpu
SHAPE = (6, 5, 4)
NVOX = 120
F_THRESH = 0.03
FIB_ERR_INVALID = -1


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def _world(nvec):
    """a peak field with every kind of fixel that does not exist, and lines with every kind of point that is not assigned"""
    rng = np.random.default_rng(40 + nvec)
    fld = Field(SHAPE, nvec)
    for k in range(nvec):
        u = 0.35 * rng.standard_normal((3, NVOX))                                       # peak k lies near axis k
        u[k] += 1
        fld.ovec[k][:] = (u / np.linalg.norm(u, axis=0)).astype(np.float32)
        fld.f[k][:] = (0.02 + 0.6 * rng.random(NVOX) / (k + 1)).astype(np.float32)      # some at or below the threshold
    hub = fld.lin((3, 3, 2))
    fld.ovec[0][:, hub] = (1, 0, 0)
    fld.f[0][hub] = 0.5                                                                # the fixel every hub line crosses
    fld.f[0][fld.lin((1, 1, 1))] = np.float32(F_THRESH)                                # f == f_thresh: no fixel
    fld.f[0][fld.lin((2, 1, 1))] = np.nan
    fld.f[0][fld.lin((3, 1, 1))] = np.inf
    fld.ovec[0][:, fld.lin((4, 1, 1))] = 0                                             # a zero peak vector
    fld.ovec[0][1, fld.lin((5, 1, 1))] = np.inf
    fld.ovec[nvec - 1][2, fld.lin((6, 1, 1))] = np.nan
    mask = np.ones(NVOX, np.uint8)
    mask[fld.lin((2, 2, 2))] = 0                                                       # a masked-out voxel
    mask[rng.integers(0, NVOX, 6)] = 0
    lines = [[], [(3, 3, 2)], [(2.6, 3, 2), (3.4, 3, 2)]]                              # npts 0, 1 and 2
    for _ in range(120):                                                               # walks of uniform step, some leaving the volume
        n = int(rng.integers(0, 71))
        step = float(rng.choice([0.05, 0.25, 0.5, 1.0]))                               # 0.05: runs of 20 points per voxel, across rounds of 16
        p = np.array([1, 1, 1]) + rng.random(3) * (np.array(SHAPE) - 1)
        d = rng.standard_normal(3) + 3 * np.eye(3)[int(rng.integers(0, 3))]              # mostly along an axis, hence along a peak
        d /= np.linalg.norm(d)
        pts = []
        for _i in range(n):
            pts.append(tuple(p))
            d = d + 0.3 * rng.standard_normal(3)
            d /= np.linalg.norm(d)
            p = p + step * d
        lines.append(pts)
    for j in range(30):                                                                # one fixel that every one of these crosses
        y = 3 + 0.4 * (j / 29.0 - 0.5)
        lines.append([(x, y, 2) for x in np.arange(1.0, 6.01, 0.25)])
    lines.append([(1 + 5 * i / 299.0, 2.2, 3.1) for i in range(300)])                  # one long line
    bad = [(2, 2, 3), (np.nan, 2, 3), (2.5, 2, 3), (np.inf, 2, 3), (3, 2, 3), (-np.inf, 1, 1), (3.5, 2, 3), (3.5, 2, 3), (3.5, 2, 3), (4, 2, 3),
           (1e30, 2, 3), (4.5, 2, 3), (0.4, 2, 3), (5, 2, 3)]
    lines.append(bad)                                                                  # NaN, +-Inf, outside, duplicate points
    lines += [[], [(9, 9, 9), (9.5, 9, 9)]]
    xyz, npts = pack(lines)
    return fld, mask, xyz, npts


_REF = {}


def _ref(nvec, niter, masked=True, with_q0=False):
    """the restatement's answer for a world, computed once"""
    key = (nvec, niter, masked, with_q0)
    if key not in _REF:
        fld, mask, xyz, npts = _world(nvec)
        q0 = None
        if with_q0:
            q0 = np.random.default_rng(3).integers(0, 1 << 22, npts.size).astype(np.uint32)
            q0[5] = 0
        _REF[key] = (fx.weights(xyz, npts, SHAPE, fld.ovec, fld.f, mask if masked else None, F_THRESH, fx.cos2_of(45), niter, q0), q0)
    return _REF[key]


def _dev_field(fld, mask, dev):
    import torch
    ov = [torch.from_numpy(o).to(dev) for o in fld.ovec]
    f = [torch.from_numpy(a).to(dev) for a in fld.f]
    return ov, f, None if mask is None else torch.from_numpy(mask).to(dev)


def _host_vols(fld):
    """the field as the host tier takes it: [nx, ny, nz, 3] and [nx, ny, nz] Fortran-ordered"""
    nx, ny, nz = fld.shape
    peaks = [o.reshape(3, nz, ny, nx).transpose(3, 2, 1, 0) for o in fld.ovec]
    return peaks, [a.reshape(nz, ny, nx).transpose(2, 1, 0) for a in fld.f]


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _check_device_result(r, ref, what):
    state = r["state"].cpu().numpy()
    assert np.array_equal(r["q"].cpu().numpy(), ref["q"]), what
    assert _same_bits(r["weights"].cpu().numpy(), ref["weights"]), what
    assert _same_bits(r["td"].cpu().numpy(), ref["td"]), what
    assert state[0:2].view(np.float64).tolist() == [ref["a_scale"], ref["mu"]], what
    assert tuple(int(v) for v in state[5:10]) == ref["counts"], (what, state[5:10], ref["counts"])
    cost = r["cost"].cpu().numpy()
    print(what, "cost", cost[[0, -1]], "largest |gpu - exact| / bound", np.max(np.abs(cost - ref["cost"]) / np.maximum(ref["cost_bound"], 1e-300)))
    assert (np.abs(cost - ref["cost"]) <= ref["cost_bound"]).all(), (what, cost, ref["cost"], ref["cost_bound"])
    return cost


@pytest.mark.parametrize("nvec", [1, 2, 3])
def test_device_tier_bit_for_bit(fj, dev, nvec):
    import torch
    fld, mask, xyz, npts = _world(nvec)
    ref, _ = _ref(nvec, 6)
    assert npts.max() == 300 and {0, 1, 2} <= set(npts.tolist()) and ref["counts"][0] > 0 and ref["counts"][1] >= 4
    assert (ref["ids"] >= 0).sum() > 1000 and len(set((ref["ids"][ref["ids"] >= 0] // NVOX).tolist())) == nvec
    ov, f, m = _dev_field(fld, mask, dev)
    dx, dn = torch.from_numpy(xyz).to(dev), torch.from_numpy(npts).to(dev)
    ids, counts = fj.fixel.fixel_assign_device(dx, dn, SHAPE, ov, f, m, F_THRESH, 45)
    assert np.array_equal(ids.cpu().numpy(), ref["ids"]), np.flatnonzero(ids.cpu().numpy() != ref["ids"])[:10]
    assert tuple(counts.tolist()) == ref["counts"][:2]
    q = torch.from_numpy(ref["q"]).to(dev)
    td = fj.fixel.fixel_td_device(ids, dn, q, nvec * NVOX)
    assert np.array_equal(td.cpu().numpy().view(np.uint64), ref["tdq"])
    r = fj.fixel.str_weights_device(dx, dn, SHAPE, ov, f, m, F_THRESH, 45, niter=6)
    cost = _check_device_result(r, ref, "nvec %d" % nvec)
    assert cost[-1] < cost[0]
    again = fj.fixel.str_weights_device(dx, dn, SHAPE, ov, f, m, F_THRESH, 45, niter=6)     # the same call twice: the same bytes
    for k in ("q", "weights", "td", "cost", "state"):
        assert _same_bits(r[k].cpu().numpy(), again[k].cpu().numpy()), k


BIG_SHAPE, BIG_NVEC = (48, 40, 24), 3
FX_COST_GRID, TM_BLOCK = 256, 256      # csrc/fixel.hip: fx_cost's fixed grid and its workgroup, 65 536 fixels a round


def _big_world():
    """_world's field and lines on 48 x 40 x 24 voxels with three peaks: random peak fields (some amplitudes at or below the threshold),
    a mask with holes, about 200 random walks and the hub lines.  Most fixels exist, so every round of a loop over the fixels adds to
    the cost."""
    rng = np.random.default_rng(77)
    fld = Field(BIG_SHAPE, BIG_NVEC)
    nvox = fld.nvox
    for k in range(BIG_NVEC):
        u = 0.35 * rng.standard_normal((3, nvox))
        u[k] += 1
        fld.ovec[k][:] = (u / np.linalg.norm(u, axis=0)).astype(np.float32)
        fld.f[k][:] = (0.02 + 0.6 * rng.random(nvox) / (k + 1)).astype(np.float32)
    hub = fld.lin((24, 20, 12))
    fld.ovec[0][:, hub] = (1, 0, 0)
    fld.f[0][hub] = 0.5
    fld.f[1][fld.lin((2, 1, 1))] = np.nan
    fld.ovec[2][:, fld.lin((48, 40, 24))] = 0                                          # the last fixel of all does not exist
    mask = np.ones(nvox, np.uint8)
    mask[rng.integers(0, nvox, 3000)] = 0
    mask[hub] = 1
    lines = [[], [(24, 20, 12)], [(23.6, 20, 12), (24.4, 20, 12)]]
    for _ in range(200):
        n = int(rng.integers(0, 71))
        step = float(rng.choice([0.05, 0.25, 0.5, 1.0]))
        p = np.array([1, 1, 1]) + rng.random(3) * (np.array(BIG_SHAPE) - 1)
        d = rng.standard_normal(3) + 3 * np.eye(3)[int(rng.integers(0, 3))]
        d /= np.linalg.norm(d)
        pts = []
        for _i in range(n):
            pts.append(tuple(p))
            d = d + 0.3 * rng.standard_normal(3)
            d /= np.linalg.norm(d)
            p = p + step * d
        lines.append(pts)
    for j in range(30):
        y = 20 + 0.4 * (j / 29.0 - 0.5)
        lines.append([(x, y, 12) for x in np.arange(22.0, 27.01, 0.25)])
    xyz, npts = pack(lines)
    return fld, mask, xyz, npts


def test_more_fixels_than_two_rounds_of_the_cost_grid(fj, dev):
    """fx_cost (csrc/fixel.hip) runs a fixed grid of FX_COST_GRID = 256 workgroups of TM_BLOCK = 256 threads, 65 536 fixels a round:
    138 240 fixels are two whole rounds and a partial third.  Every integer quantity bit for bit and each cost within n 2^-53 sum|t| of
    the restatement's exact sum, as for the small worlds; the same call twice gives the same bytes, cost included."""
    import torch
    fld, mask, xyz, npts = _big_world()
    nfix, per_round = BIG_NVEC * fld.nvox, FX_COST_GRID * TM_BLOCK
    print("%d fixels over fx_cost's %d x %d = %d a round: %.2f rounds" % (nfix, FX_COST_GRID, TM_BLOCK, per_round, nfix / per_round))
    assert nfix > 2 * per_round and nfix % per_round, \
        "%d fixels do not pass two rounds of FX_COST_GRID x TM_BLOCK = %d (csrc/fixel.hip) with a partial third" % (nfix, per_round)
    ref = fx.weights(xyz, npts, BIG_SHAPE, fld.ovec, fld.f, mask, F_THRESH, fx.cos2_of(45), 2)
    terms = fx.cost_terms(ref["aq"], ref["tdq"], ref["mu"], ref["a_scale"])
    rounds = [terms[r * per_round:(r + 1) * per_round].sum() for r in range(3)]
    print("the last cost by rounds of the grid: %s of %.6g; bound %.3g" % (rounds, ref["cost"][-1], ref["cost_bound"][-1]))
    assert min(rounds) > 1000 * ref["cost_bound"][-1]                                   # a round left out or added twice is far outside the bound
    assert (ref["ids"] >= 0).sum() > 1000 and len(set((ref["ids"][ref["ids"] >= 0] // fld.nvox).tolist())) == BIG_NVEC
    ov, f, m = _dev_field(fld, mask, dev)
    dx, dn = torch.from_numpy(xyz).to(dev), torch.from_numpy(npts).to(dev)
    r = fj.fixel.str_weights_device(dx, dn, BIG_SHAPE, ov, f, m, F_THRESH, 45, niter=2)
    cost = _check_device_result(r, ref, "%d fixels" % nfix)
    assert cost.size == 3
    again = fj.fixel.str_weights_device(dx, dn, BIG_SHAPE, ov, f, m, F_THRESH, 45, niter=2)
    for k in ("q", "weights", "td", "cost", "state"):
        assert _same_bits(r[k].cpu().numpy(), again[k].cpu().numpy()), k


@pytest.mark.parametrize("nvec,chunk", [(1, "97"), (3, "1"), (2, None)])
def test_host_form_in_chunks_equals_the_device_form(fj, dev, nvec, chunk, monkeypatch):
    """fib_str_weights with the points cut into several chunks (97 points; 1: every line a chunk of its own; None: one chunk) writes
    what fibd_str_weights writes, byte for byte, cost included; `str_weights` on top of it returns the same"""
    import torch
    fld, mask, xyz, npts = _world(nvec)
    ref, q0 = _ref(nvec, 4, with_q0=True)
    ov, f, m = _dev_field(fld, mask, dev)
    dq0 = torch.from_numpy(q0).to(dev)
    r = fj.fixel.str_weights_device(torch.from_numpy(xyz).to(dev), torch.from_numpy(npts).to(dev), SHAPE, ov, f, m, F_THRESH, 45, niter=4, q0=dq0)
    _check_device_result(r, ref, "q0, nvec %d" % nvec)
    if chunk is None:
        monkeypatch.delenv("FIBERS_FIXEL_POINTS", raising=False)
    else:
        monkeypatch.setenv("FIBERS_FIXEL_POINTS", chunk)
    peaks, fs = _host_vols(fld)
    tr = fj.Tract(xyz=xyz, npts=npts, volsize=SHAPE)
    L = fj.lib()
    L.fib_profile_enable(1)
    L.fib_profile_reset()
    try:
        h = fj.str_weights(tr, peaks, fs, mask=mask.reshape(SHAPE[::-1]).transpose(2, 1, 0), f_thresh=F_THRESH, ang_thresh=45, niter=4, q0=q0)
        ms, cnt = C.c_double(0), C.c_int64(0)
        L.fib_profile_get(b"fixel_assign", C.byref(ms), C.byref(cnt))
    finally:
        L.fib_profile_enable(0)
        L.fib_profile_reset()
    want, l = 0, 0                                                                      # the chunks the header's rule cuts: whole lines, at least one
    limit = (1 << 22) if chunk is None else int(chunk)
    while l < npts.size:
        n, l0 = 0, l
        while l < npts.size and (l == l0 or n + npts[l] <= limit):
            n += int(npts[l])
            l += 1
        want += 1
    assert cnt.value == want and (want > 1) == (chunk is not None), (cnt.value, want)
    state = r["state"].cpu().numpy()
    assert _same_bits(h.q, r["q"].cpu().numpy()) and _same_bits(h.weights, r["weights"].cpu().numpy())
    assert _same_bits(np.stack([t.vol.reshape(-1, order="F") for t in h.td]), r["td"].cpu().numpy())
    assert _same_bits(h.cost, r["cost"].cpu().numpy())
    assert h.mu == ref["mu"] == float(state[1:2].view(np.float64)[0])
    assert tuple(h.counts[k] for k in ("points_unassigned", "lines_unassigned", "lines_clamped", "lines_zero", "overflow")) == ref["counts"]
    assert h.q[5] == 0 and ref["counts"][3] >= 1                                       # the line that started at 0 stayed there


def test_niter_zero_and_no_mask(fj, dev):
    import torch
    fld, _, xyz, npts = _world(2)
    ref, _ = _ref(2, 0, masked=False)
    ov, f, _m = _dev_field(fld, None, dev)
    r = fj.fixel.str_weights_device(torch.from_numpy(xyz).to(dev), torch.from_numpy(npts).to(dev), SHAPE, ov, f, None, F_THRESH, 45, niter=0)
    _check_device_result(r, ref, "niter 0")
    assert (ref["q"] == fx.Q_ONE).all() and r["cost"].numel() == 1
    peaks, fs = _host_vols(fld)
    h = fj.str_weights(fj.Tract(xyz=xyz, npts=npts, volsize=SHAPE), peaks, fs, f_thresh=F_THRESH, niter=0)
    assert (h.weights == 1).all() and _same_bits(h.cost, r["cost"].cpu().numpy())


def test_the_rules_derived_by_hand(fj, dev):
    """the tie between two peaks, the tangent exactly on the cone, f == f_thresh, zero and NaN tangents, short lines: the ids derived by
    hand in tests/test_fixel_ref.py"""
    import torch
    fld, xyz, npts, want = rules_case()
    ov, f, _m = _dev_field(fld, None, dev)
    dx, dn = torch.from_numpy(xyz).to(dev), torch.from_numpy(npts).to(dev)
    ids, counts = fj.fixel.fixel_assign_device(dx, dn, SHAPE, ov, f, None, F_THRESH, cos2=0.125)
    assert ids.cpu().tolist() == want and counts.tolist() == [want.count(-1), 4]
    ids, _ = fj.fixel.fixel_assign_device(dx, dn, SHAPE, ov, f, None, F_THRESH, cos2=float(np.nextafter(np.float32(0.125), np.float32(1))))
    assert ids.cpu().tolist()[3] == -1


def _clamp_world():
    fld = Field((3, 1, 1), 1)
    fld.put(0, (1, 1, 1), (1, 0, 0), 1.0)
    fld.put(0, (3, 1, 1), (1, 0, 0), 1e-7)
    return fld


def test_a_lone_line_on_a_strong_fixel_reaches_the_clamp(fj, dev):
    import torch
    fld = _clamp_world()
    xyz, npts = pack([[(1, 1, 1), (1.25, 1, 1)]] + [[(2.8 + 0.01 * i, 1, 1) for i in range(40)]] * 210)
    ref = fx.weights(xyz, npts, fld.shape, fld.ovec, fld.f, None, 0.0, fx.cos2_of(45), 2)
    assert ref["q"][0] == fx.Q_CLAMP and ref["counts"][2] == 1
    ov, f, _m = _dev_field(fld, None, dev)
    r = fj.fixel.str_weights_device(torch.from_numpy(xyz).to(dev), torch.from_numpy(npts).to(dev), fld.shape, ov, f, None, 0.0, 45, niter=2)
    _check_device_result(r, ref, "clamp")


def test_overflow_is_counted_and_raised(fj, dev):
    """41 lines of 100 points in one voxel at q0 = 4095 * 2^20: TDq >= 2^44"""
    import torch
    fld = _clamp_world()
    xyz, npts = pack([[(0.6 + 0.008 * i, 1, 1) for i in range(100)]] * 41)
    q0 = np.full(41, 4095 << 20, np.uint32)
    ref = fx.weights(xyz, npts, fld.shape, fld.ovec, fld.f, None, 0.0, fx.cos2_of(45), 1, q0)
    assert ref["counts"][4] == 4100
    ov, f, _m = _dev_field(fld, None, dev)
    dx, dn, dq = torch.from_numpy(xyz).to(dev), torch.from_numpy(npts).to(dev), torch.from_numpy(q0).to(dev)
    r = fj.fixel.str_weights_device(dx, dn, fld.shape, ov, f, None, 0.0, 45, niter=1, q0=dq, check=False)
    _check_device_result(r, ref, "overflow")
    with pytest.raises(fj.FixelOverflow):
        fj.fixel.str_weights_device(dx, dn, fld.shape, ov, f, None, 0.0, 45, niter=1, q0=dq)
    peaks, fs = _host_vols(fld)
    with pytest.raises(fj.FixelOverflow):
        fj.str_weights(fj.Tract(xyz=xyz, npts=npts, volsize=fld.shape), peaks, fs, f_thresh=0.0, niter=1, q0=q0)


def test_host_form_refuses_bad_counts_before_anything_is_written(fj):
    fld, mask, xyz, npts = _world(1)
    L = fj.lib()
    nl = npts.size
    q = np.full(nl, 0xdeadbeef, np.uint32)
    w = np.full(nl, -7, np.float32)
    td = np.full(NVOX, -7, np.float32)
    cost = np.full(3, -7.0)
    mu = C.c_double(-7.0)
    counts = (C.c_int64 * 5)(*([-7] * 5))
    ov = (C.c_void_p * 1)(fld.ovec[0].ctypes.data)
    fv = (C.c_void_p * 1)(fld.f[0].ctypes.data)
    for bad_npts, npoints in ((npts, xyz.shape[0] - 1), (np.where(np.arange(nl) == 7, -1, npts).astype(np.int32), xyz.shape[0])):
        rc = L.fib_str_weights(0, xyz.ctypes.data, bad_npts.ctypes.data, nl, npoints, 6, 5, 4, 1, ov, fv, mask.ctypes.data, F_THRESH, 0.5, 2, None,
                               q.ctypes.data, w.ctypes.data, td.ctypes.data, C.byref(mu), cost.ctypes.data, counts)
        assert rc == FIB_ERR_INVALID
        assert (q == 0xdeadbeef).all() and (w == -7).all() and (td == -7).all() and (cost == -7).all() and mu.value == -7 and list(counts) == [-7] * 5
    rc = L.fib_str_weights(0, xyz.ctypes.data, npts.ctypes.data, nl, xyz.shape[0], 6, 5, 4, 1, ov, fv, mask.ctypes.data, -0.5, 0.5, 2, None,
                           q.ctypes.data, w.ctypes.data, td.ctypes.data, C.byref(mu), cost.ctypes.data, counts)
    assert rc == FIB_ERR_INVALID and (q == 0xdeadbeef).all()                           # a negative f_thresh


def test_device_tier_refuses_bad_tensors_in_python(fj, dev):
    """the device tier is reached through the module (fj.fixel): every tensor argument as a host tensor, in another element type and one
    element short is an ArgError before any launch"""
    import torch
    from fibers_jl_amd._dev import ArgError
    fld, mask, xyz, npts = _world(2)
    ov, f, m = _dev_field(fld, mask, dev)
    dx, dn = torch.from_numpy(xyz).to(dev), torch.from_numpy(npts).to(dev)
    q0 = torch.full((npts.size,), 1 << 20, dtype=torch.uint32, device=dev)
    ids, _ = fj.fixel.fixel_assign_device(dx, dn, SHAPE, ov, f, m, F_THRESH, 45)
    assert not [n for n in dir(fj) if n in ("fixel_assign_device", "fixel_td_device", "str_weights_device")]
    other = {torch.float32: torch.float64, torch.int32: torch.int64, torch.uint8: torch.int8, torch.uint32: torch.int32}

    def bad(t):
        wrong = t.view(torch.int32).to(torch.int32) if t.dtype == torch.uint32 else t.to(other[t.dtype])
        return {"host": t.cpu(), "dtype": wrong, "short": t.reshape(-1)[:-1].clone()}

    def weights(xyz=dx, npts=dn, o0=ov[0], f0=f[0], mask=m, q0=q0):
        return fj.fixel.str_weights_device(xyz, npts, SHAPE, [o0, ov[1]], [f0, f[1]], mask, F_THRESH, 45, niter=1, q0=q0)

    def assign(xyz=dx, npts=dn, o0=ov[0], f0=f[0], mask=m):
        return fj.fixel.fixel_assign_device(xyz, npts, SHAPE, [o0, ov[1]], [f0, f[1]], mask, F_THRESH, 45)

    def td(ids=ids, npts=dn, q=q0):
        return fj.fixel.fixel_td_device(ids, npts, q, 2 * NVOX)

    calls = ((weights, dict(xyz=dx, npts=dn, o0=ov[0], f0=f[0], mask=m, q0=q0)), (assign, dict(xyz=dx, npts=dn, o0=ov[0], f0=f[0], mask=m)),
             (td, dict(ids=ids, q=q0)))
    passed = []
    for fn, args in calls:
        fn()
        for name, t in args.items():
            for what, b in bad(t).items():
                if name in ("npts", "ids") and what == "short":
                    continue                                                            # (sum(npts) != npoints is the offset scan's to refuse, on the device)
                try:
                    fn(**{name: b})
                except ArgError:
                    continue
                passed.append("%s: %s %s" % (fn.__name__, name, what))
    assert not passed, passed
    with pytest.raises(ArgError):
        fj.fixel.str_weights_device(dx, dn, SHAPE, ov + ov, f + f, m, F_THRESH, 45)      # four peaks
