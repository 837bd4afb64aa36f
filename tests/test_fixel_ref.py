"""CPU tests: the NumPy restatement of the tractogram weights (tests/fixel_ref.py) against answers derived by hand from the definitions
in include/fibers_hip.h ("Tractogram weights"), and the host-side weighted connectome against a loop."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fixel_ref as fx  # noqa: E402


class Field:
    """a peak field being filled: ovec[k] float32 [3, nvox], f[k] float32 [nvox]; voxels are 1-based (x, y, z)"""

    def __init__(self, shape, nvec):
        self.shape, self.nvec = tuple(shape), nvec
        self.nvox = shape[0] * shape[1] * shape[2]
        self.ovec = [np.zeros((3, self.nvox), np.float32) for _ in range(nvec)]
        self.f = [np.zeros(self.nvox, np.float32) for _ in range(nvec)]

    def lin(self, v):
        return (v[0] - 1) + self.shape[0] * ((v[1] - 1) + self.shape[1] * (v[2] - 1))

    def put(self, k, v, direction, amp):
        self.ovec[k][:, self.lin(v)] = direction
        self.f[k][self.lin(v)] = amp
        return k * self.nvox + self.lin(v)


def pack(lines):
    npts = np.array([len(l) for l in lines], np.int32)
    xyz = np.concatenate([np.asarray(l, np.float32).reshape(-1, 3) for l in lines] + [np.zeros((0, 3), np.float32)])
    return xyz, npts


def test_separate_bundles_reach_their_weight_in_one_iteration_and_stay():
    """bundle b: m_b identical lines of n_b points inside ONE voxel, along its only fixel of amplitude f_b.  N_s = n Aq, D_s = n (m n q),
    so w' = f / (mu m n) whatever w was, and with the largest f = 1 the quantisation is exact: mu = sum f / sum (m n)."""
    fld = Field((6, 5, 4), 1)
    f, m, n = (0.5, 1.0), (3, 5), (4, 8)
    vox = ((2, 2, 2), (5, 4, 3))
    ids = [fld.put(0, v, (1, 0, 0), a) for v, a in zip(vox, f)]
    lines = []
    for b in range(2):
        lines += [[(vox[b][0] - 0.2 + 0.03 * i, vox[b][1], vox[b][2]) for i in range(n[b])]] * m[b]
    xyz, npts = pack(lines)
    mu = (f[0] + f[1]) / (m[0] * n[0] + m[1] * n[1])
    want = np.repeat([f[b] / (mu * m[b] * n[b]) for b in range(2)], m)
    first = None
    for niter in (0, 1, 2, 7):
        r = fx.weights(xyz, npts, fld.shape, fld.ovec, fld.f, f_thresh=0.03, niter=niter)
        assert r["mu"] == mu and r["a_scale"] == 2.0 ** 30
        assert r["counts"] == (0, 0, 0, 0, 0)
        assert np.array_equal(r["ids"], np.repeat(ids, [m[0] * n[0], m[1] * n[1]]))
        if niter == 0:
            assert (r["q"] == fx.Q_ONE).all() and (r["weights"] == 1).all()
            continue
        assert np.abs(r["q"].astype(np.float64) - want * 2.0 ** 20).max() <= 0.5 + 1e-6          # exact, up to the one rint
        first = r["q"] if first is None else first
        assert np.array_equal(r["q"], first)                                                      # and q stays
        for b in range(2):                                                                        # the fitted density meets the amplitude
            assert abs(r["td"].reshape(-1)[ids[b]] - f[b]) <= mu * m[b] * n[b] * 2.0 ** -21 + 1e-7
        assert r["cost"][-1] <= (mu * max(m[0] * n[0], m[1] * n[1]) * 2.0 ** -21) ** 2 * 2 < r["cost"][0]


def test_crossing_bundles_of_unequal_seeding_density():
    """bundle A along x (4 m lines), bundle B along y (m lines), crossing in one voxel that has a fixel for each; every amplitude 1.  The
    counts differ by four, the weighted densities do not: m_A w_A = m_B w_B."""
    fld = Field((5, 5, 1), 2)
    for i in range(1, 6):
        if i != 3:
            fld.put(0, (i, 3, 1), (1, 0, 0), 1.0)
            fld.put(0, (3, i, 1), (0, 1, 0), 1.0)
    fa = fld.put(0, (3, 3, 1), (1, 0, 0), 1.0)
    fb = fld.put(1, (3, 3, 1), (0, 1, 0), 1.0)
    m = 3
    A = [[(i, 3, 1) for i in range(1, 6)]] * (4 * m)
    B = [[(3, i, 1) for i in range(1, 6)]] * m
    xyz, npts = pack(A + B)
    r = fx.weights(xyz, npts, fld.shape, fld.ovec, fld.f, niter=3)
    ids = r["ids"].reshape(-1, 5)
    assert (ids[:4 * m, 2] == fa).all() and (ids[4 * m:, 2] == fb).all() and (r["ids"] >= 0).all()
    counts = np.bincount(r["ids"], minlength=2 * fld.nvox)
    assert counts[fa] == 4 * counts[fb] == 4 * m
    w = r["weights"]
    assert (w[:4 * m] == w[0]).all() and (w[4 * m:] == w[-1]).all()
    assert abs(w[-1] / w[0] - 4) < 1e-5
    td = r["td"].reshape(-1)
    exist = fx.exists(fld.ovec, fld.f, None, 0.03, fld.shape).reshape(-1)
    assert exist.sum() == 10 and np.abs(td[exist] - 1).max() < 1e-5 and (td[~exist] == 0).all()
    assert abs(td[fa] - td[fb]) < 1e-5


def test_cost_falls_where_lines_share_fixels():
    rng = np.random.default_rng(5)
    fld = Field((12, 1, 1), 1)
    for i in range(1, 13):
        fld.put(0, (i, 1, 1), (1, 0, 0), 0.2 + rng.random())
    lines = []
    for _ in range(30):
        a = int(rng.integers(1, 9))
        b = int(rng.integers(a + 2, 13))
        lines.append([(x, 1, 1) for x in np.arange(a, b + 0.25, 0.5)])
    xyz, npts = pack(lines)
    r = fx.weights(xyz, npts, fld.shape, fld.ovec, fld.f, niter=20)
    assert r["counts"][0] == 0 and r["counts"][4] == 0
    assert r["cost"].size == 21 and r["cost"][20] < r["cost"][0]
    assert (np.diff(r["cost"]) <= 1e-12).all()                        # ISRA does not raise the misfit (up to the quantisation of q)
    assert len(set(r["q"].tolist())) > 5


def rules_case():
    """(field, xyz, npts, the ids derived by hand at f_thresh = 0.03, cos2 = 0.125): tie -> smallest k; the cone with representable values;
    f == f_thresh does not exist; zero and non-finite tangents; short lines.  Shared with tests/test_gpu_fixel.py."""
    fld = Field((6, 5, 4), 3)
    fld.put(0, (2, 2, 2), (1, 0, 0), 0.5)
    fld.put(1, (2, 2, 2), (0, 1, 0), 0.5)                             # tangent (1, 1, 0): |d_0| = |d_1| -> k = 0
    fld.put(2, (2, 2, 2), (0, 0, 1), 0.9)
    fld.put(0, (4, 2, 2), (0.5, 0, 0), 0.5)                           # tangent (3, 3, 0): d = 1.5, d^2 = 2.25 = cos2 * 18 with cos2 = 0.125
    fld.put(0, (5, 4, 3), (1, 0, 0), np.float32(0.03))                # f == f_thresh: no fixel
    lines = [
        [(1.75, 1.75, 2), (2.25, 2.25, 2)],                           # both points in voxel (2, 2, 2)
        [(2.5, 0.5, 2), (4.25, 2.25, 2), (5.5, 3.5, 2)],              # outside | tangent (3, 3, 0) in voxel (4, 2, 2) | a voxel without fixel
        [(5, 4, 3), (5.25, 4, 3)],
        [(2, 2, 2)], [],
        [(2, 2, 2), (2, 2, 2), (2, 2, 2), (2.25, 2, 2)],              # duplicates: zero tangent at point 1, one-sided zero at point 0
        [(2, 2, 2), (np.nan, 2, 2), (2.25, 2, 2)],
    ]
    xyz, npts = pack(lines)
    v222, v422 = fld.lin((2, 2, 2)), fld.lin((4, 2, 2))
    return fld, xyz, npts, [v222, v222, -1, v422, -1, -1, -1, -1, -1, -1, v222, v222, -1, -1, -1]


def test_the_rules_of_the_fixel_of_a_point():
    fld, xyz, npts, want = rules_case()
    nv = fld.nvox
    v222, v422 = fld.lin((2, 2, 2)), fld.lin((4, 2, 2))
    ids, n_un, n_without = fx.assign(xyz, npts, fld.shape, fld.ovec, fld.f, None, np.float32(0.03), np.float32(0.125))
    assert ids.tolist() == want
    assert n_un == want.count(-1) and n_without == 4
    ids, _, _ = fx.assign(xyz, npts, fld.shape, fld.ovec, fld.f, None, np.float32(0.03), np.nextafter(np.float32(0.125), np.float32(1)))
    assert ids[3] == -1                                               # just inside the cone no longer
    mask = np.ones(nv, np.uint8)
    mask[v222] = 0
    ids, _, _ = fx.assign(xyz, npts, fld.shape, fld.ovec, fld.f, mask, np.float32(0.03), np.float32(0.125))
    assert (ids >= 0).sum() == 1 and ids[3] == v422


def test_clamp_zero_and_overflow():
    fld = Field((3, 1, 1), 1)
    strong = fld.put(0, (1, 1, 1), (1, 0, 0), 1.0)
    fld.put(0, (3, 1, 1), (1, 0, 0), 1e-7)                            # exists under f_thresh = 0, Aq = rint(107.37) = 107
    crowd = [[(2.8 + 0.01 * i, 1, 1) for i in range(40)]] * 210       # 8400 points on the weak fixel
    lone = [[(1, 1, 1), (1.25, 1, 1)]]
    xyz, npts = pack(lone + crowd)
    r = fx.weights(xyz, npts, fld.shape, fld.ovec, fld.f, f_thresh=0.0, niter=2)
    assert r["aq"][strong] == 2 ** 30 and r["aq"][2] == 107
    assert r["q"][0] == fx.Q_CLAMP and r["counts"][2] == 1            # mu ~ 1 / 8402: the lone line wants 8402 / 2 = 4201 > 4096
    # 41 lines of 100 points in one voxel at q0 = 4095 * 2^20: TDq = 41 * 100 * 4095 * 2^20 >= 2^44, seen by the first update's gathers
    lines = [[(0.6 + 0.008 * i, 1, 1) for i in range(100)]] * 41
    xyz, npts = pack(lines)
    q0 = np.full(41, 4095 << 20, np.uint32)
    r = fx.weights(xyz, npts, fld.shape, fld.ovec, fld.f, f_thresh=0.0, niter=1, q0=q0)
    assert r["counts"][4] == 4100
    r = fx.weights(xyz, npts, fld.shape, fld.ovec, fld.f, f_thresh=0.0, niter=0, q0=q0)
    assert r["counts"][4] == 0 and np.array_equal(r["q"], q0)
    # a line at q = 0 stays there
    q0 = np.full(41, fx.Q_ONE, np.uint32)
    q0[7] = 0
    r = fx.weights(xyz, npts, fld.shape, fld.ovec, fld.f, f_thresh=0.0, niter=3, q0=q0)
    assert r["q"][7] == 0 and r["counts"][3] == 1 and (np.delete(r["q"], 7) > 0).all()


def test_connectome_weighted_against_a_loop(fj):
    rng = np.random.default_rng(11)
    L = 6
    assign = rng.integers(0, L + 1, (200, 2)).astype(np.int32)
    w = rng.random(200).astype(np.float32)
    got = fj.connectome_weighted(assign, w, L)
    ref = fx.connectome_loop(assign, w, L)
    assert got.dtype == np.float64 and got.shape == (L + 1, L + 1)
    assert np.array_equal(got, ref) and np.array_equal(got, got.T)
    assert abs(np.triu(got).sum() - w.astype(np.float64).sum()) < 1e-9
    assert np.array_equal(fj.connectome_weighted(np.zeros((0, 2), np.int32), np.zeros(0, np.float32), 2), np.zeros((3, 3)))
