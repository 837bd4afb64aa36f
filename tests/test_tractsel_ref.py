"""The NumPy restatement of tract selection and connectomes (tests/tractsel_ref.py) against answers counted by hand from the
definitions in include/fibers_hip.h ("Tract selection and connectomes").  tests/test_gpu_tractsel.py holds the HIP kernels to this
restatement bit for bit, so what is pinned here is what the kernels are held to.  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tractmap_ref as tm  # noqa: E402
import tractsel_ref as ts  # noqa: E402
from test_tractmap_ref import SHAPE as WSHAPE, witnesses  # noqa: E402

SHAPE = (7, 6, 5)
NVOX = 7 * 6 * 5
A, B, Cb = 1, 2, 0x80000000                                    # ROI 0, ROI 1, ROI 31


def lin(x, y, z, shape=SHAPE):
    return (x - 1) + shape[0] * ((y - 1) + shape[1] * (z - 1))


def rois():
    """32 ROIs in the plane z = 2, rows y = 2, 3:  A = ROI 0: x in {2, 3};  C = ROI 31: x = 4;  B = ROI 1: x in {5, 6}; the rest empty.
    Non-zero is what counts: the values are 1, 2 and 255"""
    r = np.zeros((32,) + SHAPE[::-1], np.uint8)                 # [roi][z][y][x]: x fastest
    r[0, 1, 1:3, 1:3] = 1
    r[1, 1, 1:3, 4:6] = 2
    r[31, 1, 1:3, 3] = 255
    return r.reshape(32, NVOX)


def lines():
    """eight lines and, counted by hand, {visit, end0, end1} of each"""
    nan, inf, big = np.nan, np.inf, 1e30
    ls = [([(2.5, 2, 2), (3.5, 2, 2)], (A | Cb, A, Cb)),                                   # ties on A's border: 2.5 -> 2 (in A), 3.5 -> 4 (C, not A)
          ([(2, 2, 2), (1, 2, 2), (2, 3, 2), (4.5, 2, 2), (5.5, 2, 2)], (A | B | Cb, A, B)),   # leaves A and re-enters; 4.5 -> 4 (C), 5.5 -> 6 (B)
          ([(5, 3, 2)], (B, B, B)),                                                      # one point: end0 == end1
          ([], (0, 0, 0)),                                                               # empty
          ([(nan, 2, 2), (2, 2, 2), (inf, 2, 2), (6, 2, 2), (big, 2, 2)], (A | B, 0, 0)),  # both ends outside, the inside points still visit
          ([(3, 2, 2), (3, nan, 2), (-big, 2, 2), (3, 3, 2)], (A, A, A)),                  # NaN / -1e30 as interior points
          ([(0.5, 2, 2)], (0, 0, 0)),                                                    # 0.5 -> 0: one point, outside
          ([(4, 2, 2), (4, 3, 2)], (Cb, Cb, Cb))]
    npts = np.array([len(p) for p, _ in ls], np.int32)
    xyz = np.array([q for p, _ in ls for q in p], np.float32).reshape(-1, 3)
    return xyz, npts, np.array([h for _, h in ls], np.uint32)


def labels():
    """x <= 3: 10, x = 4: 20, x >= 5: 30; the plane z = 5 is -4; voxel (7, 6, 1) is 1000"""
    lab = np.zeros(SHAPE[::-1], np.int32)
    lab[:, :, :3] = 10
    lab[:, :, 3] = 20
    lab[:, :, 4:] = 30
    lab[4] = -4
    lab[0, 5, 6] = 1000
    return lab.reshape(-1)


def remap():
    r = np.zeros(40, np.int32)
    r[10], r[20], r[30] = 1, 2, 5
    return r


def conn_lines():
    """the eight lines and a ninth from a negative label to a label beyond remap"""
    xyz, npts, _ = lines()
    return np.concatenate([xyz, np.array([[2, 2, 5], [7, 6, 1]], np.float32)]), np.concatenate([npts, [2]]).astype(np.int32)


def test_roi_pack_and_predicates():
    bits = ts.roi_pack(rois())
    assert bits.dtype == np.uint32 and bits[lin(2, 2, 2)] == A and bits[lin(4, 3, 2)] == Cb and bits[lin(6, 2, 2)] == B and bits[lin(2, 2, 3)] == 0
    assert int((bits != 0).sum()) == 10
    both = ts.roi_pack(np.array([[0, 1, 2, 255], [7, 0, 0, 1]], np.uint8))
    assert list(both) == [2, 1, 1, 3]
    xyz, npts, want = lines()
    assert np.array_equal(ts.hits(xyz, npts, SHAPE, bits), want)
    # the tie witnesses of the tract maps, each a line of its own, in an ROI that fills the volume: visited iff inside
    wx, wv = witnesses()
    h = ts.hits(wx, [1] * len(wx), WSHAPE, np.ones(6 * 5 * 4, np.uint32))
    assert np.array_equal(h[:, 0], (wv >= 0).astype(np.uint32)) and np.array_equal(h[:, 0], h[:, 1]) and np.array_equal(h[:, 1], h[:, 2])


RULES = [(dict(), [1, 1, 1, 1, 1, 1, 1, 1]),                                               # every mask 0, window (0, 0): all, the empty line too
         (dict(visit_all=A), [1, 1, 0, 0, 1, 1, 0, 0]),
         (dict(visit_all=A | B), [0, 1, 0, 0, 1, 0, 0, 0]),
         (dict(visit_none=A), [0, 0, 1, 1, 0, 0, 1, 1]),
         (dict(visit_none=A | B | Cb), [0, 0, 0, 1, 0, 0, 1, 0]),
         (dict(end_any=A), [1, 1, 0, 0, 0, 1, 0, 0]),
         (dict(end_any=A | B), [0, 1, 0, 0, 0, 0, 0, 0]),                                  # A holds one end and B the other
         (dict(end_both=A), [0, 0, 0, 0, 0, 1, 0, 0]),
         (dict(end_both=B), [0, 0, 1, 0, 0, 0, 0, 0]),                                     # the one-point line: both ends are its point
         (dict(end_both=Cb), [0, 0, 0, 0, 0, 0, 0, 1]),
         (dict(visit_all=A, visit_none=B, end_any=Cb), [1, 0, 0, 0, 0, 0, 0, 0]),
         (dict(visit_all=A | B, end_both=A), [0, 0, 0, 0, 0, 0, 0, 0]),
         (dict(min_npts=2, max_npts=4), [1, 0, 0, 0, 0, 1, 0, 1]),                         # npts = 2 5 1 0 5 4 1 2: both edges are inside the window
         (dict(min_npts=5), [0, 1, 0, 0, 1, 0, 0, 0]),                                     # max_npts = 0: no upper edge
         (dict(max_npts=1), [0, 0, 1, 1, 0, 0, 1, 0]),
         (dict(min_npts=1, max_npts=1), [0, 0, 1, 0, 0, 0, 1, 0]),
         (dict(visit_all=A, min_npts=3), [0, 1, 0, 0, 1, 1, 0, 0])]


@pytest.mark.parametrize("kw,want", RULES)
def test_rule(kw, want):
    xyz, npts, _ = lines()
    keep, h, counts = ts.select(xyz, npts, SHAPE, ts.roi_pack(rois()), **kw)
    assert keep.dtype == np.uint8 and list(keep) == want
    assert counts == [sum(want), int(npts[np.array(want, bool)].sum())]


def test_visit_all_and_visit_none_of_one_roi_are_complements():
    xyz, npts, _ = lines()
    bits = ts.roi_pack(rois())
    for r in (A, B, Cb, 4):                                                                # (ROI 2 is empty: visit_all keeps nothing)
        a = ts.select(xyz, npts, SHAPE, bits, visit_all=r)[0]
        b = ts.select(xyz, npts, SHAPE, bits, visit_none=r)[0]
        assert (a + b == 1).all()


def test_gather_is_a_stable_copy():
    xyz, npts, _ = lines()
    xyz.view(np.uint32)[1, 2] = 0x7FC12345                                                  # a NaN payload, and -0.0
    xyz[0, 1] = -0.0
    sc = np.arange(2 * len(xyz), dtype=np.float32).reshape(-1, 2)
    x, n, i, s = ts.gather(xyz, npts, [1, 0, 7, 0, 0, 255, 0, 0], sc)                       # any non-zero flag keeps
    assert list(n) == [2, 1, 4] and list(i) == [0, 2, 5] and n.dtype == np.int32 and i.dtype == np.int64
    assert np.array_equal(x.view(np.uint32), np.concatenate([xyz[0:2], xyz[7:8], xyz[13:17]]).view(np.uint32))
    assert x.view(np.uint32)[1, 2] == 0x7FC12345 and np.signbit(x[0, 1])
    assert np.array_equal(s, np.concatenate([sc[0:2], sc[7:8], sc[13:17]]))
    x, n, i, s = ts.gather(xyz, npts, np.ones(8, np.uint8))
    assert np.array_equal(x.view(np.uint32), xyz.view(np.uint32)) and np.array_equal(n, npts) and list(i) == list(range(8)) and s is None
    x, n, i, _ = ts.gather(xyz, npts, np.zeros(8, np.uint8))
    assert x.shape == (0, 3) and n.size == 0 and i.size == 0
    with pytest.raises(ValueError):
        ts.gather(xyz, [2, 5, 1, 0, 5, 4, 1, 1], np.ones(8, np.uint8))
    # the LINES density of the gathered lines is the density of those lines
    keep = ts.select(xyz, npts, SHAPE, ts.roi_pack(rois()), visit_all=A)[0]
    x, n, _, _ = ts.gather(xyz, npts, keep)
    whole = tm.density(xyz, npts, SHAPE, tm.LINES)[0]
    rest = tm.density(*ts.gather(xyz, npts, 1 - keep)[:2], SHAPE, tm.LINES)[0]
    assert np.array_equal(tm.density(x, n, SHAPE, tm.LINES)[0] + rest, whole)


def test_connectome_with_remap():
    xyz, npts = conn_lines()
    C, W, assign, n, bound = ts.connectome(xyz, npts, SHAPE, labels(), 3, remap(), volres=(2.0, 0.5, 3.0))
    # ends: (10, 20) (10, 30 -> 5 > L) (30) empty (outside, outside) (10, 10) (outside) (20, 20) (-4, 1000: both beyond remap)
    assert assign.tolist() == [[1, 2], [1, 0], [0, 0], [0, 0], [0, 0], [1, 1], [0, 0], [2, 2], [0, 0]]
    want = np.zeros((4, 4), np.uint32)
    want[0, 0] = 4                                                                          # lines 2, 4, 6, 8: both ends unassigned
    want[0, 1] = want[1, 0] = 1
    want[1, 2] = want[2, 1] = 1
    want[1, 1] = want[2, 2] = 1                                                             # self-connections: once, on the diagonal
    assert C.dtype == np.uint32 and np.array_equal(C, want) and n == 8
    assert np.array_equal(C, C.T) and int(np.triu(C).sum()) == n == int((npts >= 1).sum())
    # lengths in mm, voxels of 2 x 0.5 x 3: line 0 is one voxel along x; line 7 one voxel along y; line 1 by hand; line 5 has a NaN point
    assert W[1, 2] == W[2, 1] == 2.0 and W[2, 2] == 0.5 and W[3, 3] == 0.0
    assert W[0, 1] == W[1, 0] == ((2.0 + np.sqrt(4.25)) + np.sqrt(25.25)) + 2.0
    assert np.isnan(W[1, 1]) and np.isnan(W[0, 0])
    assert bound[1, 2] == (2 + 1) * 2.0 ** -52 * 2.0 and bound[0, 1] == (5 + 1) * 2.0 ** -52 * W[0, 1]
    m = ts.mean_length(C, np.nan_to_num(W))
    assert m[1, 2] == 2.0 and m[3, 3] == 0.0 and m[0, 3] == 0.0
    ok = ts.weights_close(W, W, bound, C)
    assert ok.all() and not ts.weights_close(W + np.where(C == 0, 1e-300, 0), W, bound, C).all()
    # y <= L now holds for 5
    C5, _, a5, n5, _ = ts.connectome(xyz, npts, SHAPE, labels(), 5, remap())
    assert a5.tolist()[:3] == [[1, 2], [1, 5], [5, 5]] and C5[1, 5] == C5[5, 1] == 1 and C5[5, 5] == 1 and C5[0, 0] == 3 and n5 == 8
    assert ts.connectome(xyz, npts, SHAPE, labels(), 5, remap())[1] is None


def test_connectome_without_remap_and_identities():
    xyz, npts = conn_lines()
    lab = labels()
    C, _, assign, n, _ = ts.connectome(xyz, npts, SHAPE, lab, 30)
    assert assign.tolist() == [[10, 20], [10, 30], [30, 30], [0, 0], [0, 0], [10, 10], [0, 0], [20, 20], [0, 0]]       # -4 and 1000 are no nodes
    assert C[10, 20] == C[20, 10] == 1 and C[10, 30] == 1 and C[30, 30] == 1 and C[0, 0] == 3 and C.sum() == 3 + 2 + 2 + 3 and n == 8
    C20 = ts.connectome(xyz, npts, SHAPE, lab, 20)[0]
    assert C20.shape == (21, 21) and C20[0, 10] == C20[10, 0] == 1 and C20[0, 0] == 4
    # 2 C[i][i] + sum_{j != i} C[i][j] = the ENDPOINTS density summed over the voxels of node i
    ends = tm.density(xyz, npts, SHAPE, tm.ENDPOINTS)[0]
    for L, rm in ((30, None), (3, remap()), (5, remap())):
        Cm = ts.connectome(xyz, npts, SHAPE, lab, L, rm)[0].astype(np.int64)
        nodes = np.array([ts.node(v, lab, rm, L) for v in range(NVOX)])
        for i in range(1, L + 1):
            assert Cm[i, i] + Cm[i].sum() == int(ends[nodes == i].sum()), (L, i)
    # batches sum into one matrix whatever their order
    a = ts.connectome(xyz[:7], npts[:2], SHAPE, lab, 30, volres=(1, 1, 1))
    b = ts.connectome(xyz[7:], npts[2:], SHAPE, lab, 30, volres=(1, 1, 1), into=(a[0], a[1]))
    assert np.array_equal(b[0], C) and a[3] + b[3] == n
    with pytest.raises(ValueError):
        ts.connectome(xyz, [2, 5, 1, 0, 5, 4, 1, 2, -2, 4], SHAPE, lab, 30)
