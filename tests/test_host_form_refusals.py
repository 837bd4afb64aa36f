"""The argument refusals of the single-device host forms (csrc/api.hip: fib_st_eigen, fib_st_recon, fib_vol_xform, fib_warp_points,
fib_warp_volume, fib_warp_invert, fib_rumba_rec, fib_find_peaks, fib_find_peaks_work, fib_prob_stream) that come back before the call takes its
device:
one table, each row a call with one argument spoiled, its return code and a distinguishing piece of fib_last_error().  No GPU is
needed: a row that reached the device would answer FIB_ERR_NO_DEVICE here, and on a machine with a GPU it would run."""
import ctypes as C

import numpy as np
import pytest

F = np.float32
INV, BVAL, BVEC, UNS = -1, -4, -5, -7
ALL = -1                                                               # FIB_DEVICE_ALL

_keep = []                                                             # the arrays behind the pointers below


def _p(shape, dtype=F):
    a = np.zeros(shape, dtype)
    _keep.append(a)
    return a.ctypes.data


M = (C.c_float * 16)(*np.eye(4, dtype=F).reshape(-1).tolist())
VOL_IN, VOL_OUT = _p(2 * 27), _p(2 * 64)                              # 2 frames of 3 x 3 x 3 and of 4 x 4 x 4
FIELD, PTS, PTS_OUT = _p(3 * 64), _p(30), _p(30)
S6 = (C.c_void_p * 6)(*[_p(8) for _ in range(6)])
S6_HOLE = (C.c_void_p * 6)(*[S6[k] if k != 3 else None for k in range(6)])
EVEC, EVAL = _p(9 * 64), _p(3 * 64)
ODF, VERTS, FACES, TOP, NVALID = _p(8 * 181), _p(3 * 362), _p(3 * 720, np.int32), _p(8 * 181, np.int32), _p(8, np.int32)
DWI, MASK, BV, BVC = _p(8 * 4), _p(8, np.uint8), _p(4), _p(12)
SUB = _p(3)

# name -> (the arguments of a call that passes every check made before the device, by position)
GOOD = {
    "fib_st_eigen": [0, S6, 8, EVEC, EVAL],
    "fib_st_recon": [0, VOL_OUT, 4, 4, 4, 1.0, 2.0, EVEC, EVAL],
    "fib_vol_xform": [0, M, VOL_IN, 3, 3, 3, 2, 1, 0, VOL_OUT, 4, 4, 4],
    "fib_warp_points": [0, FIELD, 4, 4, 4, M, M, M, PTS, PTS_OUT, 10],
    "fib_warp_volume": [0, FIELD, 4, 4, 4, M, M, M, VOL_IN, 3, 3, 3, 2, 1, 0, VOL_OUT, 4, 4, 4],
    "fib_warp_invert": [0, FIELD, 4, 4, 4, M, M, 3, VOL_OUT, None, 4, 4, 2],
    "fib_rumba_rec": [0, DWI, 2, 2, 2, 4, MASK, 0, BV, BVC, VERTS, 362, 5, 1.7e-3, 0.2e-3, 3.0e-3, 0.8e-3, 1, 1, 1, 0, "out", None, None],
    "fib_find_peaks": [0, ODF, 8, VERTS, 362, FACES, 720, TOP, NVALID],
    "fib_find_peaks_work": [0, ODF, 8, VERTS, 362, FACES, 720, EVEC, TOP, NVALID],
    "fib_prob_stream": [0, 2, 2, 2, ODF, 181, VERTS, None, None, SUB, 1, 3, 8, 0.7, 0.5, 0.1, 1, 0, "tract"],
}

NULLARG, DIMS, FDIMS = b"NULL argument", b"volume dimensions and nframes must be positive", b"the field's dimensions must be positive"


def _rows():
    """(entry, {position: spoiled value}, code, piece of the message)"""
    t = []
    add = lambda name, change, code, msg: t.append((name, change, code, msg))          # noqa: E731
    # fib_st_eigen
    for pos in (1, 3, 4):
        add("fib_st_eigen", {pos: None}, INV, NULLARG)
    for n in (0, -1):
        add("fib_st_eigen", {2: n}, INV, b"nvox must be positive")
    add("fib_st_eigen", {1: S6_HOLE}, INV, b"NULL structure tensor volume 3")
    # fib_st_recon
    for pos in (1, 7, 8):
        add("fib_st_recon", {pos: None}, INV, NULLARG)
    for pos in (2, 3, 4):
        for n in (0, -1):
            add("fib_st_recon", {pos: n}, INV, b"nx, ny, nz must be positive")
    add("fib_st_recon", {0: ALL}, UNS, b"st_recon runs on one device (FIB_DEVICE_ALL is not supported)")
    add("fib_st_recon", {5: float("nan")}, INV, b"sigma and rho must be finite")
    add("fib_st_recon", {6: float("inf")}, INV, b"sigma and rho must be finite")
    add("fib_st_recon", {5: 9.0}, UNS, b"at most 16 is supported")
    add("fib_st_recon", {6: 8.5}, UNS, b"at most 16 is supported")
    add("fib_st_recon", {0: ALL, 5: 9.0}, UNS, b"st_recon runs on one device")              # the device set is refused before the radii
    # fib_vol_xform
    for pos in (1, 2, 9):
        add("fib_vol_xform", {pos: None}, INV, NULLARG)
    for pos in (3, 4, 5, 6, 10, 11, 12):
        for n in (0, -2):
            add("fib_vol_xform", {pos: n}, INV, DIMS)
    for interp in (-1, 2):
        add("fib_vol_xform", {7: interp}, INV, b"unknown interpolation %d" % interp)
    add("fib_vol_xform", {9: VOL_IN}, INV, b"vol and out must not overlap")
    add("fib_vol_xform", {9: VOL_IN + 4 * 53}, INV, b"vol and out must not overlap")        # out starts in vol's last voxel
    add("fib_vol_xform", {2: VOL_OUT + 4 * 127}, INV, b"vol and out must not overlap")      # vol starts in out's last voxel
    add("fib_vol_xform", {0: ALL}, UNS, b"vol_xform runs on one device (FIB_DEVICE_ALL is not supported)")
    add("fib_vol_xform", {0: ALL, 7: 5}, INV, b"unknown interpolation 5")                    # .. after the argument checks
    # fib_warp_points
    for pos in (1, 5, 6, 7):
        add("fib_warp_points", {pos: None}, INV, NULLARG)
    for pos in (2, 3, 4):
        for n in (0, -1):
            add("fib_warp_points", {pos: n}, INV, FDIMS)
    add("fib_warp_points", {10: -1}, INV, b"npoints must not be negative")
    for pos in (8, 9):
        add("fib_warp_points", {pos: None}, INV, NULLARG)
    add("fib_warp_points", {9: PTS + 12}, INV, b"xyz and out must be the same array or not overlap")
    add("fib_warp_points", {8: PTS_OUT + 4 * 29}, INV, b"xyz and out must be the same array or not overlap")
    add("fib_warp_points", {0: ALL}, UNS, b"warp_points runs on one device (FIB_DEVICE_ALL is not supported)")
    add("fib_warp_points", {0: ALL, 8: None, 9: None, 10: 0}, UNS, b"warp_points runs on one device")   # no points: refused all the same
    add("fib_warp_points", {0: ALL, 10: -1}, INV, b"npoints must not be negative")
    # fib_warp_volume
    for pos in (1, 5, 6, 7, 8, 15):
        add("fib_warp_volume", {pos: None}, INV, NULLARG)
    for pos in (2, 3, 4):
        for n in (0, -1):
            add("fib_warp_volume", {pos: n}, INV, FDIMS)
    for pos in (9, 10, 11, 12, 16, 17, 18):
        for n in (0, -2):
            add("fib_warp_volume", {pos: n}, INV, DIMS)
    add("fib_warp_volume", {2: 0, 9: 0}, INV, FDIMS)                                          # the field's dimensions come first
    for interp in (-1, 2):
        add("fib_warp_volume", {13: interp}, INV, b"unknown interpolation %d" % interp)
    add("fib_warp_volume", {15: VOL_IN}, INV, b"vol and out must not overlap")
    add("fib_warp_volume", {15: VOL_IN + 4 * 53}, INV, b"vol and out must not overlap")
    add("fib_warp_volume", {8: VOL_OUT + 4 * 127}, INV, b"vol and out must not overlap")
    add("fib_warp_volume", {0: ALL}, UNS, b"warp_volume runs on one device (FIB_DEVICE_ALL is not supported)")
    add("fib_warp_volume", {0: ALL, 13: 5}, INV, b"unknown interpolation 5")
    # fib_warp_invert
    for pos in (1, 5, 6, 8):
        add("fib_warp_invert", {pos: None}, INV, NULLARG)
    for pos in (2, 3, 4, 10, 11, 12):
        for n in (0, -1):
            add("fib_warp_invert", {pos: n}, INV, b"the field's and the output's dimensions must be positive")
    add("fib_warp_invert", {7: -1}, INV, b"niter must not be negative")
    add("fib_warp_invert", {0: ALL}, UNS, b"warp_invert runs on one device (FIB_DEVICE_ALL is not supported)")
    add("fib_warp_invert", {0: ALL, 7: -1}, INV, b"niter must not be negative")
    # fib_rumba_rec: its own checks, then those of the plan constructor -- all before the device, FIB_DEVICE_ALL or not
    for dev in (0, ALL):
        for pos in (1, 6, 21):
            add("fib_rumba_rec", {0: dev, pos: None}, INV, NULLARG)
        for pos in (2, 3, 4):
            for n in (0, -1):
                add("fib_rumba_rec", {0: dev, pos: n}, INV, b"volume dimensions must be positive")
        add("fib_rumba_rec", {0: dev, 8: None}, BVAL, b"Missing b-value table")
        add("fib_rumba_rec", {0: dev, 5: 0}, BVAL, b"Missing b-value table")
        add("fib_rumba_rec", {0: dev, 9: None}, BVEC, b"Missing gradient table")
        add("fib_rumba_rec", {0: dev, 10: None}, INV, b"invalid ODF tessellation")
        for n in (0, 361):
            add("fib_rumba_rec", {0: dev, 11: n}, INV, b"invalid ODF tessellation")
        add("fib_rumba_rec", {0: dev, 11: 100}, UNS, b"sphere_362/642/724 only")
    add("fib_rumba_rec", {1: None, 8: None}, INV, NULLARG)                                    # the form's own checks come first
    # the peak finders: their own checks, then the plan constructor's vertex limit
    for name, ptrs in (("fib_find_peaks", (1, 3, 5, 7, 8)), ("fib_find_peaks_work", (1, 3, 5, 7, 8, 9))):
        for dev in (0, ALL):
            for pos in ptrs:
                add(name, {0: dev, pos: None}, INV, NULLARG)
            for change in ({2: 0}, {2: -1}, {4: 0}, {4: 1}, {4: 361}, {6: 0}, {6: -1}):
                add(name, {0: dev, **change}, INV, b"invalid sizes")
            add(name, {0: dev, 4: 65536}, UNS, b"too many ODF vertices")
            for pos in ptrs:                                                                # a NULL pointer is named before a bad size
                for change in ({2: 0}, {4: 0}, {4: 1}, {4: -1}, {6: 0}):
                    add(name, {0: dev, pos: None, **change}, INV, NULLARG)
    # fib_prob_stream: out, the device set, the pointers, the dimensions, nsub -- in that order
    one_dev = b"prob_stream runs on one device (FIB_DEVICE_ALL is not supported)"
    add("fib_prob_stream", {18: None}, INV, b"NULL out")
    add("fib_prob_stream", {18: None, 0: ALL, 4: None}, INV, b"NULL out")
    add("fib_prob_stream", {0: ALL}, UNS, one_dev)
    add("fib_prob_stream", {0: ALL, 4: None}, UNS, one_dev)                                  # the device set is refused before a NULL odf
    add("fib_prob_stream", {0: ALL, 1: 0, 10: 0}, UNS, one_dev)
    for pos in (4, 6, 9):
        add("fib_prob_stream", {pos: None}, INV, NULLARG)
        add("fib_prob_stream", {pos: None, 2: 0, 10: 0}, INV, NULLARG)                       # a NULL pointer is named before a bad size
    for pos in (1, 2, 3):
        for n in (0, -1):
            add("fib_prob_stream", {pos: n}, INV, b"volume dimensions must be positive")
    add("fib_prob_stream", {3: 0, 10: 0}, INV, b"volume dimensions must be positive")
    for n in (0, -1):
        add("fib_prob_stream", {10: n}, INV, b"sublist must hold at least one offset")
    return t


ROWS = _rows()


@pytest.fixture(scope="module")
def rumba_out(fj):
    from fibers_jl_amd import _lib
    out = _lib.RumbaOut()
    out.fodf, out.fgm, out.fcsf, out.gfa, out.var = _p(8 * 181), _p(8), _p(8), _p(8), _p(8)
    for i in range(5):
        out.peak[i] = _p(24)
    return out


@pytest.fixture(scope="module")
def tract_out(fj):
    from fibers_jl_amd import _lib
    return _lib.TractOut()


def test_every_entry_has_rows():
    assert {r[0] for r in ROWS} == set(GOOD) and len(GOOD) == 10


@pytest.mark.parametrize("name", sorted(GOOD))
def test_refusals_before_the_device(fj, rumba_out, tract_out, name):
    L = fj.lib()
    fn = getattr(L, name)
    rows = [r for r in ROWS if r[0] == name]
    assert rows
    for _, change, code, msg in rows:
        args = [C.byref({"out": rumba_out, "tract": tract_out}[a]) if isinstance(a, str) else a for a in GOOD[name]]
        for pos, v in change.items():
            args[pos] = v
        rc = fn(*args)
        err = L.fib_last_error()
        assert rc == code and msg in err, (name, change, rc, err)
    # nothing was written
    assert not any(a.any() for a in _keep)
    assert not any(bytes(tract_out))
