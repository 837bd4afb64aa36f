"""The single-device host forms of csrc/api.hip as a family: what each answers to FIB_DEVICE_ALL and to a device index out of range,
and two threads that call all of them on one device at once (each form holds its worker's lock for the call: the results are those of
a call made alone, nothing deadlocks, and fib_trim from a third thread comes back)."""
import ctypes as C
import os
import sys
import threading

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_volxform as TV  # noqa: E402
import test_gpu_warp as TW  # noqa: E402
import volxform_ref as V  # noqa: E402
import warp_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

F = np.float32
NO_DEVICE, UNSUPPORTED = -2, -7
SMALL, LARGE, FSHAPE, OSHAPE = TW.SMALL, TW.LARGE, TW.FSHAPE, TW.OSHAPE


class Inputs:
    """the operands of one call of each form (the generators of the warp and vol_xform tests), made once"""

    def __init__(self, fj):
        rng = np.random.default_rng(44)
        self.frames = TV._floats(5, SMALL, 13)
        self.out2in = TW._m16(V.out2in(V.oblique()))
        self.field = np.ascontiguousarray(R.smooth_field(TW.FV2R, FSHAPE, 2.0))
        self.vol_mats = [TW._m16(m) for m in TW._vol_mats(SMALL, LARGE)]
        self.pt_mats = [TW._m16(m) for m in R.point_matrices(TW.FV2R, TW.IN_V2R, TW.OUT_V2R, TW.PRE, TW.POST, 1)]
        self.points = TW._points(300, 12)
        self.inv_mats = [TW._m16(m) for m in R.invert_matrices(TW.FV2R, TW.OV2R)]
        self.st_vol = rng.standard_normal((9, 10, 12)).astype(F)             # [nz, ny, nx]
        self.S = [rng.standard_normal(500).astype(F) for _ in range(6)]
        self.S_ptrs = (C.c_void_p * 6)(*[s.ctypes.data for s in self.S])
        self.verts = np.asfortranarray(fj.sphere_362.vertices, dtype=F)
        self.faces = np.asfortranarray(fj.sphere_362.faces, dtype=np.int32)
        self.nvert = fj.sphere_362.nvert
        self.odf = rng.uniform(0.0, 1.0, (self.nvert, 64)).astype(F)         # planar: a row of 64 voxels per vertex
        # fib_rumba_rec (the refusals only): 2 x 2 x 2 voxels, 1 + 6 frames
        self.bval = np.array([0] + [1000] * 6, F)
        self.bvec = np.ascontiguousarray(np.vstack([np.zeros((1, 3)), np.eye(3), np.eye(3)[::-1]]).T, dtype=F)
        self.dwi, self.mask = np.ones(8 * 7, F), np.ones(8, np.uint8)


def _calls(L, x, device):
    """name -> (call, outputs): the sequence of the concurrency test on `device`, every call with output arrays of its own"""
    bits = int(np.array([-1.0], F).view(np.int32)[0])
    seq = []
    for interp in (0, 1):
        o = np.zeros((5,) + LARGE[::-1], F)
        seq.append(("vol_xform %d" % interp, lambda o=o, interp=interp: L.fib_vol_xform(
            device, x.out2in, x.frames.ctypes.data, *SMALL, 5, interp, bits, o.ctypes.data, *LARGE), [o]))
    for interp in (0, 1):
        o = np.zeros((5,) + LARGE[::-1], F)
        seq.append(("warp_volume %d" % interp, lambda o=o, interp=interp: L.fib_warp_volume(
            device, x.field.ctypes.data, *FSHAPE, *x.vol_mats, x.frames.ctypes.data, *SMALL, 5, interp, bits, o.ctypes.data, *LARGE), [o]))
    po = np.zeros_like(x.points)
    seq.append(("warp_points", lambda: L.fib_warp_points(device, x.field.ctypes.data, *FSHAPE, *x.pt_mats, x.points.ctypes.data, po.ctypes.data, 300), [po]))
    inv, err = np.zeros((3,) + OSHAPE[::-1], F), np.zeros(OSHAPE[::-1], F)
    seq.append(("warp_invert", lambda: L.fib_warp_invert(device, x.field.ctypes.data, *FSHAPE, *x.inv_mats, 20, inv.ctypes.data, err.ctypes.data, *OSHAPE),
                [inv, err]))
    rvec, rval = np.zeros(9 * x.st_vol.size, F), np.zeros(3 * x.st_vol.size, F)
    seq.append(("st_recon", lambda: L.fib_st_recon(device, x.st_vol.ctypes.data, 12, 10, 9, 1.0, 1.0, rvec.ctypes.data, rval.ctypes.data), [rvec, rval]))
    evec, eval_ = np.zeros(9 * 500, F), np.zeros(3 * 500, F)
    seq.append(("st_eigen", lambda: L.fib_st_eigen(device, x.S_ptrs, 500, evec.ctypes.data, eval_.ctypes.data), [evec, eval_]))
    top, nv = np.zeros((3, 64), np.int32), np.zeros(64, np.int32)
    seq.append(("find_peaks", lambda: L.fib_find_peaks(device, x.odf.ctypes.data, 64, x.verts.ctypes.data, x.verts.shape[0], x.faces.ctypes.data,
                                                       x.faces.shape[0], top.ctypes.data, nv.ctypes.data), [top, nv]))
    pk, isort, nv2 = np.zeros((x.nvert, 64), F), np.zeros((x.nvert, 64), np.int32), np.zeros(64, np.int32)
    seq.append(("find_peaks_work", lambda: L.fib_find_peaks_work(device, x.odf.ctypes.data, 64, x.verts.ctypes.data, x.verts.shape[0], x.faces.ctypes.data,
                                                                 x.faces.shape[0], pk.ctypes.data, isort.ctypes.data, nv2.ctypes.data), [pk, isort, nv2]))
    return seq


def _rumba(L, x, device):
    from fibers_jl_amd import _lib
    keep = [np.zeros(8 * x.nvert, F)] + [np.zeros(8, F) for _ in range(4)] + [np.zeros(24, F) for _ in range(5)]
    out = _lib.RumbaOut(*[a.ctypes.data for a in keep[:5]], (C.c_void_p * 5)(*[a.ctypes.data for a in keep[5:]]))
    sm, ss = C.c_float(0), C.c_float(0)
    rc = L.fib_rumba_rec(device, x.dwi.ctypes.data, 2, 2, 2, 7, x.mask.ctypes.data, 0, x.bval.ctypes.data, x.bvec.ctypes.data, x.verts.ctypes.data,
                         x.verts.shape[0], 2, 1.7e-3, 0.2e-3, 3.0e-3, 0.8e-4, 1, 0, 1, 0, C.byref(out), C.byref(sm), C.byref(ss))
    return rc, keep


@pytest.fixture(scope="module")
def inputs(fj):
    return Inputs(fj)


def test_device_all_and_an_index_out_of_range(fj, inputs):
    """The five forms with a sentence of their own refuse FIB_DEVICE_ALL with it; fib_st_eigen, fib_rumba_rec and the peak finders answer
    it as a device index that does not exist.  An index past the last device is FIB_ERR_NO_DEVICE everywhere.  Nothing is written."""
    L = fj.lib()
    n = L.fib_device_count()
    assert n >= 1
    own = {"vol_xform": b"vol_xform", "warp_volume": b"warp_volume", "warp_points": b"warp_points", "warp_invert": b"warp_invert",
           "st_recon": b"st_recon"}
    for device in (fj.DEVICE_ALL, n + 3):
        range_msg = b"device %d out of range [0,%d)" % (device, n)
        calls = _calls(L, inputs, device)
        assert len(calls) == 10
        for name, call, outs in calls:
            rc, err = call(), L.fib_last_error()
            form = name.split()[0]
            if device == fj.DEVICE_ALL and form in own:
                assert rc == UNSUPPORTED and err == own[form] + b" runs on one device (FIB_DEVICE_ALL is not supported)", (name, rc, err)
            else:
                assert rc == NO_DEVICE and err == range_msg, (name, device, rc, err)
            assert not any(o.any() for o in outs), name
        rc, keep = _rumba(L, inputs, device)
        err = L.fib_last_error()
        assert rc == NO_DEVICE and err == range_msg, (device, rc, err)
        assert not any(a.any() for a in keep)


def test_two_threads_on_one_device(fj, inputs, monkeypatch):
    """Every chunked form cut into several chunks; one call of each alone, then two threads that each make the same calls three times
    while the main thread calls fib_trim: every call returns FIB_OK with the bytes of the call made alone."""
    for k, v in (("FIBERS_VOL_XFORM_FRAMES", "1"), ("FIBERS_WARP_FRAMES", "2"), ("FIBERS_ST_RECON_SLAB", "2"), ("FIBERS_WARP_POINTS", "7")):
        monkeypatch.setenv(k, v)
    L = fj.lib()
    solo = {}
    for name, call, outs in _calls(L, inputs, 0):
        assert call() == 0, (name, L.fib_last_error())
        solo[name] = [o.tobytes() for o in outs]
        assert any(o.any() for o in outs), name
    bad = [[], []]

    def worker(t):
        for rep in range(3):
            for name, call, outs in _calls(L, inputs, 0):
                rc = call()
                if rc != 0:
                    bad[t].append((rep, name, rc, L.fib_last_error()))
                elif [o.tobytes() for o in outs] != solo[name]:
                    bad[t].append((rep, name, "bytes differ from the call made alone"))

    threads = [threading.Thread(target=worker, args=(t,)) for t in range(2)]
    for th in threads:
        th.start()
    assert L.fib_trim() == 0
    for th in threads:
        th.join(120.0)
    assert not any(th.is_alive() for th in threads), "a host form never came back"
    assert bad == [[], []]
