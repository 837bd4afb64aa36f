"""Plan constructors and destructors hold no device memory they should not (csrc/common.h: fib::upload / fib::zeroed /
fib::plan_destroy, one std::unique_ptr per constructor), through the raw C ABI.

1. each of the seven constructors, created and destroyed N times, leaves a library whose next plan has bit-identical tables;
2. a GQI plan on sphere_642 with 64 frames whose face table names vertex 0 is refused by host_neighbours AFTER finish_plan has put the
   split image, Gdev, the extra row and the fused image on the device: N refusals, each -1 "references vertex" with a NULL handle,
   and a valid creation afterwards succeeds;
3. the free device memory (torch.cuda.mem_get_info after a synchronize) drops over each loop by less than one eighth of what N leaked
   plans would hold.  What a leaked plan holds is computed below from odf.hip's formulas for the ODF plans created with an explicit
   fp16x2 format (ntile_m * stages * pieces * 512 * 2 bytes per image, gM * gK * 4 for Gdev); the DTI / DKI / CSD / RUMBA / cone plans
   and every small table are left out, so the bound is a lower one.

Measured with N = 64 on the commit before the constructors were rewritten (which freed by hand on both paths, so its figures are
the noise of the allocator and the machine): loop 1 dropped by 0 bytes, loop 2 by 0 bytes.  N leaked plans would hold 14 296 064 bytes
(loop 1: 39 056 per GQI plan, 184 320 per DSI plan) and 15 745 024 bytes (loop 2: 246 016 per half-built plan); an eighth of either is
more than four times the noise.  (fib_prob_plan has no table getter: it is created and destroyed only.)"""
import ctypes as C

import numpy as np
import pytest

import dki_ref

pytestmark = pytest.mark.gpu

N = 64
KT = 16                                                   # frames per stage of the contraction (odf.hip)
FP16X2 = 1                                                # FIB_ODF_FORMAT_FP16X2: two pieces per element


def _tile(M):
    """finish_plan's choice of (MB, NX, ntile_m) for M rows of a split-format plan"""
    best = None
    for mb in range(10, 4, -1):
        for nx in (0, 1):
            rows = mb * 32 + nx
            nt = -(-M // rows)
            cost = nt * (64 * mb + 4 * nx)
            if best is None or cost < best[0]:
                best = (cost, mb, nx, nt)
    return best[1:]


def _image_bytes(M, K):
    mb, nx, nt = _tile(M)
    stages = -(-K // KT)
    assert stages >= 2 and nt * nx * stages * KT <= 2048   # (else the plan has no split image and this test's bound would be void)
    return nt * stages * 2 * mb * 512 * 2


def _f(a):
    return np.asfortranarray(a, dtype=np.float32)


class _Kinds:
    """the seven constructors on sphere_362: name -> (create(handle) -> rc, destroy, tables(handle) -> list of arrays or None)"""

    def __init__(self, fj):
        from fibers_jl_amd import _lib, phantom
        L = self.L = fj.lib()
        s = fj.sphere_362
        v, fc = _f(s.vertices), np.asfortranarray(s.faces, dtype=np.int32)
        nv = s.nvert
        U = np.ascontiguousarray(s.vertices[:nv], np.float32)
        b7, g7 = phantom.scheme_dti(6, 1)
        b22, g22 = dki_ref.scheme(22)
        b34, g34 = dki_ref.shells_scheme(4, (30,), (3000.0,), 5, b0=5.0)
        b20, g20 = dki_ref.shells_scheme(1, (19,), (1000.0,), 3)
        bd, gd = phantom.scheme_dsi(r2max=16)
        g7, g22, g34, g20, gd = (_f(g) for g in (g7, g22, g34, g20, gd))
        self.nvert, self.n20, self.nd = nv, len(b20), len(bd)
        self.keep = (v, fc, U, b7, g7, b22, g22, b34, g34, b20, g20, bd, gd)
        csdp = _lib.CsdParams(4, 1.7e-3, 0.3e-3, 1000.0, 50.0, 0.0, 0.05, 1.0, 0.1, 50)
        vp, nvs, fp, nf = v.ctypes.data, v.shape[0], fc.ctypes.data, fc.shape[0]

        def dti_tables(n, np_):
            def get(h):
                A, pA = np.zeros((n, np_), np.float32, order="F"), np.zeros((np_, n), np.float32, order="F")
                assert L.fib_dti_plan_tables(h, A.ctypes.data, pA.ctypes.data, None) == 0
                return [A, pA]
            return get

        def dki_tables(h):
            A, pA = np.zeros((22, 22), np.float32, order="F"), np.zeros((22, 22), np.float32, order="F")
            dirs = np.zeros((nv, 21), np.float32)
            assert L.fib_dki_plan_tables(h, A.ctypes.data, pA.ctypes.data, dirs.ctypes.data) == 0
            return [A, pA, dirs]

        def csd_tables(h):
            ns = C.c_int(0)
            assert L.fib_csd_plan_tables(h, None, C.byref(ns), None, None, None, None) == 0
            assert ns.value == 30
            fr, R = np.zeros(30, np.int32), np.zeros(3, np.float32)
            X, B, Y = (np.zeros((r, 15), np.float32, order="F") for r in (30, nv, nv))
            assert L.fib_csd_plan_tables(h, fr.ctypes.data, None, R.ctypes.data, X.ctypes.data, B.ctypes.data, Y.ctypes.data) == 0
            return [fr, R, X, B, Y]

        def rumba_tables(h):
            nd, nc = C.c_int(0), C.c_int(0)
            assert L.fib_rumba_plan_kernel(h, None, C.byref(nd), C.byref(nc)) == 0
            K = np.zeros((nd.value, nc.value), np.float32, order="F")
            assert L.fib_rumba_plan_kernel(h, K.ctypes.data, None, None) == 0
            return [K]

        def odf_tables(h):
            nr, nvol, nvt = C.c_int(0), C.c_int(0), C.c_int(0)
            assert L.fib_odf_plan_matrix(h, None, C.byref(nr), C.byref(nvol), C.byref(nvt)) == 0
            A = np.zeros((nr.value, nvol.value), np.float32, order="F")
            assert L.fib_odf_plan_matrix(h, A.ctypes.data, None, None, None) == 0
            return [A, np.array([nr.value, nvol.value, nvt.value])]

        self.kinds = {
            "dti": (lambda h: L.fib_dti_plan_create(0, b7.ctypes.data, g7.ctypes.data, 7, h), L.fib_dti_plan_destroy, dti_tables(7, 7)),
            "adc": (lambda h: L.fib_dti_plan_create(0, b7.ctypes.data, None, 7, h), L.fib_dti_plan_destroy, dti_tables(7, 2)),
            "dki": (lambda h: L.fib_dki_plan_create(0, b22.ctypes.data, g22.ctypes.data, 22, vp, nvs, None, h), L.fib_dki_plan_destroy, dki_tables),
            "csd": (lambda h: L.fib_csd_plan_create(0, b34.ctypes.data, g34.ctypes.data, 34, vp, nvs, fp, nf, C.byref(csdp), h),
                    L.fib_csd_plan_destroy, csd_tables),
            "rumba": (lambda h: L.fib_rumba_plan_create(0, b20.ctypes.data, g20.ctypes.data, 20, vp, nvs, 1.7e-3, 0.2e-3, 3.0e-3, 0.8e-4, h),
                      L.fib_rumba_plan_destroy, rumba_tables),
            "gqi": (lambda h: L.fib_gqi_plan_create_fmt(0, b20.ctypes.data, g20.ctypes.data, 20, vp, nvs, fp, nf, 1.25, FP16X2, h),
                    L.fib_odf_plan_destroy, odf_tables),
            "dsi": (lambda h: L.fib_dsi_plan_create_fmt(0, bd.ctypes.data, gd.ctypes.data, len(bd), vp, nvs, fp, nf, 32, FP16X2, h),
                    L.fib_odf_plan_destroy, odf_tables),
            "prob": (lambda h: L.fib_prob_plan_create(0, U.ctypes.data, nv, 0.7071, h), L.fib_prob_plan_destroy, None),
        }

    def make(self, name):
        create, destroy, tables = self.kinds[name]
        h = C.c_void_p()
        rc = create(C.byref(h))
        assert rc == 0 and h.value, (name, rc, self.L.fib_last_error())
        out = tables(h) if tables else None
        destroy(h)
        return out

    def cycle(self, name):
        create, destroy, _ = self.kinds[name]
        h = C.c_void_p()
        assert create(C.byref(h)) == 0 and h.value, (name, self.L.fib_last_error())
        destroy(h)


def _free():
    import torch
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0]


def test_plans_come_and_go_without_holding_device_memory(fj):
    from fibers_jl_amd import phantom
    k = _Kinds(fj)
    L = k.L
    assert L.fib_odf_default_format() > 0                                      # (the library is up before anything is measured)
    first = {name: k.make(name) for name in k.kinds}

    # ---- 1. success pairs ----
    nrep = (k.nd + 1) // 2                                                     # a symmetric lattice folds onto the origin + one of each pair
    leak1 = N * (_image_bytes(k.nvert, k.n20) + k.nvert * k.n20 * 4 + _image_bytes(nrep + k.nvert, nrep))
    free0 = _free()
    for _ in range(N):
        for name in k.kinds:
            k.cycle(name)
    drop1 = free0 - _free()
    for name in k.kinds:
        again = k.make(name)
        if first[name] is not None:
            assert len(again) == len(first[name])
            for a, b in zip(first[name], again):
                assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes(order="A") == b.tobytes(order="A"), name

    # ---- 2. refused after the device holds something ----
    s = fj.sphere_642
    v, fc = _f(s.vertices), np.asfortranarray(s.faces, dtype=np.int32)
    bad = fc.copy(order="F")
    bad[fc.shape[0] // 2, 1] = 0
    b64, g64 = phantom.scheme_gqi(4, 20, (1000.0, 2000.0, 3000.0), 3)
    g64 = _f(g64)
    assert len(b64) == 64 and _tile(s.nvert) == (10, 1, 1)                     # the fused shape: two images
    img = _image_bytes(s.nvert, 64)
    leak2 = N * (2 * img + s.nvert * 64 * 4)

    def gqi642(faces, h):
        return L.fib_gqi_plan_create_fmt(0, b64.ctypes.data, g64.ctypes.data, 64, v.ctypes.data, v.shape[0], faces.ctypes.data,
                                         faces.shape[0], 1.25, FP16X2, C.byref(h))
    free1 = _free()
    for _ in range(N):
        h = C.c_void_p(1)
        assert gqi642(bad, h) == -1
        assert h.value is None
        assert b"references vertex" in L.fib_last_error()
    drop2 = free1 - _free()
    h = C.c_void_p()
    assert gqi642(fc, h) == 0 and h.value, L.fib_last_error()
    L.fib_odf_plan_destroy(h)

    # ---- 3. nothing leaked ----
    print("plan lifecycle: N = %d, loop 1 dropped %d of %d bytes a leak would hold, loop 2 %d of %d" % (N, drop1, leak1, drop2, leak2))
    assert drop1 < leak1 // 8, (drop1, leak1)
    assert drop2 < leak2 // 8, (drop2, leak2)
