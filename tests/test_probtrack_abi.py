"""CPU tests (no GPU) of the probabilistic-tracking entries: they are exported and bound, the parts that need no device answer, and the
refusals come before any device is touched."""
import ctypes as C

import numpy as np
import pytest

NAMES = ("fib_prob_row_pitch", "fibd_prob_table", "fib_prob_plan_create", "fib_prob_plan_destroy", "fibd_prob_work_size", "fibd_prob_run",
         "fib_prob_stream")


def test_entries_are_exported_and_bound(fj):
    from fibers_jl_amd import _lib
    L = C.CDLL(_lib.LIB_PATH)
    for n in NAMES:
        assert hasattr(L, n) and n in _lib._PROTOS, n
    for n in ("ProbPlan", "prob_stream", "prob_row_pitch", "prob_work_size"):
        assert hasattr(fj, n), n
    for n in ("prob_stream_device", "prob_table_device"):        # the device tier, through the module
        assert hasattr(fj.probtrack, n), n


def test_row_pitch_and_work_size(fj):
    assert [fj.prob_row_pitch(n) for n in (1, 64, 65, 181, 321, 362, 512)] == [64, 64, 128, 192, 384, 384, 512]
    for n in (0, -3, 513):
        with pytest.raises(ValueError):
            fj.prob_row_pitch(n)
    # 24 bytes per line, the two totals and one pair of block totals per 1024 lines; 8-byte aligned; monotone
    assert fj.prob_work_size(0) == 24 + 16 + 16 and fj.prob_work_size(1024) == 24 * 1024 + 16 + 16 and fj.prob_work_size(1025) == 24 * 1025 + 16 + 32
    assert all(fj.prob_work_size(n) % 8 == 0 for n in (1, 7, 1000, 10 ** 7))


def test_refusals_need_no_device(fj):
    L = fj.lib()
    U = np.ascontiguousarray(fj.sphere_362.vertices[:181], np.float32)
    h = C.c_void_p()
    assert L.fib_prob_plan_create(0, U.ctypes.data, 181, 0.0, C.byref(h)) == -1 and not h       # 90 degrees
    assert b"below 90" in L.fib_last_error()
    assert L.fib_prob_plan_create(0, U.ctypes.data, 181, float("nan"), C.byref(h)) == -1
    assert L.fib_prob_plan_create(0, U.ctypes.data, 513, 0.7, C.byref(h)) == -7
    assert L.fib_prob_plan_create(0, None, 181, 0.7, C.byref(h)) == -1
    from fibers_jl_amd import _lib
    out = _lib.TractOut()
    odf = np.zeros((2, 2, 2, 181), np.float32, order="F")
    sub = np.zeros((1, 3), np.float32)
    rc = L.fib_prob_stream(_lib.DEVICE_ALL, 2, 2, 2, odf.ctypes.data, 181, U.ctypes.data, None, None, sub.ctypes.data, 1, 3, 8, 0.7, 0.5, 0.1, 1, 0,
                           C.byref(out))
    assert rc == -7 and out.nlines == 0 and not out.xyz
    with pytest.raises(ValueError):
        fj.prob_stream(fj.MRI(np.zeros((2, 2, 2, 180), np.float32)), fj.sphere_362)               # one frame per direction


def test_no_gpu_is_a_loud_error_not_a_fallback(fj):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(fj.FibersError) as e:
        fj.ProbPlan(fj.sphere_362, 45, 0)
    assert e.value.code == -2 and "no CPU fallback" in str(e.value)
    with pytest.raises(fj.FibersError) as e:
        fj.prob_stream(fj.MRI(np.ones((2, 2, 2, 181), np.float32)), fj.sphere_362, sublist=np.zeros((1, 3), np.float32))
    assert e.value.code == -2
