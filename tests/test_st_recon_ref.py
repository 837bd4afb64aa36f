"""CPU tests (no GPU) of st_recon: the float64 restatement the GPU tests compare against (tests/st_recon_ref.py), and the C entry
points' argument checks, which come back before any device call."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import st_recon_ref as ref  # noqa: E402

FIB_ERR_INVALID, FIB_ERR_UNSUPPORTED = -1, -7


def test_reflect_index_is_numpy_reflect_padding():
    for n in (1, 2, 3, 7):
        for r in (1, 3, 9):
            a = np.arange(n, dtype=np.float64) + 1.0
            want = np.pad(a, r, mode="reflect")
            got = a[ref.reflect_index(np.arange(-r, n + r), n)]
            assert np.array_equal(got, want), (n, r)


def test_restatement_matches_scipy_mirror():
    ndimage = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(5)
    for shape in ((1, 5, 4), (2, 3, 9), (6, 1, 2), (4, 7, 3)):
        a = rng.normal(size=shape)
        for w in (ref.gaussian_taps(1.0), ref.gaussian_taps(2.0), ref.SCHARR_D, ref.SCHARR_S):   # radius 4 > several axes here
            for axis in range(3):
                want = ndimage.correlate1d(a, w, axis=axis, mode="mirror")
                np.testing.assert_allclose(ref.correlate1d(a, w, axis), want, rtol=1e-12, atol=1e-12)
        # the whole pipeline's first stage: one Gaussian per axis, as scipy.ndimage.correlate with the outer-product kernel
        w = ref.gaussian_taps(1.5)
        want = a
        for axis in range(3):
            want = ndimage.correlate1d(want, w, axis=axis, mode="mirror")
        np.testing.assert_allclose(ref.separable(a, [w] * 3), want, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("s", [0.5, 1.0, 1.5, 2.0, 3.7])
def test_gaussian_taps(s):
    w = ref.gaussian_taps(s)
    assert len(w) == 4 * math.ceil(s) + 1
    assert abs(w.sum() - 1.0) < 1e-14
    assert np.array_equal(w, w[::-1]) and w.argmax() == len(w) // 2
    x = np.arange(len(w)) - len(w) // 2
    np.testing.assert_allclose(w / w[len(w) // 2], np.exp(-x * x / (2 * s * s)), rtol=1e-14)


@pytest.mark.parametrize("sigma,rho", [(0, 0), (1, 0), (0, 2), (1, 2)])
def test_ramp_known_answer(sigma, rho):
    """vol = a x + b y + c z: away from the faces the gradient is g = (a, b, c) exactly, S = g g^T, eigenvalues (0, 0, |g|^2) and
    the top eigenvector +-g/|g|"""
    g = np.array([0.7, -1.3, 0.4])
    shape = (18, 19, 20)
    x, y, z = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")
    vol = g[0] * x + g[1] * y + g[2] * z
    vec, val, S = ref.st_recon(vol, sigma, rho)
    H = ref.radius(sigma) + 1 + ref.radius(rho)
    inner = tuple(slice(H, n - H) for n in shape)
    assert val[inner].size > 0
    gg = g @ g
    np.testing.assert_allclose(val[inner], np.broadcast_to([0.0, 0.0, gg], val[inner].shape), atol=1e-12 * gg)
    cos = np.abs(vec[inner][..., :, 2] @ (g / np.sqrt(gg)))
    np.testing.assert_allclose(cos, 1.0, atol=1e-12)
    # the faces see the reflection: the gradient across a face vanishes at the edge voxel
    gx, _, _ = ref.gradients(vol, sigma)
    assert np.allclose(gx[0], 0.0) and np.allclose(gx[-1], 0.0)


def test_fib_st_recon_argument_errors_need_no_device(fj):
    L = fj.lib()
    vol = np.zeros((4, 4, 4), np.float32, order="F")
    ev = np.zeros((4, 4, 4, 3, 3), np.float32, order="F")
    ew = np.zeros((4, 4, 4, 3), np.float32, order="F")
    assert L.fib_st_recon(0, None, 4, 4, 4, 1.0, 2.0, ev.ctypes.data, ew.ctypes.data) == FIB_ERR_INVALID
    assert L.fib_st_recon(0, vol.ctypes.data, 4, 4, 4, 1.0, 2.0, None, ew.ctypes.data) == FIB_ERR_INVALID
    assert L.fib_st_recon(0, vol.ctypes.data, 0, 4, 4, 1.0, 2.0, ev.ctypes.data, ew.ctypes.data) == FIB_ERR_INVALID
    assert L.fib_st_recon(0, vol.ctypes.data, 4, -1, 4, 1.0, 2.0, ev.ctypes.data, ew.ctypes.data) == FIB_ERR_INVALID
    assert L.fib_st_recon(0, vol.ctypes.data, 4, 4, 4, 9.0, 2.0, ev.ctypes.data, ew.ctypes.data) == FIB_ERR_UNSUPPORTED
    assert b"at most 16" in L.fib_last_error()
    assert L.fib_st_recon(0, vol.ctypes.data, 4, 4, 4, 1.0, 8.5, ev.ctypes.data, ew.ctypes.data) == FIB_ERR_UNSUPPORTED
    assert L.fib_st_recon(fj.DEVICE_ALL, vol.ctypes.data, 4, 4, 4, 1.0, 2.0, ev.ctypes.data, ew.ctypes.data) == FIB_ERR_UNSUPPORTED
    # the device form checks its arguments before touching the device, too
    assert L.fibd_st_recon(None, 4, 4, 4, 0, 4, 0, 4, 1.0, 2.0, None, None, None, None, 0, None) == FIB_ERR_INVALID


def test_halo_and_work_size(fj):
    for sigma, rho in ((0, 0), (1, 0), (0, 2), (1, 2), (1.5, 3), (8, 8)):
        assert fj.st_recon_halo(sigma, rho) == ref.radius(sigma) + 1 + ref.radius(rho)
    with pytest.raises(fj.FibersError) as e:
        fj.st_recon_halo(8.01, 1)
    assert e.value.code == FIB_ERR_UNSUPPORTED
    n = C.c_uint64()
    assert fj.lib().fibd_st_recon_work_size(10, 20, 5, 1.0, 3.0, C.byref(n)) == 0
    assert n.value == 12 * 10 * 20 * (5 + 2 * 6)
