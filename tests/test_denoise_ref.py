"""CPU tests (no GPU) of dwi_denoise: the float64 restatement the GPU tests compare against (tests/denoise_ref.py) -- its two routes
agree, its inputs stay clear of the definition's discontinuities, it estimates the noise level -- and the refusals of the library and
of the Python layer that need no device."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import denoise_ref as ref  # noqa: E402

FIB_ERR_INVALID, FIB_ERR_UNSUPPORTED = -1, -7
CASES = pytest.mark.parametrize("case", ref.CASES, ids=ref.case_id)
ESTS = pytest.mark.parametrize("estimator", ref.ESTIMATORS)


@CASES
@ESTS
def test_the_two_routes_agree(case, estimator):
    """eigh of the Gram matrix against svd of X: equal rank in every voxel; rows within 1e-9 absolute and 5e-12 of the largest sample,
    sigma within 1e-10 relative.  Both routes are backward stable in float64 (2.2e-16 of lambda_max); the rows lose the factor
    lambda_max / gap <= 1e6 that the gap condition below allows to the projector, a few e-10 of a sample of about 1e3 at the very worst,
    and far less where the gap is wide.  sigma^2 is a mean of noise eigenvalues, about sigma^2 q = 4e5 each under a lambda_max of up to
    1e11 (343 x 128 samples of about 1.5e3): eigh's absolute error of 2.2e-16 lambda_max is 6e-11 of them, and half of that in sigma."""
    a, b, d_rows, d_sigma = ref.case_reference(case, estimator)
    print("%s %s: d_rows %.3g (%.3g of max), d_sigma %.3g rel" % (ref.case_id(case), estimator, d_rows, d_rows / np.abs(a["dwi"]).max(),
                                                                     (np.abs(a["sigma"] - b["sigma"]) / a["sigma"]).max()))
    assert np.array_equal(a["rank"], b["rank"])
    assert d_rows <= 1e-9 and d_rows <= 5e-12 * np.abs(a["dwi"]).max()
    assert np.all(np.abs(a["sigma"] - b["sigma"]) <= 1e-10 * a["sigma"])


@CASES
@ESTS
def test_the_inputs_keep_their_distance_from_the_discontinuities(case, estimator):
    """conditions on the inputs, so that no GPU test needs to leave a voxel out: the rule's decision margin >= 1e-4 and the spectral
    gap at the cut >= 1e-6 of lambda_max in every voxel"""
    a = ref.case_reference(case, estimator)[0]
    print("%s %s: margin %.3g gap %.3g" % (ref.case_id(case), estimator, a["margin"].min(), a["gap"].min()))
    assert a["margin"].min() >= 1e-4
    assert a["gap"].min() >= 1e-6


@CASES
@ESTS
def test_sigma_estimates_the_noise_level(case, estimator):
    shape, N, P, k = case
    a = ref.case_reference(case, estimator)[0]
    print("%s %s: mean sigma %.2f (true %.2f), ranks %s" % (ref.case_id(case), estimator, a["sigma"].mean(), ref.SIGMA, np.unique(a["rank"])))
    if N >= 16:
        assert abs(a["sigma"].mean() - ref.SIGMA) <= 0.2 * ref.SIGMA


@pytest.mark.parametrize("case,estimator", ref.LARGE_HELD, ids=lambda v: v if isinstance(v, str) else ref.case_id(v))
def test_the_large_cases_meet_the_same_conditions(case, estimator):
    """the cases above the kernel's 512 persistent workgroups (ref.LARGE_CASES), under the estimators the GPU tests hold them with.
    Equal rank by both routes, the rule's decision margin >= 1e-4 and sigma within 1e-10 relative, as for ref.CASES.  Among a thousand
    patches of 125 rows some spectral gap at the cut is narrower than any in ref.CASES, so the gap is held to 1e-7 of lambda_max here,
    and the rows to what that allows: a backward-stable float64 route perturbs the projector by about eps64 lambda_max / gap <=
    2.2e-16 x 1e7 = 2.2e-9, hence a row by 2.2e-9 of the largest sample.  That is fifty times below the 2^-23 = 1.2e-7 of one rounding
    to float32, the other term of the GPU tests' tolerance, so the routes' disagreement d decides no GPU comparison.  More than one
    rank a case: successive tickets of a workgroup then cut at different places."""
    shape, N, P, k = case
    a, b, d_rows, d_sigma = ref.case_reference(case, estimator)
    print("%s %s: d_rows %.3g (%.3g of max), d_sigma %.3g rel, margin %.3g, gap %.3g, mean sigma %.2f, ranks %s" % (
        ref.case_id(case), estimator, d_rows, d_rows / np.abs(a["dwi"]).max(), (np.abs(a["sigma"] - b["sigma"]) / a["sigma"]).max(),
        a["margin"].min(), a["gap"].min(), a["sigma"].mean(), np.unique(a["rank"])))
    assert int(np.prod(shape)) > 2 * 512
    assert np.array_equal(a["rank"], b["rank"]) and len(np.unique(a["rank"])) >= 2
    assert a["margin"].min() >= 1e-4 and a["gap"].min() >= 1e-7
    assert d_rows <= 2.2e-9 * np.abs(a["dwi"]).max()
    assert np.all(np.abs(a["sigma"] - b["sigma"]) <= 1e-10 * a["sigma"])
    assert abs(a["sigma"].mean() - ref.SIGMA) <= 0.2 * ref.SIGMA


@pytest.mark.parametrize("route", ["eigh", "svd"])
@ESTS
def test_an_all_zero_volume(route, estimator):
    for shape, N, P in (((4, 3, 3), 5, 3), ((3, 4, 3), 40, 3)):
        o = ref.denoise(np.zeros(shape + (N,), np.float32), P, estimator, route)
        assert not o["dwi"].any() and not o["sigma"].any() and np.all(o["rank"] == min(P ** 3, N))


def test_the_patch_is_the_nearest_block_inside_the_volume():
    assert [ref.patch_start(v, 7, 5) for v in range(7)] == [0, 0, 0, 1, 2, 2, 2]
    assert [ref.patch_start(v, 3, 3) for v in range(3)] == [0, 0, 0]
    # a mask changes nothing inside it: the patch reads every voxel
    case = ref.CASES[0]
    vol = ref.case_volume(case)
    m = np.zeros(vol.shape[:3], bool)
    m[::2, 1::2, :] = True
    full, part = ref.case_reference(case, "exp2")[0], ref.denoise(vol, case[2], "exp2", "eigh", mask=m)
    assert np.array_equal(part["dwi"][m], full["dwi"][m]) and not part["dwi"][~m].any() and not part["rank"][~m].any()


REFUSALS = [((6, 5, 4), 16, 4, "exp2", FIB_ERR_INVALID, "patch edge must be 3, 5 or 7"),
            ((6, 5, 4), 16, 5, "exp2", FIB_ERR_INVALID, "must be at least the patch edge 5"),
            ((2, 5, 4), 16, 3, "exp1", FIB_ERR_INVALID, "must be at least the patch edge 3"),
            ((6, 5, 4), 1, 3, "exp2", FIB_ERR_INVALID, "at least 2 frames"),
            ((8, 7, 7), 129, 7, "exp2", FIB_ERR_UNSUPPORTED, "P = 7 with N = 129 frames")]


@pytest.mark.parametrize("shape,N,P,est,code,msg", REFUSALS)
def test_refusals_need_no_device(fj, shape, N, P, est, code, msg):
    """by the library's own message, through the check every entry shares"""
    with pytest.raises(fj.FibersError) as e:
        fj.denoise.dwi_denoise_check(shape, N, P, est)
    assert e.value.code == code and msg in str(e.value), str(e.value)
    if code == FIB_ERR_UNSUPPORTED:
        assert "128" in str(e.value)
    # the host form refuses with the same sentence before it looks for a device
    vol = np.zeros(shape + (N,), np.float32, order="F")
    with pytest.raises(fj.FibersError) as e:
        fj.dwi_denoise(fj.MRI(vol), patch=P, estimator=est)
    assert e.value.code == code and msg in str(e.value), str(e.value)


def test_the_python_layer_and_the_limits(fj):
    import ctypes as C
    fj.denoise.dwi_denoise_check((8, 7, 7), 128, 7)                       # the limit itself is served
    fj.denoise.dwi_denoise_check((5, 5, 5), 100000, 5)                    # P = 5 serves any N
    with pytest.raises(ValueError, match="estimator"):
        fj.dwi_denoise(fj.MRI(np.zeros((3, 3, 3, 4), np.float32)), estimator="mp")
    with pytest.raises(ValueError, match="mask of shape"):
        fj.dwi_denoise(fj.MRI(np.zeros((3, 3, 3, 4), np.float32)), mask=np.ones((3, 3, 4), np.uint8))
    L = fj.lib()
    z = np.zeros(27 * 4, np.float32)
    m = np.ones(27, np.uint8)
    args = [z.ctypes.data, 3, 3, 3, 4, m.ctypes.data, 3, 2, z.ctypes.data, z.ctypes.data, z.ctypes.data]
    assert L.fib_dwi_denoise(fj.DEVICE_ALL, *args) == FIB_ERR_UNSUPPORTED and b"dwi_denoise runs on one device" in L.fib_last_error()
    assert L.fib_dwi_denoise(0, None, *args[1:]) == FIB_ERR_INVALID and b"NULL argument" in L.fib_last_error()
    assert L.fib_dwi_denoise(0, *args[:7], 3, *args[8:]) == FIB_ERR_INVALID and b"unknown estimator 3" in L.fib_last_error()
    # the workspace is sized by the cap and the workgroups, not by the volume
    nb = [C.c_uint64() for _ in range(3)]
    for b, (nx, ny, nz) in zip(nb, ((40, 40, 40), (140, 140, 140), (8, 8, 8))):
        assert L.fibd_dwi_denoise_work_size(nx, ny, nz, 270, 5, C.byref(b)) == 0
    assert nb[0].value == nb[1].value == 256 + 512 * 24 * 125 * 63 * 8 and nb[2].value == nb[0].value
    assert L.fibd_dwi_denoise_work_size(8, 8, 8, 129, 7, C.byref(nb[0])) == FIB_ERR_UNSUPPORTED
    assert not hasattr(fj, "dwi_denoise_device") and hasattr(fj.denoise, "dwi_denoise_device")     # the device tier, through the module
    assert fj.Denoised is fj.denoise.Denoised
