"""dwi_degibbs on the GPU against the float64 restatement (tests/degibbs_ref.py): every case through the device tier and through
fib_dwi_degibbs, held to |gpu - ref64| <= 4 d + 2^-23 |ref64| in every pixel (d: the case's own difference between the restatement's two
routes; the second term is the one rounding to float32) and to the restatement's j* wherever its gap exceeds 64 e_t -- which
tests/test_degibbs_ref.py shows to be everywhere, and this file asserts; chunks, determinism, a non-finite slice, the workspace and
argument contracts, the refusals, and the tensor fit of the unrung series end to end."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import degibbs_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = pytest.mark.parametrize("case", ref.CASES, ids=ref.case_id)
MID = ref.CASES[3]                    # 15x14x2, N = 3
AX0, AX1 = ref.CASES[6], ref.CASES[7]


def _planar(vol):
    """host [nx,ny,nz,N] -> device [N, nvox]"""
    import torch
    N = vol.shape[3]
    return torch.from_numpy(np.array(vol.reshape(-1, N, order="F").T, order="C")).cuda()     # (a copy: the shared volumes are read-only)


def _host(t, shape):
    """device [N, nvox] -> host [nx,ny,nz,N]"""
    a = t.cpu().numpy()
    return a.T.reshape(tuple(shape) + (a.shape[0],), order="F")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _kw(case):
    _, _, axis, K, minW, maxW, _ = case
    return dict(slice_axis=axis, nshifts=K, min_w=minW, max_w=maxW)


def _device(fj, vol, shifts=True, **kw):
    import torch
    shape = vol.shape[:3]
    o = fj.degibbs.dwi_degibbs_device(_planar(vol), shape, shifts=shifts, **kw)
    torch.cuda.synchronize()
    return tuple(_host(o[k], shape) for k in (("dwi", "shift_u", "shift_v") if shifts else ("dwi",)))


def _host_form(fj, vol, **kw):
    r = fj.dwi_degibbs(fj.MRI(vol), shifts=True, **kw)
    return r.dwi.vol, r.shift_u.vol, r.shift_v.vol


def _hold_values(dwi, r, what):
    err, tol = np.abs(dwi.astype(np.float64) - r["out"]), 4 * r["d"] + 2.0 ** -23 * np.abs(r["out"])
    print("%s: values %.3g of the tolerance (d %.3g)" % (what, (err / np.maximum(tol, 1e-300)).max(), r["d"]))
    assert np.all(err <= tol)


def _hold(got, case):
    dwi, su, sv = got
    r = ref.case_reference(case)
    for s, j, gap, name in ((su, r["ju"], r["gap_u"], "shift_u"), (sv, r["jv"], r["gap_v"], "shift_v")):
        held = gap > 64 * r["e_t"]
        out = 1.0 - held.mean()
        print("%s %s: %d of %d pixels differ, share left out %.3g" % (ref.case_id(case), name, np.count_nonzero(s != j), s.size, out))
        assert out == 0.0, "the gap rule leaves pixels of a phantom case out"
        assert np.array_equal(s[held], j[held]), "%s differs in %d pixels" % (name, np.count_nonzero(s[held] != j[held]))
    _hold_values(dwi, r, ref.case_id(case))


@CASES
def test_device_tier_matches_restatement(fj, case):
    _hold(_device(fj, ref.case_volume(case), **_kw(case)), case)


@CASES
def test_host_form_matches_restatement(fj, case):
    _hold(_host_form(fj, ref.case_volume(case), **_kw(case)), case)


@functools.lru_cache(maxsize=None)
def _flat(axis):
    """frame 0 all zero, frame 1 constant, slices across `axis`; and the restatement of it"""
    vol = np.zeros((10, 9, 12, 2), np.float32, order="F")
    vol[..., 1] = 417.25
    return vol, ref.degibbs(vol, axis)


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_zero_and_constant_slices(fj, axis):
    """only the value rule applies (every candidate ties on such a slice); the zero slice comes back as exact zeros with j* = 0"""
    vol, r = _flat(axis)
    for got in (_device(fj, vol, slice_axis=axis), _host_form(fj, vol, slice_axis=axis)):
        _hold_values(got[0], r, "flat-a%d" % axis)
        assert not got[0][..., 0].any() and not got[1][..., 0].any() and not got[2][..., 0].any()
        assert not np.signbit(got[0][..., 0]).any()


def test_two_runs_give_identical_bits(fj):
    a, b = _device(fj, ref.case_volume(MID), **_kw(MID)), _device(fj, ref.case_volume(MID), **_kw(MID))
    for u, v in zip(a, b):
        assert np.array_equal(_bits(u), _bits(v))


@pytest.mark.parametrize("case", [ref.CASES[1], AX0, AX1], ids=ref.case_id)
def test_chunks_of_the_host_form(fj, monkeypatch, case):
    """chunks of 1 slice, 2 slices, one frame, and all slices give the device tier's bits, whichever axis the slices lie across"""
    vol, axis = ref.case_volume(case), case[2]
    ns, N = vol.shape[axis], vol.shape[3]
    dev = _device(fj, vol, **_kw(case))
    for per in (None, 1, 2, ns, ns * N):
        if per is None:
            monkeypatch.delenv("FIBERS_DEGIBBS_SLICES", raising=False)
        else:
            monkeypatch.setenv("FIBERS_DEGIBBS_SLICES", str(per))
        for a, b in zip(dev, _host_form(fj, vol, **_kw(case))):
            assert np.array_equal(_bits(a), _bits(b)), per


@pytest.mark.parametrize("case", [ref.CASES[1], AX0], ids=ref.case_id)
def test_a_non_finite_sample_spoils_its_slice_only(fj, case):
    vol, axis = ref.case_volume(case), case[2]
    clean = _device(fj, vol, **_kw(case))
    for bad in (np.nan, np.inf):
        v = np.array(vol, order="F")
        ix = [4, 4, 4, 1]
        ix[axis] = 1
        v[tuple(ix)] = bad
        got = _device(fj, v, **_kw(case))                    # (FIB_OK: a refusal would have raised)
        keep = np.ones(vol.shape, bool)
        sl = [slice(None)] * 4
        sl[axis], sl[3] = 1, 1
        keep[tuple(sl)] = False
        for a, b in zip(clean, got):
            assert np.array_equal(_bits(a[keep]), _bits(b[keep]))
        r = fj.dwi_degibbs(fj.MRI(v), shifts=True, **_kw(case))
        assert np.array_equal(_bits(r.dwi.vol[keep]), _bits(clean[0][keep]))


def test_the_shift_outputs_do_not_change_the_series(fj):
    vol = ref.case_volume(MID)
    with_s, without = _device(fj, vol, **_kw(MID)), _device(fj, vol, shifts=False, **_kw(MID))
    assert np.array_equal(_bits(with_s[0]), _bits(without[0]))
    r = fj.dwi_degibbs(fj.MRI(vol), **_kw(MID))
    assert r.shift_u is None and r.shift_v is None and np.array_equal(_bits(r.dwi.vol), _bits(with_s[0]))


def test_workspace_contract(fj):
    import torch
    vol = ref.case_volume(MID)
    nx, ny, nz, N = vol.shape
    need = fj.degibbs.dwi_degibbs_work_size(nx, ny, nz, N)
    assert need == fj.dwi_degibbs_work_size(nx, ny, nz, N, **_kw(MID)) and need % 8 == 0
    own = _device(fj, vol)
    exact = _device(fj, vol, work=torch.empty(need, dtype=torch.uint8, device="cuda"))
    for u, v in zip(own, exact):
        assert np.array_equal(_bits(u), _bits(v))
    with pytest.raises(fj._dev.ArgError, match="dwi_degibbs_work_size"):
        _device(fj, vol, work=torch.empty(need - 1, dtype=torch.uint8, device="cuda"))
    with pytest.raises(fj._dev.ArgError, match="work"):
        _device(fj, vol, work=torch.empty(need, dtype=torch.uint8))
    # the C entry refuses a short workspace itself
    d, w = _planar(vol), torch.empty(need // 8 + 1, dtype=torch.int64, device="cuda")
    o = torch.empty(N * nx * ny * nz, dtype=torch.float32, device="cuda")
    rc = fj.lib().fibd_dwi_degibbs(d.data_ptr(), nx, ny, nz, N, None, o.data_ptr(), None, None, w.data_ptr(), need - 1, None)
    assert rc == -1 and b"fibd_dwi_degibbs_work_size" in fj.lib().fib_last_error()
    rc = fj.lib().fibd_dwi_degibbs(d.data_ptr(), nx, ny, nz, N, None, o.data_ptr(), None, None, w.data_ptr() + 4, need, None)
    assert rc == -1 and b"aligned" in fj.lib().fib_last_error()


def test_device_arguments_are_checked_before_a_launch(fj, monkeypatch):
    import torch
    from fibers_jl_amd import _lib
    shape, N = (9, 10, 2), 2
    nvox = 180
    good = torch.zeros((N, nvox), dtype=torch.float32, device="cuda")
    bad = [good.double(), good.cpu(), torch.zeros((N, nvox - 1), dtype=torch.float32, device="cuda"),
           torch.zeros((N, 2 * nvox), dtype=torch.float32, device="cuda")[:, ::2], good.reshape(-1), torch.zeros((0, nvox), dtype=torch.float32, device="cuda")]
    outs = dict(dwi=torch.zeros((N, nvox), dtype=torch.float32, device="cuda"), shift_u=torch.zeros((N, nvox), dtype=torch.int8, device="cuda"),
                shift_v=torch.zeros((N, nvox), dtype=torch.int8, device="cuda"))
    fj.degibbs.dwi_degibbs_device(good, shape, out=outs)                                   # the valid call goes through
    monkeypatch.setattr(_lib, "lib", lambda: pytest.fail("the library was reached with a bad argument"))
    for t in bad:
        with pytest.raises(fj._dev.ArgError):
            fj.degibbs.dwi_degibbs_device(t, shape)
    for k in outs:
        wrong = outs[k].double() if k == "dwi" else outs[k].to(torch.uint8)
        for t in (wrong, outs[k].cpu(), outs[k].reshape(-1)[:-1].clone()):
            with pytest.raises(fj._dev.ArgError):
                fj.degibbs.dwi_degibbs_device(good, shape, out=dict(outs, **{k: t}))
    if torch.cuda.device_count() > 1:
        with pytest.raises(fj._dev.ArgError):
            fj.degibbs.dwi_degibbs_device(good, shape, out=dict(outs, dwi=outs["dwi"].to("cuda:1")))
    with pytest.raises(fj._dev.ArgError, match="in-place"):                                # out aliasing dwi, whole and in part
        fj.degibbs.dwi_degibbs_device(good, shape, out=dict(dwi=good))
    both = torch.zeros(2 * N * nvox - nvox, dtype=torch.float32, device="cuda")
    with pytest.raises(fj._dev.ArgError, match="in-place"):
        fj.degibbs.dwi_degibbs_device(both[:N * nvox].view(N, nvox), shape, out=dict(dwi=both[N * nvox - nvox:].view(N, nvox)))
    with pytest.raises(fj._dev.ArgError, match="positive"):
        fj.degibbs.dwi_degibbs_device(good, (9, 10, 0))


def test_gpu_refusals(fj):
    import torch
    L = ref.LIMIT
    d = torch.zeros((1, (L + 1) * 9), dtype=torch.float32, device="cuda")
    with pytest.raises(fj.FibersError) as e:
        fj.degibbs.dwi_degibbs_device(d, (L + 1, 9, 1))
    assert e.value.code == -7 and str(L) in str(e.value)
    with pytest.raises(fj.FibersError) as e:
        fj.dwi_degibbs(fj.MRI(np.zeros((L + 1, 9, 1, 1), np.float32)))
    assert e.value.code == -7 and str(L) in str(e.value)
    with pytest.raises(fj.FibersError) as e:
        fj.dwi_degibbs(fj.MRI(np.zeros((9, 9, 2, 1), np.float32)), device=fj.DEVICE_ALL)
    assert e.value.code == -7
    with pytest.raises(fj.FibersError) as e:                                               # 15 x 14 is below 2 maxW + 3 at maxW = 6
        fj.dwi_degibbs(fj.MRI(np.zeros((15, 14, 2, 1), np.float32)), min_w=2, max_w=6)
    assert e.value.code == -1
    # out == dwi at the C entries themselves
    g = torch.zeros((1, 162), dtype=torch.float32, device="cuda")
    w = torch.empty(fj.dwi_degibbs_work_size(9, 9, 2, 1) // 8, dtype=torch.int64, device="cuda")
    rc = fj.lib().fibd_dwi_degibbs(g.data_ptr(), 9, 9, 2, 1, None, g.data_ptr(), None, None, w.data_ptr(), w.numel() * 8, None)
    assert rc == -1 and b"overlap" in fj.lib().fib_last_error()
    h = np.zeros((9, 9, 2, 1), np.float32, order="F")
    assert fj.lib().fib_dwi_degibbs(0, h.ctypes.data, 9, 9, 2, 1, None, h.ctypes.data, None, None) == -1
    assert b"overlap" in fj.lib().fib_last_error()


def test_tensor_fit_of_the_unrung_series(fj):
    """dti_fit(dwi_degibbs(dwi_denoise(x).dwi).dwi, mask) with bval / bvec carried through, against dti_fit of the restatement's float32
    output: fa to DESIGN.md §5's DTI tolerance"""
    from fibers_jl_amd import phantom
    shape = (9, 10, 5)
    bval, bvec = phantom.scheme_dti(6, 1)
    vol, _, _ = phantom.make_volume(shape, bval, bvec, seed=11)
    x = fj.MRI(vol, bval, bvec, volres=(2.0, 2.0, 2.5), tr=3.5)
    mask = fj.MRI(np.ones(shape, np.uint8))
    den = fj.dwi_denoise(x, patch=3)
    deg = fj.dwi_degibbs(den.dwi)
    assert np.array_equal(deg.dwi.bval, x.bval) and np.array_equal(deg.dwi.bvec, x.bvec)
    assert deg.dwi.volres == x.volres and deg.dwi.tr == x.tr and np.array_equal(deg.dwi.vox2ras, x.vox2ras)
    got = fj.dti_fit(deg.dwi, mask)
    want = fj.dti_fit(fj.MRI(np.asfortranarray(ref.degibbs(den.dwi.vol)["out"].astype(np.float32)), bval, bvec), mask)
    assert np.isfinite(got.fa.vol).all()
    assert np.allclose(got.fa.vol, want.fa.vol, atol=1e-4)
    assert fj.dwi_mask(deg.dwi).mask.vol.shape[:3] == shape           # and it goes into dwi_mask as it is
