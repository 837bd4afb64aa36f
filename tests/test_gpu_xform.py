"""xfm_apply (util.jl:385-420) and str_xform's .trk body (trk.jl:316-347) on the GPU, bit for bit against the float32 restatement
(tests/xform_ref.py): fibd_xfm_apply (affine and projective matrices, points where an fma-contracted evaluation rounds differently,
in place, tiny counts, a view 12 bytes off, Inf / NaN, a side stream), fib_xfm_apply (host buffers), the row-major matrix order,
and fibd_stream_pack_trk_xfm on the tile and the plain pack paths, down to the file stream_to_trk writes.  In-process only."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import xform_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

AFFINE = np.array([[0.98, -0.17, 0.05, 3.25],
                   [0.16, 0.97, -0.11, -7.5],
                   [-0.07, 0.12, 1.03, 12.125],
                   [0.0, 0.0, 0.0, 1.0]], np.float32)
PROJECTIVE = np.array([[1.1, 0.2, -0.3, 4.0],
                       [-0.25, 0.9, 0.15, -2.0],
                       [0.05, -0.4, 1.2, 0.5],
                       [0.001, -0.002, 0.0015, 1.0]], np.float32)


def _xfm(fj, m, outres=(1.0, 1.0, 1.0)):
    return fj.Xform(insize=(20, 20, 20), outsize=(30, 25, 20), outres=outres, vox2vox=m,
                    outvox2ras=np.array([[0, 0, -1.5, 20], [1.25, 0, 0, -30], [0, 2.0, 0, 5], [0, 0, 0, 1]], np.float32))


def _points(n, seed):
    return (np.random.default_rng(seed).random((n, 3)) * 200.0 - 50.0).astype(np.float32)


def _fma_witnesses(m, k=4096):
    """points whose fma-contracted evaluation differs from the reference's in at least one coordinate"""
    rng = np.random.default_rng(5)
    found = []
    while sum(len(f) for f in found) < k:
        p = (rng.random((1 << 16, 3)) * 300.0 - 100.0).astype(np.float32)
        d = np.any(ref.apply_f32(m, p) != ref.apply_fma(m, p), axis=1)
        found.append(p[d])
    return np.concatenate(found)[:k]


def _bits_equal(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint32), b[~nb].view(np.uint32))


@pytest.mark.parametrize("name", ["affine", "projective"])
def test_device_apply_is_bit_identical_to_the_reference_loop(fj, name):
    import torch
    m = AFFINE if name == "affine" else PROJECTIVE
    wit = _fma_witnesses(m)
    assert not np.array_equal(ref.apply_f32(m, wit), ref.apply_fma(m, wit))          # a contracted kernel cannot pass
    pts = np.concatenate([_points(3_000_000, 1), wit])
    d = torch.from_numpy(pts).cuda()
    out = fj.xfm_apply(_xfm(fj, m), d)
    torch.cuda.synchronize()
    assert _bits_equal(out.cpu().numpy(), ref.apply_f32(m, pts))
    fj.xfm_apply(_xfm(fj, m), d, out=d)                                                 # in place
    torch.cuda.synchronize()
    assert _bits_equal(d.cpu().numpy(), ref.apply_f32(m, pts))


def test_device_apply_small_counts_offsets_and_bounds(fj):
    import torch
    x = _xfm(fj, PROJECTIVE)
    pts = _points(64, 2)
    for n in (0, 1, 2, 3, 5, 7, 8, 9, 13):
        for shift in range(4):                                   # the view starts 0, 1, 2, 3 points into the buffer
            buf = torch.full((3 * (n + 8),), -7.0, device="cuda")
            src = torch.from_numpy(pts[: n + 8].reshape(-1).copy()).cuda()
            buf_in = src[3 * shift: 3 * (shift + n)]
            dst = buf[3 * shift: 3 * (shift + n)]
            fj.xfm_apply(x, buf_in, out=dst)
            torch.cuda.synchronize()
            assert _bits_equal(dst.cpu().numpy(), ref.apply_f32(PROJECTIVE, pts[shift: shift + n]).reshape(-1)), (n, shift)
            rest = torch.cat([buf[: 3 * shift], buf[3 * (shift + n):]])
            assert bool((rest == -7.0).all()), "wrote outside the range (n=%d, shift=%d)" % (n, shift)
    # in place on a view one point (12 bytes) into a large buffer: the vector path after a 3-point head
    big = torch.from_numpy(_points(100_003, 3)).cuda()
    want = ref.apply_f32(PROJECTIVE, big[1:].cpu().numpy())
    v = big[1:]
    fj.xfm_apply(x, v, out=v)
    torch.cuda.synchronize()
    assert _bits_equal(v.cpu().numpy(), want)
    # in and out misaligned against each other (the scalar path)
    src = torch.from_numpy(_points(1001, 4)).cuda()
    dst = torch.empty(3 * 1001 + 1, device="cuda")[1:]                        # 4 bytes off against the source's 12
    fj.xfm_apply(x, src[1:].reshape(-1), out=dst[: 3000])
    torch.cuda.synchronize()
    assert _bits_equal(dst[:3000].cpu().numpy(), ref.apply_f32(PROJECTIVE, src[1:].cpu().numpy()).reshape(-1))


def test_non_finite_inputs_give_nan_triplets_where_the_reference_does(fj):
    import torch
    pts = _points(4096, 6)
    rng = np.random.default_rng(7)
    idx = rng.choice(4096, 300, replace=False)
    pts[idx[:100], rng.integers(0, 3, 100)] = np.inf
    pts[idx[100:200], rng.integers(0, 3, 100)] = -np.inf
    pts[idx[200:], rng.integers(0, 3, 100)] = np.nan
    for m in (AFFINE, PROJECTIVE):
        want = ref.apply_f32(m, pts)
        assert np.isnan(want[idx]).all()                       # the division turns the non-finite w into a NaN triplet
        got = fj.xfm_apply(_xfm(fj, m), torch.from_numpy(pts).cuda())
        torch.cuda.synchronize()
        assert _bits_equal(got.cpu().numpy(), want)


def test_device_apply_on_a_side_stream(fj):
    import torch
    pts = _points(1 << 20, 8)
    d = torch.from_numpy(pts).cuda()
    late = torch.zeros_like(d)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                                 # the points reach `late` only after a delay on `s`: a kernel on any
        torch.cuda._sleep(20_000_000)                          # other stream would read zeros
        late.copy_(d)
    out = fj.xfm_apply(_xfm(fj, PROJECTIVE), late, stream=s)
    s.synchronize()
    assert _bits_equal(out.cpu().numpy(), ref.apply_f32(PROJECTIVE, pts))


def test_host_form_matches_the_reference_and_pins_the_matrix_order(fj):
    pts = np.concatenate([_points(700_001, 9), _fma_witnesses(PROJECTIVE, 512)])
    x = _xfm(fj, PROJECTIVE)
    assert _bits_equal(fj.xfm_apply(x, pts), ref.apply_f32(PROJECTIVE, pts))
    flat = pts.reshape(-1).copy()
    assert _bits_equal(fj.xfm_apply(x, flat, device=fj.DEVICE_ALL), ref.apply_f32(PROJECTIVE, pts).reshape(-1))
    fj.xfm_apply(x, flat, out=flat)                                                      # in place
    assert _bits_equal(flat, ref.apply_f32(PROJECTIVE, pts).reshape(-1))
    # the C ABI takes vox2vox row-major: a pure x-translation lands on x, its transpose (a projective row) would not
    L = fj.lib()
    m = np.eye(4, dtype=np.float32)
    m[0, 3] = 5.0
    one = np.array([[1.0, 2.0, 3.0]], np.float32)
    out = np.empty_like(one)
    rowmajor = (C.c_float * 16)(*m.reshape(-1).tolist())
    assert L.fib_xfm_apply(0, rowmajor, one.ctypes.data, out.ctypes.data, 1) == 0
    assert out.tolist() == [[6.0, 2.0, 3.0]]
    assert fj.xfm_apply(fj.Xform(vox2vox=m), one).tolist() == [[6.0, 2.0, 3.0]]


# ---- fibd_stream_pack_trk_xfm -------------------------------------------------------------------------------------------------------
def _job(fj, n=20, len_max=None, lcm=False):
    """a traced job on a small curved field (fibd_stream_trace / _trace_lcm), with the field, seeds and sublist it came from"""
    import torch
    from fibers_jl_amd import _lib
    from fibers_jl_amd.stream import default_workspace, params
    nz = 1 if lcm else n
    x, y, z = np.meshgrid(np.arange(n), np.arange(n), np.arange(nz), indexing="ij")
    c = (n - 1) / 2.0
    v = np.stack([-(y - c), (x - c), np.full(x.shape, 0.0 if lcm else 0.2)], -1)
    v /= np.maximum(np.linalg.norm(v, axis=-1, keepdims=True), 1e-9)
    nvox = n * n * nz
    o = torch.from_numpy(np.ascontiguousarray(v.reshape(nvox, 3, order="F").T.astype(np.float32))).cuda()
    field, mout = fj.stream_field_device([o], mask=torch.ones(nvox, dtype=torch.uint8, device="cuda"))
    seeds = torch.nonzero(mout).flatten()
    sub = torch.tensor([[0.1, -0.2, 0.0 if lcm else 0.3], [0.3, 0.25, 0.0]], dtype=torch.float32, device="cuda")
    shape = (n, n, nz)
    prm = params(shape, 1, 3, len_max if len_max else max(shape), 60 if len_max else 45, 0.5, 0.2, ws=default_workspace(0))
    job, nl, npnt = C.c_void_p(), C.c_int64(0), C.c_int64(0)
    L = _lib.lib()
    sp = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    if lcm:
        lcms = torch.rand((10, nvox), device="cuda")
        _lib.check(L.fibd_stream_trace_lcm(C.byref(prm), field.data_ptr(), lcms.data_ptr(), 0.2, 0, 1, 11, seeds.data_ptr(), seeds.numel(),
                                           sub.data_ptr(), sub.shape[0], sp, C.byref(job), C.byref(nl), C.byref(npnt)))
    else:
        _lib.check(L.fibd_stream_trace(C.byref(prm), field.data_ptr(), seeds.data_ptr(), seeds.numel(), sub.data_ptr(), sub.shape[0], sp,
                                       C.byref(job), C.byref(nl), C.byref(npnt)))
    return job, nl.value, npnt.value, (field, shape, seeds, sub)


def _pack(fj, job, nl, npnt):
    import torch
    L = fj.lib()
    npts = torch.empty(nl, dtype=torch.int32, device="cuda")
    seed = torch.empty(nl, dtype=torch.int64, device="cuda")
    xyz = torch.empty((npnt, 3), dtype=torch.float32, device="cuda")
    sp = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert L.fibd_stream_pack(job, npts.data_ptr(), seed.data_ptr(), xyz.data_ptr(), sp) == 0
    torch.cuda.synchronize()
    return fj.Tract(xyz=xyz.cpu().numpy(), npts=npts.cpu().numpy(), seed_index=seed.cpu().numpy(), volsize=(20, 20, 20))


def _pack_trk(fj, job, nl, npnt, xfm=None, vs=(1.0, 1.0, 1.0)):
    import torch
    from fibers_jl_amd._host import m16
    L = fj.lib()
    body = torch.full((nl + 3 * npnt,), -7.0, dtype=torch.float32, device="cuda")
    sp = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    v = (C.c_float * 3)(*vs)
    if xfm is None:
        rc = L.fibd_stream_pack_trk(job, C.byref(v), body.data_ptr(), sp)
    else:
        rc = L.fibd_stream_pack_trk_xfm(job, m16(xfm.vox2vox), C.byref(v), body.data_ptr(), sp)
    torch.cuda.synchronize()
    return rc, body.cpu().numpy().tobytes()


@pytest.mark.parametrize("path", ["tile", "plain"])
def test_pack_trk_xfm_is_the_body_of_str_xform(fj, path):
    from fibers_jl_amd.trk import trk_body
    job, nl, npnt, _ = _job(fj, len_max=3000 if path == "plain" else None)     # len_max 3000: 16 lines no longer fit the LDS tile
    L = fj.lib()
    try:
        assert nl > 100
        tr = _pack(fj, job, nl, npnt)
        for m, outres in ((PROJECTIVE, (1.5, 1.25, 2.0)), (AFFINE, (0.7, 0.7, 0.9))):
            x = _xfm(fj, m, outres)
            rc, got = _pack_trk(fj, job, nl, npnt, x, tuple(float(v) for v in x.outres))
            assert rc == 0
            assert got == trk_body(ref.str_xform(x, tr), x.outres)
        rc, plain = _pack_trk(fj, job, nl, npnt, None, (1.0, 1.0, 1.0))                 # identity, outres = volres: the old body
        rc2, ident = _pack_trk(fj, job, nl, npnt, fj.Xform(), (1.0, 1.0, 1.0))
        assert rc == 0 and rc2 == 0 and ident == plain
    finally:
        L.fib_stream_job_destroy(job)


def test_pack_trk_xfm_refuses_an_lcm_job(fj):
    job, nl, npnt, _ = _job(fj, n=16, lcm=True)
    L = fj.lib()
    try:
        assert nl > 0
        rc, _ = _pack_trk(fj, job, nl, npnt, fj.Xform(vox2vox=AFFINE))
        assert rc == -7 and b"LCM" in L.fib_last_error()
    finally:
        L.fib_stream_job_destroy(job)


def test_stream_to_trk_with_xfm_writes_trk_write_of_str_xform(fj, tmp_path):
    import torch
    job, nl, npnt, (field, shape, seeds, sub) = _job(fj)
    try:
        tr = _pack(fj, job, nl, npnt)
    finally:
        fj.lib().fib_stream_job_destroy(job)
    x = _xfm(fj, PROJECTIVE, (1.5, 1.25, 2.0))
    mri = fj.MRI(np.ones(shape, np.uint8))
    f1, f2 = str(tmp_path / "host.trk"), str(tmp_path / "gpu.trk")
    assert fj.trk_write(ref.str_xform(x, tr), f1) is False
    info = fj.stream_to_trk(f2, field, shape, seeds, sub, mri, xfm=x)
    torch.cuda.synchronize()
    assert info["nlines"] == nl and open(f1, "rb").read() == open(f2, "rb").read()
    # and str_xform itself (the host-buffer path) gives the same Tract
    t2 = fj.str_xform(x, tr)
    assert _bits_equal(t2.xyz, ref.apply_f32(PROJECTIVE, tr.xyz)) and t2.volsize == (30, 25, 20)
