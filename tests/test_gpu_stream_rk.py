"""The trilinear tracker's midpoint (RK2) and classical Runge-Kutta (RK4) integrators (fib_stream_params.interp = 2, 3; NOT in the
reference) through the public interface and the C ABI, against the NumPy Float32 restatement of the header's definition
(tests/stream_rk_ref.py, pinned by tests/test_stream_rk_ref.py): every operation on both sides is an IEEE single operation in the
header's order, so lines are compared EXACTLY."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stream_rk_ref as rk  # noqa: E402
from test_gpu_stream import _fields  # noqa: E402  (the inputs of test_trilinear_option_follows_its_definition)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIB_ERR_INVALID, FIB_ERR_UNSUPPORTED = -1, -7


def _same(tr, ref):
    assert tr.nstr == len(ref["npts"]), (tr.nstr, len(ref["npts"]))
    assert np.array_equal(tr.npts, ref["npts"]) and np.array_equal(tr.seed_index, ref["seed_index"])
    assert tr.xyz.shape == ref["xyz"].shape and np.array_equal(tr.xyz, ref["xyz"]), float(np.abs(tr.xyz - ref["xyz"]).max())


def _noisy_case(nvec):
    rng = np.random.default_rng(21 + nvec)
    n = 10
    f = _fields(n, 5)
    ov = [f["noisy"]]
    if nvec >= 2:
        o2 = f["circ"].copy()
        o2[rng.random((n, n, n)) < 0.25] = 0                              # voxels with one vector only
        ov.append(np.asfortranarray(o2))
    if nvec >= 3:
        ov.append(f["wavy"])
    mask = (rng.random((n, n, n)) < 0.92).astype(np.uint8)
    sub = np.array([[0.1, -0.2, 0.3], [-0.25, 0.15, 0.05]], np.float32)
    return ov, mask, sub, rng


@pytest.mark.parametrize("integrator", ["rk2", "rk4"])
@pytest.mark.parametrize("nvec,smooth", [(1, 0.2), (2, 0.2), (2, 0.0)])
def test_rk_lines_equal_the_restatement_bit_for_bit(fj, orc, integrator, nvec, smooth):
    """10^3 noisy field, 8 % mask holes, a second volume with 25 % empty voxels, two offsets, len_max = 14: corners outside the volume,
    corners without a vector, stages that find nothing, the carried vector index, len_max"""
    ov, mask, sub, _ = _noisy_case(nvec)
    kw = dict(mask=fj.MRI(mask), sublist=sub, len_min=3, len_max=14, smooth_coeff=smooth, interp="trilinear")
    tr = fj.stream([fj.MRI(o) for o in ov], integrator=integrator, **kw)
    eul = fj.stream([fj.MRI(o) for o in ov], **kw)
    mk, arr = orc.stream_work(ov, None, 0.03, None, 0.1, mask)
    ref = rk.stream(arr, mk, orc.seeds_from_mask(mk), sub, len_min=3, smooth=smooth, len_max=14, integrator=integrator)
    _same(tr, ref)
    assert tr.nstr > 200
    assert tr.nstr != eul.nstr or not np.array_equal(tr.xyz, eul.xyz)        # (it is another tracker than Euler on the same field)


@pytest.mark.parametrize("integrator", ["rk2", "rk4"])
def test_rk_step_one_len_max_seed_mask_three_vectors(fj, orc, integrator):
    ov, mask, sub, rng = _noisy_case(3)
    seed = (rng.random(mask.shape) < 0.3).astype(np.uint8)
    tr = fj.stream([fj.MRI(o) for o in ov], mask=fj.MRI(mask), seed=fj.MRI(seed), sublist=sub, len_min=2, len_max=5, step_size=1.0,
                   interp="trilinear", integrator=integrator)
    mk, arr = orc.stream_work(ov, None, 0.03, None, 0.1, mask)
    ref = rk.stream(arr, mk, orc.seeds_from_mask(seed > 0), sub, len_min=2, step=1.0, len_max=5, integrator=integrator)
    _same(tr, ref)
    assert tr.nstr > 100 and tr.npts.max() == 7                             # lines that use up len_max (+ 2, stream.jl:674)


@pytest.mark.parametrize("step,integrator,lo,hi", [(0.5, "euler", 0.5, None), (0.5, "rk2", None, 0.01), (0.5, "rk4", None, 0.01),
                                                   (1.0, "rk2", None, 0.03), (1.0, "rk4", None, 0.03)])
def test_circular_field_known_answer_on_the_gpu(fj, step, integrator, lo, hi):
    """tests/test_stream_rk_ref.py's circles, on the GPU result itself: 102 points per line; Euler leaves its circle by more than half a
    voxel, RK2 and RK4 stay within 0.01 (step 0.5) / 0.03 (step 1.0) of it"""
    seedvol = np.zeros(rk.CIRCLE_SHAPE, np.uint8)
    for s in rk.CIRCLE_SEEDS:
        seedvol[s[0] - 1, s[1] - 1, s[2] - 1] = 1
    tr = fj.stream(fj.MRI(rk.circle_field()), mask=fj.MRI(np.ones(rk.CIRCLE_SHAPE, np.uint8)), seed=fj.MRI(seedvol), sublist=rk.CIRCLE_SUB,
                   smooth_coeff=0.0, ang_thresh=45, len_max=100, step_size=step, interp="trilinear", integrator=integrator)
    assert tr.nstr == 4 and list(tr.npts) == [102] * 4
    seeds = sorted(rk.CIRCLE_SEEDS, key=lambda s: s[0] - 1 + 48 * (s[1] - 1))      # findall order
    for i, s in enumerate(seeds):
        drift = rk.circle_drift(tr.line(i), s, rk.CIRCLE_SUB[0])
        print("step %.1f %-5s seed %s drift %.5f" % (step, integrator, s, drift))
        assert lo is None or drift >= lo, (s, drift)
        assert hi is None or drift <= hi, (s, drift)


def _device_case(fj, nvec=2):
    import torch
    dev = torch.device("cuda", 0)
    ov, mask, sub, _ = _noisy_case(nvec)
    n = mask.shape[0]
    planar = [torch.from_numpy(np.ascontiguousarray(o.reshape(n ** 3, 3, order="F").T)).to(dev) for o in ov]
    field, mout = fj.stream_field_device(planar, mask=torch.from_numpy(mask.reshape(-1, order="F").copy()).to(dev))
    return ov, mask, sub, field, torch.nonzero(mout).flatten(), torch.from_numpy(sub).to(dev), (n, n, n)


@pytest.mark.parametrize("integrator", ["rk2", "rk4"])
def test_every_road_gives_the_same_lines(fj, integrator):
    """host tier on one device and on a device set that names GPU 0 twice, stream_device, stream_device_run, the enqueue form"""
    import torch
    ov, mask, sub, field, seeds, subd, shape = _device_case(fj)
    kw = dict(len_min=3, len_max=14, interp="trilinear", integrator=integrator)
    one = fj.stream([fj.MRI(o) for o in ov], mask=fj.MRI(mask), sublist=sub, **kw)
    assert one.nstr > 200
    try:
        fj.init([0, 0])
        two = fj.stream([fj.MRI(o) for o in ov], mask=fj.MRI(mask), sublist=sub, device=fj.DEVICE_ALL, **kw)
    finally:
        fj.shutdown()
    assert np.array_equal(two.npts, one.npts) and np.array_equal(two.seed_index, one.seed_index) and np.array_equal(two.xyz, one.xyz)
    d = fj.stream_device(field, shape, seeds, subd, **kw)
    r = fj.stream_device_run(field, shape, seeds, subd, **kw)
    bufs = fj.StreamBuffers(field.device, one.nstr, one.xyz.shape[0])
    _, counts = fj.stream_device_run_enqueue(field, shape, seeds, subd, bufs, **kw)
    torch.cuda.synchronize()
    nl, npnt = counts.tolist()
    e = dict(npts=bufs.npts[:nl], seed_index=bufs.seed_index[:nl], xyz=bufs.xyz[:npnt])
    for what, got in (("stream_device", d), ("stream_device_run", r), ("stream_device_run_enqueue", e)):
        assert np.array_equal(got["npts"].cpu().numpy(), one.npts), what
        assert np.array_equal(got["seed_index"].cpu().numpy(), one.seed_index), what
        assert np.array_equal(got["xyz"].cpu().numpy(), one.xyz), what


def test_wide_form_of_the_rk_tracers_matches_the_32_bit_form():
    """stream_trace_kernel<.., 2 | 3, WIDE> on small fields, where only the DIAGNOSTIC build can force the wide form: a child process
    that loads libfibers_hip_stamp.so (tools/stream_rk_wide_check.py, as tools/stream_wide_check.py does for the other modes)"""
    if not os.path.exists(os.path.join(ROOT, "fibers.jl_amd", "libfibers_hip_stamp.so")):
        pytest.skip("the diagnostic build is absent (make -C fibers.jl_amd/csrc stamp)")
    env = {k: v for k, v in os.environ.items() if k != "FIBERS_HIP_LIB"}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "stream_rk_wide_check.py")], env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    assert "stream rk wide check: ok" in out.stdout


def test_error_codes(fj):
    import torch
    from fibers_jl_amd import _lib
    ov, mask, sub, field, seeds, subd, shape = _device_case(fj, 1)
    smod = sys.modules[fj.stream_device_run.__module__]
    L = _lib.lib()

    def trace(interp, search_dist=0, lcms=None):
        prm = smod._params(shape, 1, 3, 14, 45, 0.5, 0.2, search_dist, 10, None)
        prm.interp = interp
        job, nl, npnt = C.c_void_p(), C.c_int64(0), C.c_int64(0)
        if lcms is None:
            rc = L.fibd_stream_trace(C.byref(prm), field.data_ptr(), seeds.data_ptr(), seeds.numel(), subd.data_ptr(), subd.shape[0], None,
                                     C.byref(job), C.byref(nl), C.byref(npnt))
        else:
            rc = L.fibd_stream_trace_lcm(C.byref(prm), field.data_ptr(), lcms.data_ptr(), 0.099, 0, 1, 0, seeds.data_ptr(), seeds.numel(),
                                         subd.data_ptr(), subd.shape[0], None, C.byref(job), C.byref(nl), C.byref(npnt))
        if job:
            L.fib_stream_job_destroy(job)
        return rc
    assert trace(4) == FIB_ERR_INVALID and trace(-1) == FIB_ERR_INVALID
    assert trace(2, search_dist=3) == FIB_ERR_UNSUPPORTED and trace(3, search_dist=3) == FIB_ERR_UNSUPPORTED
    lc = torch.rand((10, shape[0] ** 3), device=field.device)
    assert trace(2, lcms=lc) == FIB_ERR_UNSUPPORTED and trace(3, lcms=lc) == FIB_ERR_UNSUPPORTED
    assert trace(2) == 0 and trace(3) == 0
    with pytest.raises(ValueError):
        fj.stream(fj.MRI(ov[0]), mask=fj.MRI(mask), sublist=sub, integrator="rk4", interp="nearest")
    with pytest.raises(ValueError):
        fj.stream(fj.MRI(ov[0]), mask=fj.MRI(mask), sublist=sub, integrator="rk3", interp="trilinear")
    with pytest.raises(ValueError):
        fj.stream_device(field, shape, seeds, subd, integrator="rk2")


def test_nearest_and_euler_trilinear_results_are_unchanged(fj, orc):
    """interp = 0 is the reference's tracker (the oracle), interp = 1 the NumPy restatement of the Euler form, as before"""
    from oracle import oracle_np as onp
    ov, mask, sub, _ = _noisy_case(2)
    kw = dict(mask=fj.MRI(mask), sublist=sub, len_min=3, len_max=14)
    near = fj.stream([fj.MRI(o) for o in ov], **kw)
    ref = orc.stream(ov, sub, mask=mask, len_min=3, len_max=14, nthreads=2)
    _same(near, ref)
    tri = fj.stream([fj.MRI(o) for o in ov], interp="trilinear", **kw)
    tri2 = fj.stream([fj.MRI(o) for o in ov], interp="trilinear", integrator="euler", **kw)
    mk, arr = orc.stream_work(ov, None, 0.03, None, 0.1, mask)
    npts, sidx, xyz = [], [], []
    for si, seed in enumerate(orc.seeds_from_mask(mk)):
        for k in range(sub.shape[0]):
            line = onp.stream_line([int(v) for v in seed], sub[k], arr, mk, len_max=14, interp="trilinear")
            if line.shape[0] >= 3:
                npts.append(line.shape[0]); sidx.append(si * sub.shape[0] + k); xyz.append(line)
    want = dict(npts=np.array(npts, np.int32), seed_index=np.array(sidx, np.int64), xyz=np.concatenate(xyz, 0))
    _same(tri, want)
    _same(tri2, want)
