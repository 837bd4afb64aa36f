"""Timing of the transform hot path on the C4 tracking job (DTI 140^3 principal eigenvector, ball mask, one sub-voxel offset):
  - fibd_xfm_apply on C4's packed points (24 B per point), out of place and in place: hipEvent ms and TB/s against 8 and 6.3 TB/s;
  - fibd_stream_pack_trk_xfm against fibd_stream_pack_trk on the same traced job (interleaved calls, medians);
  - fib_xfm_apply (host buffers, PCIe both ways) against the NumPy float32 restatement run on 16 threads.
Prints one JSON object and writes it to --out.  The kernel split: run under `rocprofv3 --kernel-trace --stats -- python tools/xform_time.py
--no-host`."""
import argparse
import ctypes as C
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import fibers_jl_amd as fj  # noqa: E402
from fibers_jl_amd import _lib, phantom  # noqa: E402
from fibers_jl_amd._host import m16  # noqa: E402
from fibers_jl_amd.stream import default_workspace, params  # noqa: E402
import xform_ref  # noqa: E402

M = np.array([[0.98, -0.17, 0.05, 3.25], [0.16, 0.97, -0.11, -7.5], [-0.07, 0.12, 1.03, 12.125], [1e-4, -2e-4, 1.5e-4, 1.0]], np.float32)


def events_ms(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-host", action="store_true", help="skip the host-form comparison (profiler runs)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    shape = (140, 140, 140)
    L = _lib.lib()
    bval, bvec = phantom.scheme_dti(60, 4, 1000.0, seed=2)
    dwi, _ = phantom.make_dwi_torch(shape, bval, bvec, seed=2, device=dev, nfib=1)
    plan = fj.DtiPlan(bval, bvec)
    o = fj.dti_fit_device(plan, dwi, torch.ones(140 ** 3, dtype=torch.uint8, device=dev))
    del dwi
    bm = phantom.ball_mask_torch(shape, dev)
    field, mout = fj.stream_field_device([o["eigvec1"]], fa=o["fa"], fa_thresh=0.1, mask=bm)
    seeds = torch.nonzero(mout).flatten()
    sub = torch.tensor([[0.1, -0.2, 0.3]], dtype=torch.float32, device=dev)
    prm = params(shape, 1, 3, None, 45, 0.5, 0.2, ws=default_workspace(0))
    job, nl, npnt = C.c_void_p(), C.c_int64(0), C.c_int64(0)
    sp = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(L.fibd_stream_trace(C.byref(prm), field.data_ptr(), seeds.data_ptr(), seeds.numel(), sub.data_ptr(), 1, sp,
                                   C.byref(job), C.byref(nl), C.byref(npnt)))
    nl, npnt = nl.value, npnt.value
    res = dict(job=dict(seeds=int(seeds.numel()), lines=nl, points=npnt), matrix=M.tolist())
    try:
        npts = torch.empty(nl, dtype=torch.int32, device=dev)
        seed_index = torch.empty(nl, dtype=torch.int64, device=dev)
        xyz = torch.empty((npnt, 3), dtype=torch.float32, device=dev)
        _lib.check(L.fibd_stream_pack(job, npts.data_ptr(), seed_index.data_ptr(), xyz.data_ptr(), sp))
        # pack_trk vs pack_trk_xfm, interleaved
        body = torch.empty(nl + 3 * npnt, dtype=torch.float32, device=dev)
        vs = (C.c_float * 3)(1.0, 1.0, 1.0)
        mx = m16(M)
        plain, xf = [], []
        for _ in range(args.reps):
            plain += events_ms(lambda: _lib.check(L.fibd_stream_pack_trk(job, C.byref(vs), body.data_ptr(), sp)), 1, 1)
            xf += events_ms(lambda: _lib.check(L.fibd_stream_pack_trk_xfm(job, mx, C.byref(vs), body.data_ptr(), sp)), 1, 1)
        res["pack_trk_ms"] = dict(median=float(np.median(plain)), min=float(np.min(plain)))
        res["pack_trk_xfm_ms"] = dict(median=float(np.median(xf)), min=float(np.min(xf)))
        res["pack_trk_xfm_over_pack_trk"] = res["pack_trk_xfm_ms"]["median"] / res["pack_trk_ms"]["median"]
    finally:
        L.fib_stream_job_destroy(job)
    # the standalone apply on C4's points
    out = torch.empty_like(xyz)
    x = fj.Xform(vox2vox=M)
    t_oop = events_ms(lambda: fj.xfm_apply(x, xyz, out=out), args.reps)
    work = xyz.clone()
    t_ip = events_ms(lambda: fj.xfm_apply(x, work, out=work), args.reps)
    nbytes = 24.0 * npnt
    for name, t in (("xfm_apply_out_of_place", t_oop), ("xfm_apply_in_place", t_ip)):
        med = float(np.median(t))
        res[name] = dict(median_ms=med, min_ms=float(np.min(t)), bytes=nbytes, tb_per_s=nbytes / (med * 1e-3) / 1e12,
                         frac_of_8tbs=nbytes / (med * 1e-3) / 8e12, frac_of_6_3tbs=nbytes / (med * 1e-3) / 6.3e12)
    if not args.no_host:
        pts = xyz.cpu().numpy()
        want_dev = out.cpu().numpy()
        t_host = []
        for _ in range(3):
            t0 = time.perf_counter()
            got = fj.xfm_apply(x, pts)
            t_host.append(time.perf_counter() - t0)
        res["host_form_bit_identical_to_device"] = bool(np.array_equal(got.view(np.uint32), want_dev.view(np.uint32)))
        chunks = np.array_split(np.arange(npnt), 16)
        ref_out = np.empty_like(pts)

        def part(ix):
            ref_out[ix[0]: ix[-1] + 1] = xform_ref.apply_f32(M, pts[ix[0]: ix[-1] + 1])
        t_np = []
        with ThreadPoolExecutor(16) as pool:
            for _ in range(3):
                t0 = time.perf_counter()
                list(pool.map(part, chunks))
                t_np.append(time.perf_counter() - t0)
        res["numpy_restatement_bit_identical"] = bool(np.array_equal(ref_out.view(np.uint32), want_dev.view(np.uint32)))
        res["host_form_s"] = dict(median=float(np.median(t_host)), all=t_host, gb_per_s_each_way=nbytes / 2 / np.median(t_host) / 1e9)
        res["numpy_16_threads_s"] = dict(median=float(np.median(t_np)), all=t_np)
    res["device"] = torch.cuda.get_device_name(0)
    line = json.dumps(res, indent=1)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
