#!/usr/bin/env python3
"""Kernel time of Marchenko-Pastur denoising on the headline volume (140^3 x 270), P = 5, estimator exp2, device-resident inputs, HIP
events on the launch stream, the median of RUNS runs after two warm-ups: fibd_dwi_denoise on the 84 frames of the b = 3000 shell
(r = 84) and on all 270 frames (r = 125), under mask A (SURVEY.md's name for the whole 140^3 box, all ones) and under the ball mask,
with fibd_csd_rec (lmax 8, sphere_724) on the same volume beside it, and the distribution of the ranks kept.
Usage: python tools/denoise_time.py [--shape 140] [--runs 7] [--label product] [--out profiles/denoise/NAME.json]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import fibers_jl_amd as fj  # noqa: E402
from fibers_jl_amd import phantom  # noqa: E402
from fibers_jl_amd.csd import csd_rec_device  # noqa: E402
from fibers_jl_amd.denoise import dwi_denoise_device, dwi_denoise_work_size  # noqa: E402

RESPONSE = (1.7e-3, 0.3e-3, 1000.0)


def timed(fn, runs):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, default=140)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--patch", type=int, default=5)
    ap.add_argument("--label", default="product")
    ap.add_argument("--no-csd", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.runs >= 1
    shape = (a.shape,) * 3
    nvox = a.shape ** 3
    dev = torch.device("cuda", 0)
    bval, bvec = phantom.scheme_gqi()
    dwi, _ = phantom.make_dwi_torch(shape, bval, bvec, 2, dev, nfib=2)
    shell = torch.as_tensor(bval == bval.max(), device=dev)
    series = {"shell %d" % int(shell.sum().item()): dwi[shell].contiguous(), "all %d" % len(bval): dwi}
    masks = {"mask A": torch.ones(nvox, dtype=torch.uint8, device=dev), "ball": phantom.ball_mask_torch(shape, dev)}
    stream = torch.cuda.current_stream()
    res = dict(shape=list(shape), runs=a.runs, label=a.label, patch=a.patch, estimator="exp2", lib=os.path.basename(fj.LIB_PATH),
               device=torch.cuda.get_device_name(0), cases={})
    for sname, d in series.items():
        N = d.shape[0]
        out = dict(dwi=torch.empty((N, nvox), dtype=torch.float32, device=dev), sigma=torch.empty(nvox, dtype=torch.float32, device=dev),
                   rank=torch.empty(nvox, dtype=torch.float32, device=dev))
        work = torch.empty(dwi_denoise_work_size(a.shape, a.shape, a.shape, N, a.patch) // 8 + 1, dtype=torch.int64, device=dev)
        for mname, m in masks.items():
            inside = int(m.sum().item())
            med, lo, hi = timed(lambda: dwi_denoise_device(d, m, shape, a.patch, "exp2", out=out, work=work, stream=stream), a.runs)
            rk = out["rank"][m != 0]
            failed = int((rk < 0).sum().item())
            hist = torch.bincount(rk.clamp(min=0).to(torch.int64)).cpu().tolist()
            sg = out["sigma"][m != 0]
            res["cases"]["dwi_denoise %s %s" % (sname, mname)] = dict(
                frames=N, r=min(a.patch ** 3, N), median_ms=med, min_ms=lo, max_ms=hi, voxels_inside=inside, kvoxels_inside_per_s=inside / med,
                us_per_voxel_inside=med * 1e3 / inside, not_converged=failed, rank_histogram=hist, sigma_mean=float(sg[rk >= 0].mean().item()),
                work_bytes=work.numel() * 8)
            print("dwi_denoise %-9s %-7s median %.1f ms (min %.1f, max %.1f)  %.1f kvoxels/s inside the mask, %.1f us a voxel, %d not converged"
                  % (sname, mname, med, lo, hi, inside / med, med * 1e3 / inside, failed), flush=True)
        del out, work
    if not a.no_csd:
        plan = fj.CsdPlan(bval, bvec, RESPONSE, fj.sphere_724, lmax=8)
        out = dict(sh=torch.empty((plan.n, nvox), dtype=torch.float32, device=dev), odf=torch.empty((plan.nreg, nvox), dtype=torch.float32, device=dev),
                   niter=torch.empty(nvox, dtype=torch.float32, device=dev), peak=[torch.empty((3, nvox), dtype=torch.float32, device=dev) for _ in range(3)],
                   f=[torch.empty(nvox, dtype=torch.float32, device=dev) for _ in range(3)])
        for mname, m in masks.items():
            inside = int(m.sum().item())
            med, lo, hi = timed(lambda: csd_rec_device(plan, dwi, m, out=out, stream=stream), a.runs)
            res["cases"]["csd_rec lmax 8 %s" % mname] = dict(median_ms=med, min_ms=lo, max_ms=hi, voxels_inside=inside, kvoxels_inside_per_s=inside / med)
            print("csd_rec lmax 8 %-7s median %.2f ms (min %.2f, max %.2f)" % (mname, med, lo, hi), flush=True)
        plan.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
