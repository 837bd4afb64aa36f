#!/usr/bin/env python3
"""Kernel time of constrained spherical deconvolution on the headline volume (140^3 x 270; its b = 3000 shell has 84 frames), sphere_724,
device-resident inputs, HIP events on the launch stream, the median of RUNS runs after two warm-ups: fibd_csd_rec at lmax 6 and 8
under mask A (SURVEY.md's name for the whole 140^3 box, all ones) and under the ball mask, with fibd_dki_fit on the same volume beside
it, and the distribution of the solves per voxel.  The time covers the whole call: the deconvolution kernel, the peak finder and the
peak gather.  FIBERS_HIP_LIB selects another build of the library: the A/B partners of the two design choices are csd.hip compiled with
-DFIB_CSD_B_GLOBAL (B read through the cache instead of LDS) and with -DFIB_CSD_ADD_ONLY (the matrix always built by adding the set's
rows, never by subtracting the complement's), e.g. tools/build_variant.sh csd_bglobal csd.hip -DFIB_CSD_B_GLOBAL.
Usage: python tools/csd_time.py [--shape 140] [--runs 7] [--label product] [--out profiles/csd/NAME.json]"""
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
from fibers_jl_amd.dki import DKI_FIELDS, nframes  # noqa: E402

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
    ap.add_argument("--label", default="product")
    ap.add_argument("--no-dki", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.runs >= 5
    shape = (a.shape,) * 3
    nvox = a.shape ** 3
    dev = torch.device("cuda", 0)
    bval, bvec = phantom.scheme_gqi()
    nvol = len(bval)
    dwi, _ = phantom.make_dwi_torch(shape, bval, bvec, 2, dev, nfib=2)
    masks = {"mask A": torch.ones(nvox, dtype=torch.uint8, device=dev), "ball": phantom.ball_mask_torch(shape, dev)}
    stream = torch.cuda.current_stream()
    res = dict(shape=list(shape), nvol=nvol, runs=a.runs, label=a.label, lib=os.path.basename(fj.LIB_PATH), device=torch.cuda.get_device_name(0),
               response=list(RESPONSE), sphere="sphere_724", cases={})
    for lmax in (6, 8):
        plan = fj.CsdPlan(bval, bvec, RESPONSE, fj.sphere_724, lmax=lmax)
        res["nshell"] = plan.nshell
        out = dict(sh=torch.empty((plan.n, nvox), dtype=torch.float32, device=dev), odf=torch.empty((plan.nreg, nvox), dtype=torch.float32, device=dev),
                   niter=torch.empty(nvox, dtype=torch.float32, device=dev), peak=[torch.empty((3, nvox), dtype=torch.float32, device=dev) for _ in range(3)],
                   f=[torch.empty(nvox, dtype=torch.float32, device=dev) for _ in range(3)])
        for name, m in masks.items():
            inside = int(m.sum().item())
            med, lo, hi = timed(lambda: csd_rec_device(plan, dwi, m, out=out, stream=stream), a.runs)
            it = out["niter"][m != 0]
            hist = torch.bincount(it.to(torch.int64)).cpu().tolist()
            res["cases"]["csd_rec lmax %d %s" % (lmax, name)] = dict(
                median_ms=med, min_ms=lo, max_ms=hi, voxels_inside=inside, kvoxels_inside_per_s=inside / med, us_per_voxel_inside=med * 1e3 / inside,
                solves_median=float(it.median().item()), solves_mean=float(it.mean().item()), solves_max=float(it.max().item()), solves_histogram=hist)
            print("csd_rec lmax %d %-7s median %.2f ms (min %.2f, max %.2f)  %.0f kvoxels/s inside the mask, solves median %.0f mean %.2f max %.0f"
                  % (lmax, name, med, lo, hi, inside / med, it.median().item(), it.mean().item(), it.max().item()))
        del out
        plan.close()
    if not a.no_dki:
        kplan = fj.DkiPlan(bval, bvec)
        kout = {k: torch.empty((nframes(k), nvox) if nframes(k) > 1 else (nvox,), dtype=torch.float32, device=dev) for k in DKI_FIELDS}
        for name, m in masks.items():
            inside = int(m.sum().item())
            med, lo, hi = timed(lambda: fj.dki_fit_device(kplan, dwi, m, out=kout, stream=stream), a.runs)
            res["cases"]["dki_fit %s" % name] = dict(median_ms=med, min_ms=lo, max_ms=hi, voxels_inside=inside, kvoxels_inside_per_s=inside / med)
            print("dki_fit %-7s median %.3f ms (min %.3f, max %.3f)" % (name, med, lo, hi))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
