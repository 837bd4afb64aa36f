#!/usr/bin/env python3
"""Kernel time of multi-shell multi-tissue deconvolution on the headline volume (140^3 x 270: 18 frames at b = 5 and 84 directions each at
b = 1000, 2000, 3000), all 270 frames, sphere_724, lmax 8, two isotropic tissues; device-resident inputs, HIP events on the launch
stream, the median of RUNS runs after two warm-ups: fibd_msmt_rec under mask A (SURVEY.md's name for the whole 140^3 box, all ones) and
under the ball mask, with fibd_csd_rec (lmax 8) on the b = 3000 shell of the same volume beside it in the same run, the mean solves per
voxel and the share of voxels at the niter cap.  The time covers the whole call: the deconvolution kernel, the peak finder and the peak
gather.  FIBERS_HIP_LIB selects another build of the library: the A/B partner of the one design choice is msmt.hip compiled with
-DFIB_MSMT_B_GLOBAL (the WM rows of B read through the cache instead of LDS): tools/build_variant.sh msmt_bglobal msmt.hip -DFIB_MSMT_B_GLOBAL;
-DFIB_MSMT_FOUR_CHAINS makes X's four independent chains of FMAs instead of one.  --frames N replaces the headline scheme by N frames (5 at b = 5, the
rest random directions in equal parts on b = 1000, 2000, 3000): 512 is the most a plan takes and the largest workgroup.
Usage: python tools/msmt_time.py [--shape 140] [--frames N] [--runs 7] [--label product] [--out profiles/msmt/NAME.json]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

import fibers_jl_amd as fj  # noqa: E402
from csd_time import RESPONSE, timed  # noqa: E402
from fibers_jl_amd import phantom  # noqa: E402
from fibers_jl_amd.csd import csd_rec_device  # noqa: E402
from fibers_jl_amd.msmt import msmt_rec_device  # noqa: E402

GM, CSF = (0.8e-3, 900.0), (3.0e-3, 1500.0)      # mono-exponential isotropic responses: (diffusivity, b = 0 signal)


def outputs(n, nreg, nvox, dev, niso=None):
    o = dict(sh=torch.empty((n, nvox), dtype=torch.float32, device=dev), odf=torch.empty((nreg, nvox), dtype=torch.float32, device=dev),
             niter=torch.empty(nvox, dtype=torch.float32, device=dev), peak=[torch.empty((3, nvox), dtype=torch.float32, device=dev) for _ in range(3)],
             f=[torch.empty(nvox, dtype=torch.float32, device=dev) for _ in range(3)])
    if niso is not None:
        o["iso"] = [torch.empty(nvox, dtype=torch.float32, device=dev) for _ in range(niso)]
    return o


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, default=140)
    ap.add_argument("--frames", type=int, default=0)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--label", default="product")
    ap.add_argument("--no-csd", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.runs >= 5
    shape = (a.shape,) * 3
    nvox = a.shape ** 3
    dev = torch.device("cuda", 0)
    bval, bvec = phantom.scheme_gqi()
    if a.frames:
        nd = (a.frames - 5) // 3
        assert a.frames == 5 + 3 * nd, "--frames must be 5 + a multiple of 3"
        g = np.random.default_rng(5).normal(size=(3 * nd, 3))
        bval = np.concatenate([np.full(5, 5.0)] + [np.full(nd, b) for b in (1000.0, 2000.0, 3000.0)]).astype(np.float32)
        bvec = np.concatenate([np.zeros((5, 3)), g / np.linalg.norm(g, axis=1)[:, None]]).astype(np.float32)
    nvol = len(bval)
    dwi, _ = phantom.make_dwi_torch(shape, bval, bvec, 2, dev, nfib=2)
    masks = {"mask A": torch.ones(nvox, dtype=torch.uint8, device=dev), "ball": phantom.ball_mask_torch(shape, dev)}
    stream = torch.cuda.current_stream()
    shell, bbar = fj.msmt_shells(bval)
    resp = fj.MsmtResponse(bbar, fj.msmt_wm_response(*RESPONSE, bbar, 8), np.array([s0 * np.exp(-bbar * d) for d, s0 in (GM, CSF)], np.float32))
    res = dict(shape=list(shape), nvol=nvol, runs=a.runs, label=a.label, lib=os.path.basename(fj.LIB_PATH), device=torch.cuda.get_device_name(0),
               response=list(RESPONSE), gm=list(GM), csf=list(CSF), shells=[float(b) for b in bbar],
               frames_per_shell=np.bincount(shell).tolist(), sphere="sphere_724", cases={})

    def case(label, fn, out, m, cap):
        inside = int(m.sum().item())
        med, lo, hi = timed(fn, a.runs)
        it = out["niter"][m != 0]
        at_cap = int((it >= cap).sum().item())
        res["cases"][label] = dict(median_ms=med, min_ms=lo, max_ms=hi, voxels_inside=inside, kvoxels_inside_per_s=inside / med,
                                   us_per_voxel_inside=med * 1e3 / inside, solves_median=float(it.median().item()),
                                   solves_mean=float(it.mean().item()), solves_max=float(it.max().item()), voxels_at_cap=at_cap,
                                   share_at_cap=at_cap / inside, solves_histogram=torch.bincount(it.to(torch.int64)).cpu().tolist())
        print("%-24s median %.2f ms (min %.2f, max %.2f)  %.0f kvoxels/s inside the mask, solves median %.0f mean %.2f max %.0f, at the cap %d of %d"
              % (label, med, lo, hi, inside / med, it.median().item(), it.mean().item(), it.max().item(), at_cap, inside), flush=True)

    plan = fj.MsmtPlan(bval, bvec, resp, fj.sphere_724, lmax=8)
    out = outputs(plan.nwm, plan.nreg, nvox, dev, plan.niso)
    for name, m in masks.items():
        case("msmt_rec lmax 8 niso 2 %s" % name, lambda: msmt_rec_device(plan, dwi, m, out=out, stream=stream), out, m, 50)
    iso = torch.stack(out["iso"])[:, masks["ball"] != 0]
    res["iso_negative_share_ball"] = [float((iso[t] < 0).float().mean().item()) for t in range(plan.niso)]
    del out, iso
    plan.close()
    if not a.no_csd:
        cplan = fj.CsdPlan(bval, bvec, RESPONSE, fj.sphere_724, lmax=8)
        res["csd_nshell"] = cplan.nshell
        out = outputs(cplan.n, cplan.nreg, nvox, dev)
        for name, m in masks.items():
            case("csd_rec lmax 8 %s" % name, lambda: csd_rec_device(cplan, dwi, m, out=out, stream=stream), out, m, 50)
        cplan.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
