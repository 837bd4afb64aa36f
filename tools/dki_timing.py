#!/usr/bin/env python3
"""Kernel time of the kurtosis fit on the headline volume (140^3 x 270, sphere_642), device-resident inputs, HIP events on the launch
stream (torch's current stream, passed to the fit explicitly, is the one the events are recorded on), the median of RUNS runs after
two warm-ups: fibd_dki_fit under mask A (SURVEY.md's name for the whole 140^3 box, all ones) and under the ball mask, fibd_dti_fit on
the same volume for comparison, and the HBM floor of the algorithmic traffic (4 * nvol + 1 bytes in, 136 out per voxel inside the mask;
1 byte per voxel outside).  FIBERS_HIP_LIB selects another build of the library (e.g. one compiled with -DFIB_DKI_NO_MAPS, which
leaves the direction loop out).  Usage: python tools/dki_timing.py [--shape 140] [--runs 7] [--out profiles/dki/NAME.json]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import fibers_jl_amd as fj  # noqa: E402
from fibers_jl_amd import phantom  # noqa: E402
from fibers_jl_amd.dki import DKI_FIELDS, nframes  # noqa: E402
from fibers_jl_amd.dti import DTI_FIELDS  # noqa: E402

HBM_BYTES_PER_S = 8.0e12


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
    kplan, tplan = fj.DkiPlan(bval, bvec), fj.DtiPlan(bval, bvec)
    kout = {k: torch.empty((nframes(k), nvox) if nframes(k) > 1 else (nvox,), dtype=torch.float32, device=dev) for k in DKI_FIELDS}
    tout = {k: kout[k] for k in DTI_FIELDS}
    res = dict(shape=list(shape), nvol=nvol, ndir=kplan.ndir, runs=a.runs, lib=os.path.basename(fj.LIB_PATH), device=torch.cuda.get_device_name(0), cases={})
    for name, m in masks.items():
        inside = int(m.sum().item())
        for what, fn, out_bytes in (("dki_fit", lambda: fj.dki_fit_device(kplan, dwi, m, out=kout, stream=stream), 136),
                                    ("dti_fit", lambda: fj.dti_fit_device(tplan, dwi, m, out=tout, stream=stream), 64)):
            med, lo, hi = timed(fn, a.runs)
            # whole waves outside the mask read no frame; outputs are written (as zeros) everywhere
            floor_ms = ((4.0 * nvol) * inside + (1 + out_bytes) * nvox) / HBM_BYTES_PER_S * 1e3
            res["cases"]["%s %s" % (what, name)] = dict(median_ms=med, min_ms=lo, max_ms=hi, voxels_inside=inside, hbm_floor_ms=floor_ms,
                                                       fraction_of_floor=floor_ms / med, mvoxels_inside_per_s=inside / med / 1e3)
            print("%-8s %-9s median %.3f ms (min %.3f, max %.3f)  HBM floor %.3f ms -> %.2f of it, %.0f Mvoxels/s inside the mask"
                  % (what, name, med, lo, hi, floor_ms, floor_ms / med, inside / med / 1e3))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
