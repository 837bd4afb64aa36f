#!/usr/bin/env python3
"""Kernel times of dwi_mask on the headline volume (140^3 x 270): the 18 frames of the smallest b-value, radius 2, four passes,
device-resident inputs, HIP events on the launch stream, the median of RUNS runs after two warm-ups.  It times the whole fibd_dwi_mask,
every stage of it (the library's profile brackets, summed over the launches of a stage), one pass of the median at each radius, the
components alone, and the device-to-device copy of one frame beside them.  With the diagnostic library (FIBERS_HIP_LIB pointing at
libfibers_hip_stamp.so) it runs the median under each selection scheme at every radius (FIBERS_MEDIAN_SCHEME = bisect | columns);
the library itself runs bisection at radius 1 and 2 and sorted columns at radius 3.
Usage: python tools/mask_time.py [--shape 140] [--runs 7] [--label product] [--out profiles/mask/NAME.json]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import fibers_jl_amd as fj  # noqa: E402
from fibers_jl_amd import phantom  # noqa: E402
from fibers_jl_amd.mask import (dwi_mask_device, dwi_mask_work_size, info_dict, mask_components_device, mask_components_work_size,  # noqa: E402
                                vol_median_device, vol_median_work_size)

STAGES = ("vm_mean_frames", "vm_median", "vm_minmax_hist", "vm_otsu", "vm_threshold", "vm_cc_label", "vm_cc_fill", "vm_dilate")


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
    return dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms))


def stages(fn, runs):
    """ms per call of every profile bracket, over `runs` calls"""
    L = fj.lib()
    torch.cuda.synchronize()
    L.fib_profile_enable(1)
    L.fib_profile_reset()
    for _ in range(runs):
        fn()
    torch.cuda.synchronize()
    L.fib_profile_enable(0)
    out = {}
    for name in STAGES:
        ms, cnt = C.c_double(), C.c_int64()
        L.fib_profile_get(name.encode(), C.byref(ms), C.byref(cnt))
        out[name] = dict(ms_per_call=ms.value / runs, launches_per_call=cnt.value / runs)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, default=140)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--label", default="product")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.runs >= 1
    shape = (a.shape,) * 3
    nvox = a.shape ** 3
    dev = torch.device("cuda", 0)
    bval, bvec = phantom.scheme_gqi()
    dwi, _ = phantom.make_dwi_torch(shape, bval, bvec, 2, dev, nfib=2)
    ball = phantom.ball_mask_torch(shape, dev)
    dwi = dwi * (0.02 + 0.98 * ball.to(torch.float32))          # a head: the signal outside the ball is 2 % of what it was
    frames = [int(i) for i in (bval == bval.min()).nonzero()[0]]
    stream = torch.cuda.current_stream()
    diagnostic = "stamp" in os.path.basename(fj.LIB_PATH)
    res = dict(shape=list(shape), runs=a.runs, label=a.label, lib=os.path.basename(fj.LIB_PATH), device=torch.cuda.get_device_name(0),
               frames=len(frames), radius=2, numpass=4, cases={})

    def show(name, r):
        res["cases"][name] = r
        print("%-44s median %.3f ms (min %.3f, max %.3f)" % (name, r["median_ms"], r["min_ms"], r["max_ms"]), flush=True)

    frame = dwi[frames[0]]
    copy = torch.empty_like(frame)
    show("copy of one frame (device to device)", timed(lambda: copy.copy_(frame), a.runs))

    out = dict(mask=torch.empty(nvox, dtype=torch.uint8, device=dev), b0=torch.empty(nvox, dtype=torch.float32, device=dev),
               info=torch.empty(8, dtype=torch.int64, device=dev))
    work = torch.empty(dwi_mask_work_size(*shape) // 8 + 1, dtype=torch.int64, device=dev)
    schemes = ("bisect", "columns") if diagnostic else ("library: bisect at r = 1, 2, columns at r = 3",)
    for scheme in schemes:
        if diagnostic:
            os.environ["FIBERS_MEDIAN_SCHEME"] = scheme
        whole = lambda: dwi_mask_device(dwi, shape, frames, 2, 4, out=out, work=work, stream=stream)     # noqa: E731
        r = timed(whole, a.runs)
        r["info"] = info_dict(out["info"])
        r["work_bytes"] = work.numel() * 8
        r["stages"] = stages(whole, a.runs)
        show("fibd_dwi_mask r=2 numpass=4 [%s]" % scheme, r)
        for name, s in r["stages"].items():
            print("    %-16s %.3f ms a call in %.0f launches" % (name, s["ms_per_call"], s["launches_per_call"]), flush=True)
        b0 = out["b0"].clone()
        med = torch.empty_like(b0)
        for radius in (1, 2, 3):
            w = torch.empty(vol_median_work_size(*shape, 1) // 8 + 1, dtype=torch.int64, device=dev)
            r = timed(lambda: vol_median_device(b0, shape, radius, 1, out=med, work=w, stream=stream), a.runs)
            r["ns_per_voxel"] = r["median_ms"] * 1e6 / nvox
            show("fibd_vol_median r=%d one pass [%s]" % (radius, scheme), r)
    os.environ.pop("FIBERS_MEDIAN_SCHEME", None)

    cw = torch.empty(mask_components_work_size(*shape) // 8 + 1, dtype=torch.int64, device=dev)
    co = dict(labels=torch.empty(nvox, dtype=torch.int32, device=dev), mask=torch.empty(nvox, dtype=torch.uint8, device=dev),
              info=torch.empty(8, dtype=torch.int64, device=dev))
    noise = (torch.rand(nvox, device=dev) < 0.5).to(torch.uint8)
    for name, m in (("ball", ball), ("random, density 0.5", noise)):
        for kl, fh in ((False, False), (True, True)):
            r = timed(lambda: mask_components_device(m, shape, kl, fh, out=co, work=cw, stream=stream), a.runs)
            r["info"] = info_dict(co["info"])
            show("fibd_mask_components %s keep_largest=%d fill_holes=%d" % (name, kl, fh), r)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
