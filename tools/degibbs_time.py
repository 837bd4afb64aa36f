#!/usr/bin/env python3
"""Kernel time of the Gibbs-ringing removal on the headline volume (140^3 x 270), slices across z, nshifts 20, windows 1..3,
device-resident inputs, a caller's workspace, HIP events on the launch stream, the median of RUNS runs after two warm-ups:
fibd_dwi_degibbs on one frame, on the 18 frames of b = 5 and on all 270 frames (if the series and its result do not fit, one frame's
time x 270, marked as derived), its two stages apart (the library's profile brackets: the filter, the search), the float64 FMA count a
voxel and the share of the vector rate that is, and fibd_dwi_mask on the same volume beside it.  fibd_dwi_denoise takes 10-26 s a run
there: its figure is quoted from profiles/denoise/headline.json unless --denoise measures it again (one run).  With the diagnostic
library (FIBERS_HIP_LIB pointing at libfibers_hip_stamp.so) the search runs with its candidate table staged in LDS and read through the
cache (FIBERS_DEGIBBS_TABLE).
Usage: python tools/degibbs_time.py [--shape 140] [--runs 7] [--label product] [--out profiles/degibbs/NAME.json]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import fibers_jl_amd as fj  # noqa: E402
from fibers_jl_amd import phantom  # noqa: E402
from fibers_jl_amd.degibbs import dwi_degibbs_device, dwi_degibbs_work_size  # noqa: E402
from fibers_jl_amd.mask import dwi_mask_device, dwi_mask_work_size  # noqa: E402

STAGES = ("dwi_degibbs_filter", "dwi_degibbs_search")
PEAK_FMA = 78.6e12 / 2                  # float64 vector FMAs a second of an MI355X (78.6 TFLOP/s)
K, MINW, MAXW = 20, 1, 3


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
    """ms per call of the two profile brackets, over `runs` calls"""
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
        out[name] = dict(ms_per_call=ms.value / runs, brackets_per_call=cnt.value / runs)
    return out


def fma_per_voxel(nu, nv):
    """float64 FMAs a voxel and frame as the kernels count them: the four DFT stages on the half spectrum, and 2K circulant products of
    the row length along either axis (the padding of a row to whole 8-sample items not counted)"""
    nvh = nv // 2 + 1
    filt = (2 * nvh * nu * nv + 4 * nu * nvh * nu + 4 * nu * nvh * nu + 2 * nv * nu * nvh) / (nu * nv)
    return dict(filter=filt, search=2 * K * (nu + nv), total=filt + 2 * K * (nu + nv))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, default=140)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--label", default="product")
    ap.add_argument("--denoise", action="store_true", help="measure fibd_dwi_denoise again (one run of all frames, ball mask)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.runs >= 1
    n = a.shape
    shape, nvox = (n,) * 3, n ** 3
    dev = torch.device("cuda", 0)
    bval, bvec = phantom.scheme_gqi()
    dwi, _ = phantom.make_dwi_torch(shape, bval, bvec, 2, dev, nfib=2)
    ball = phantom.ball_mask_torch(shape, dev)
    dwi = dwi * (0.02 + 0.98 * ball.to(torch.float32))          # a head with an edge to ring at, as tools/mask_time.py makes it
    b0 = [int(i) for i in (bval == bval.min()).nonzero()[0]]
    stream = torch.cuda.current_stream()
    diagnostic = "stamp" in os.path.basename(fj.LIB_PATH)
    fma = fma_per_voxel(n, n)
    res = dict(shape=list(shape), runs=a.runs, label=a.label, lib=os.path.basename(fj.LIB_PATH), device=torch.cuda.get_device_name(0),
               nshifts=K, min_w=MINW, max_w=MAXW, slice_axis=2, fma_per_voxel_and_frame=fma, peak_fma_per_s=PEAK_FMA, cases={})

    def show(name, r):
        res["cases"][name] = r
        print("%-52s median %.3f ms (min %.3f, max %.3f)" % (name, r["median_ms"], r["min_ms"], r["max_ms"]), flush=True)

    free = torch.cuda.mem_get_info()[0]
    series = [("1 frame", dwi[b0[0]:b0[0] + 1].contiguous()), ("%d frames of b = %g" % (len(b0), bval.min()), dwi[b0].contiguous())]
    need = 2 * dwi.numel() * 4 + dwi_degibbs_work_size(n, n, n, len(bval))
    if need < free // 2:
        series.append(("all %d frames" % len(bval), dwi))
    tables = ("lds", "cache") if diagnostic else ("library",)
    for table in tables:
        if diagnostic:
            os.environ["FIBERS_DEGIBBS_TABLE"] = table
        for sname, d in series:
            N = d.shape[0]
            out = dict(dwi=torch.empty((N, nvox), dtype=torch.float32, device=dev))
            work = torch.empty(dwi_degibbs_work_size(n, n, n, N) // 8 + 1, dtype=torch.int64, device=dev)
            call = lambda: dwi_degibbs_device(d, shape, 2, K, MINW, MAXW, out=out, work=work, stream=stream)     # noqa: E731
            r = timed(call, a.runs)
            r.update(frames=N, work_bytes=work.numel() * 8, ns_per_voxel_and_frame=r["median_ms"] * 1e6 / (nvox * N),
                     share_of_vector_fma_rate=fma["total"] * nvox * N / (r["median_ms"] * 1e-3) / PEAK_FMA)
            r["stages"] = stages(call, min(a.runs, 3))
            for k, s in r["stages"].items():
                part = "filter" if k.endswith("filter") else "search"
                s["share_of_vector_fma_rate"] = fma[part] * nvox * N / (s["ms_per_call"] * 1e-3) / PEAK_FMA if s["ms_per_call"] > 0 else None
            show("fibd_dwi_degibbs %s [%s]" % (sname, table), r)
            print("    %.2f ns a voxel and frame, %.1f %% of the float64 vector FMA rate" % (r["ns_per_voxel_and_frame"],
                                                                                           100 * r["share_of_vector_fma_rate"]), flush=True)
            for k, s in r["stages"].items():
                print("    %-20s %.3f ms a call, %.1f %% of the rate" % (k, s["ms_per_call"], 100 * (s["share_of_vector_fma_rate"] or 0)), flush=True)
            if sname == "1 frame" and len(series) == 2:
                res["cases"]["fibd_dwi_degibbs all %d frames [%s] (derived: one frame's time x %d)" % (len(bval), table, len(bval))] = dict(
                    median_ms=r["median_ms"] * len(bval), derived=True)
            del out, work
    os.environ.pop("FIBERS_DEGIBBS_TABLE", None)

    out = dict(mask=torch.empty(nvox, dtype=torch.uint8, device=dev), b0=torch.empty(nvox, dtype=torch.float32, device=dev),
               info=torch.empty(8, dtype=torch.int64, device=dev))
    work = torch.empty(dwi_mask_work_size(*shape) // 8 + 1, dtype=torch.int64, device=dev)
    show("fibd_dwi_mask r=2 numpass=4 (%d frames)" % len(b0), timed(lambda: dwi_mask_device(dwi, shape, b0, 2, 4, out=out, work=work, stream=stream), a.runs))
    if a.denoise:
        from fibers_jl_amd.denoise import dwi_denoise_device, dwi_denoise_work_size
        o = dict(dwi=torch.empty((len(bval), nvox), dtype=torch.float32, device=dev), sigma=torch.empty(nvox, dtype=torch.float32, device=dev),
                 rank=torch.empty(nvox, dtype=torch.float32, device=dev))
        w = torch.empty(dwi_denoise_work_size(n, n, n, len(bval), 5) // 8 + 1, dtype=torch.int64, device=dev)
        a0, a1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a0.record()
        dwi_denoise_device(dwi, ball, shape, 5, "exp2", out=o, work=w, stream=stream)
        a1.record()
        a1.synchronize()
        ms = a0.elapsed_time(a1)
        show("fibd_dwi_denoise all %d frames, ball mask (one run)" % len(bval), dict(median_ms=ms, min_ms=ms, max_ms=ms))
    else:
        try:
            rec = json.load(open(os.path.join(ROOT, "profiles", "denoise", "headline.json")))["cases"]["dwi_denoise all 270 ball"]
            res["cases"]["fibd_dwi_denoise all 270 frames, ball mask (quoted from profiles/denoise/headline.json)"] = dict(
                median_ms=rec["median_ms"], quoted=True)
            print("fibd_dwi_denoise all 270 frames, ball mask: %.0f ms (quoted from profiles/denoise/headline.json)" % rec["median_ms"])
        except (OSError, KeyError, ValueError):
            pass
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
