#!/usr/bin/env python3
"""The trace kernel's time for every integrator of the tracer on C4's job (DTI 140^3 principal eigenvector, ball mask, 998 592 seeds,
one sub-voxel offset -- built as tools/bench_legs.py dti_and_c4 builds it): nearest voxel (interp 0), trilinear + Euler (1), RK2 (2) and
RK4 (3) at step 0.5, and RK4 at step 1.0.  hipEvent brackets of the library's own `stream_trace` scope (fib_profile_*), one per call:
median of --reps runs after --warmup calls, the chip first brought out of its idle state the way bench.py's `timed` does it (the same
call repeated for PRECOND_S seconds).  Points written and Gpoints/s of the trace kernel beside each, and RK against the expectation
T(k stages) ~ T0 + k (T1 - T0).  One JSON line per case, then a table.

    python tools/stream_rk_time.py [--reps 7] [--warmup 2] [--cases nearest,euler,rk2,rk4,rk4_step1] [--json FILE]
FIBERS_HIP_LIB=<another build of the same ABI> times that library instead (its interp 2 / 3 may be refused: such cases are skipped)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

import fibers_jl_amd as fj  # noqa: E402
from fibers_jl_amd import phantom  # noqa: E402
from bench_legs import PEAK_HBM_GBS  # noqa: E402  (the roof the project quotes)

SHAPE = (140, 140, 140)
PRECOND_S = 0.15                                                   # bench.py: ~50 ms of load takes the chip out of its idle power state
CASES = {"nearest": dict(interp="nearest"), "euler": dict(interp="trilinear"), "rk2": dict(interp="trilinear", integrator="rk2"),
         "rk4": dict(interp="trilinear", integrator="rk4"), "rk4_step1": dict(interp="trilinear", integrator="rk4", step_size=1.0),
         "euler_step1": dict(interp="trilinear", step_size=1.0), "rk2_step1": dict(interp="trilinear", integrator="rk2", step_size=1.0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cases", default="nearest,euler,rk2,rk4,rk4_step1")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    assert args.reps >= 5 and args.warmup >= 2
    dev = torch.device("cuda", 0)
    L = fj.lib()
    bval, bvec = phantom.scheme_dti(60, 4, 1000.0, seed=2)
    dwi, _ = phantom.make_dwi_torch(SHAPE, bval, bvec, seed=2, device=dev, nfib=1)
    o = fj.dti_fit_device(fj.DtiPlan(bval, bvec), dwi, torch.ones(SHAPE[0] ** 3, dtype=torch.uint8, device=dev))
    del dwi
    field, mout = fj.stream_field_device([o["eigvec1"]], fa=o["fa"], fa_thresh=0.1, mask=phantom.ball_mask_torch(SHAPE, dev))
    seeds = torch.nonzero(mout).flatten()
    sub = torch.tensor([[0.1, -0.2, 0.3]], dtype=torch.float32, device=dev)
    xyz = {}

    def xyz_out(n):
        if xyz.get("t") is None or xyz["t"].numel() < 3 * n:
            xyz["t"] = torch.empty(int(3 * n * 1.05) + 16, dtype=torch.float32, device=dev)
        return xyz["t"]
    rows = {}
    for name in args.cases.split(","):
        kw = CASES[name]
        run = lambda: fj.stream_device(field, SHAPE, seeds, sub, xyz_out=xyz_out, **kw)   # noqa: E731
        try:
            t0 = time.perf_counter()
            r = run()
            torch.cuda.synchronize()
        except fj.FibersError as e:
            print(json.dumps(dict(case=name, skipped=str(e))), flush=True)
            continue
        for _ in range(int(max(5.0, min(2000.0, PRECOND_S / max(time.perf_counter() - t0, 1e-5))))):
            run()
        for _ in range(args.warmup):
            run()
        torch.cuda.synchronize()
        L.fib_profile_filter(b"stream_trace")
        ms = []
        for _ in range(args.reps):
            L.fib_profile_enable(1); L.fib_profile_reset()
            run()
            torch.cuda.synchronize()
            t, cnt = C.c_double(), C.c_int64()
            L.fib_profile_get(b"stream_trace", C.byref(t), C.byref(cnt))
            L.fib_profile_enable(0)
            assert cnt.value == 1
            ms.append(t.value)
        L.fib_profile_filter(None)
        npt, nl = int(r["xyz"].shape[0]), int(r["npts"].numel())
        med = statistics.median(ms)
        rows[name] = dict(case=name, lib=os.path.basename(fj.LIB_PATH), seeds=int(seeds.numel()), lines=nl, points=npt, trace_ms_median=round(med, 4),
                          trace_ms_min=round(min(ms), 4), trace_ms_max=round(max(ms), 4), reps=args.reps, gpoints_per_s=round(npt / med / 1e6, 2),
                          scratch_bytes_written=12 * npt, scratch_store_frac_of_roof=round(12 * npt / (med * 1e-3) / 1e9 / PEAK_HBM_GBS, 4))
        print(json.dumps(rows[name]), flush=True)
    if "nearest" in rows and "euler" in rows:
        t0, t1 = rows["nearest"]["trace_ms_median"], rows["euler"]["trace_ms_median"]
        for name, k in (("rk2", 2), ("rk4", 4), ("rk4_step1", 4)):
            if name in rows:
                exp = t0 + k * (t1 - t0)
                print("%-10s %.3f ms   T0 + %d (T1 - T0) = %.3f ms   ratio %.2f   (needs an explanation above %.3f ms)"
                      % (name, rows[name]["trace_ms_median"], k, exp, rows[name]["trace_ms_median"] / exp, t0 + 1.5 * k * (t1 - t0)))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(list(rows.values()), f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
