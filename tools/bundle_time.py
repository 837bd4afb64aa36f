#!/usr/bin/env python
"""Timing of the bundle kernels (csrc/bundle.hip) on C4's packed lines: 140^3 DTI phantom, ~1 M seeds, ~129 M points, made as
tests/test_gpu_fullsize.py makes them (and as tools/tract_select_time.py does).  HIP-event medians of
  resample      to K = 12, 20 and 100 points per line,
  assign        of the lines resampled to K = 20 to 1, 32 and 256 models (every nlines / nmodels-th line is a model),
  centroids     of the same lines with the labels and flips those assignments gave,
next to their yardstick on the same points: fibd_str_stats without scalars (one pass over the points, the same float64 segment
lengths, G lanes per line: what resample does twice, plus its running sum).  Every row is the whole API call, offset scan and
zero-fills included.  One process; run it under `timeout`.

    python tools/bundle_time.py --out profiles/bundles [--runs 7] [--only resample20,assign32] [--tag x]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
COPY_GBS = 6300.0                                                             # the device copy rate DESIGN.md section 0 quotes (GB/s)


def median_ms(fn, runs, warm=2):
    import torch
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), [round(t, 4) for t in ts]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bundles"))
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--only", default="", help="comma-separated rows to time")
    ap.add_argument("--tag", default="")
    a = ap.parse_args()
    assert a.runs >= 5, "a median of at least 5"
    import torch
    import fibers_jl_amd as fj
    from fibers_jl_amd import phantom
    dev = torch.device("cuda", 0)
    shape = (140, 140, 140)
    nvox = 140 ** 3
    bval, bvec = phantom.scheme_dti(60, 4, 1000.0, seed=2)
    dwi, _ = phantom.make_dwi_torch(shape, bval, bvec, seed=2, device=dev, nfib=1)
    o = fj.dti_fit_device(fj.DtiPlan(bval, bvec, device=0), dwi, torch.ones(nvox, dtype=torch.uint8, device=dev))
    del dwi
    field, mout = fj.stream_field_device([o["eigvec1"]], fa=o["fa"], fa_thresh=0.1, mask=phantom.ball_mask_torch(shape, dev))
    seeds = torch.nonzero(mout).flatten()
    sub = torch.tensor([[0.1, -0.2, 0.3]], dtype=torch.float32, device=dev)
    r = fj.stream_device_run(field, shape, seeds, sub, buffers=fj.StreamBuffers(dev))
    xyz, npts = r["xyz"], r["npts"]
    nl, npnt = int(npts.numel()), int(xyz.shape[0])
    res = (1.25, 1.25, 1.25)
    want = set(x for x in a.only.split(",") if x)
    rows = {}

    def row(name, fn, nbytes, note="", **extra):
        if want and name not in want:
            return
        ms, all_ms = median_ms(fn, a.runs)
        rows[name] = dict(ms=round(ms, 4), runs_ms=all_ms, bytes=int(nbytes), gb_per_s=nbytes / ms * 1e-6, note=note, **extra)
        print("%-14s %9.3f ms  %7.1f GB/s on its bytes  %s" % (name, ms, rows[name]["gb_per_s"], note), flush=True)

    work = torch.empty(fj.str_work_size(nl) // 8 + 1, dtype=torch.int64, device=dev)
    props = torch.empty((nl, 1), dtype=torch.float32, device=dev)
    row("stats", lambda: fj.str_stats_device(xyz, npts, res, out=props, work=work), npnt * 12 + nl * (4 + 8 + 4), "yardstick: one pass, the same segment lengths")
    del props
    status = torch.empty(1, dtype=torch.int64, device=dev)
    lines20 = None
    for K in (12, 20, 100):
        out = torch.empty((nl, K, 3), dtype=torch.float32, device=dev)
        nbytes = npnt * 12 + nl * (4 + 8) + nl * K * 12                       # input points + counts and offsets + K * 12 B per line
        row("resample%d" % K, lambda: fj.str_resample_device(xyz, npts, res, K, out=out, status=status, work=work), nbytes,
            "byte floor %.3f ms at %.0f GB/s" % (nbytes / COPY_GBS * 1e-6, COPY_GBS), floor_ms=nbytes / COPY_GBS * 1e-6)
        if K == 20:
            fj.str_resample_device(xyz, npts, res, K, out=out, status=status, work=work)
            assert int(status.item()) == nl
            lines20 = out
        del out
    K = 20
    for nm in (1, 32, 256):
        models = lines20[torch.arange(nm, device=dev) * (nl // nm) + nl // (2 * nm)].contiguous()
        got = fj.str_assign_device(lines20, models, res, 20.0)
        pair_points = nl * nm * K
        row("assign%d" % nm, lambda: fj.str_assign_device(lines20, models, res, 20.0), nl * (K * 12 + 9) + nm * K * 12,
            "%d lines x %d models x %d points, two norms each" % (nl, nm, K), pair_points=pair_points)
        if "assign%d" % nm in rows:
            rows["assign%d" % nm]["pair_points_per_s"] = pair_points / rows["assign%d" % nm]["ms"] * 1e3
            rows["assign%d" % nm]["norms_per_s"] = 2 * pair_points / rows["assign%d" % nm]["ms"] * 1e3
        label, flip = got["label"], got["flip"]
        kept = int((label >= 0).sum())
        acc = fj.str_centroids_device(lines20, label, flip, nm)

        def cent(nm=nm, label=label, flip=flip, acc=acc):
            # (`out=` accumulates; the timed call is the plain form, zero-fill included, into arrays that exist)
            from fibers_jl_amd import _lib
            _lib.check(_lib.lib().fibd_str_centroids(lines20.data_ptr(), nl, K, label.data_ptr(), flip.data_ptr(), nm, 0, acc[0].data_ptr(),
                                                     acc[1].data_ptr(), None))
        row("centroids%d" % nm, cent, kept * K * 12 + nl * 5 + nm * (K * 24 + 4), "%d of %d lines labelled" % (kept, nl), labelled=kept)
    res_out = dict(workload="C4 lines: 140^3 DTI phantom, ball mask, one offset, step 0.5", nlines=nl, npoints=npnt, runs=a.runs, warmups=2,
                   library=os.path.basename(fj.LIB_PATH), device=torch.cuda.get_device_name(0), copy_gb_per_s=COPY_GBS, rows=rows,
                   bytes_note="bytes: what the definition reads and writes -- resample 12 B per input point, 12 B per line (count, offset) and K * 12 B "
                              "per line out; assign the lines once, 9 B per line out, the models once; centroids the labelled lines, 5 B per line, "
                              "sums and counts once")
    if "stats" in rows:
        for k, v in rows.items():
            if k.startswith("resample"):
                v["ratio_to_stats"] = v["ms"] / rows["stats"]["ms"]
                v["ratio_to_floor"] = v["ms"] / v["floor_ms"]
    os.makedirs(a.out, exist_ok=True)
    name = os.path.join(a.out, "timings%s.json" % (("_" + a.tag) if a.tag else ""))
    with open(name, "w") as fh:
        json.dump(res_out, fh, indent=1)
    print("wrote", name)


if __name__ == "__main__":
    main()
