#!/usr/bin/env python
"""Timing of the tract-map kernels (csrc/tractmap.hip) on C4's packed lines: 140^3 DTI phantom, ~1 M seeds, ~129 M points, made as
tests/test_gpu_fullsize.py makes them.  HIP-event medians of the three density modes, the sample at nframes = 1 and 3 and the
statistics, next to two rows of the same points for scale: fibd_xfm_apply (a 24-B/point copy) and the trace + pack that produced
the lines.  One process; run it under `timeout`.

    python tools/tract_maps_time.py --out profiles/tract_maps [--runs 7] [--only lines]

With FIBERS_HIP_LIB pointing at the diagnostic build (libfibers_hip_stamp.so), FIBERS_TM_LINES_G = 8 | 16 | 32 | 64 selects the lanes
per line of tm_density_lines (the A/B partners of the shipped mapping); the value is recorded in the result."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tract_maps"))
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--only", default="", help="comma-separated rows to time (points, lines, endpoints, sample1, sample3, stats, xfm, trace)")
    ap.add_argument("--tag", default="")
    a = ap.parse_args()
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
    bufs = fj.StreamBuffers(dev)
    r = fj.stream_device_run(field, shape, seeds, sub, buffers=bufs)
    xyz, npts = r["xyz"], r["npts"]
    nl, npnt = int(npts.numel()), int(xyz.shape[0])
    want = set(x for x in a.only.split(",") if x)
    rows = {}

    def row(name, fn, bytes_per_point, atomics=None):
        if want and name not in want:
            return
        ms, all_ms = median_ms(fn, a.runs)
        rows[name] = dict(ms=round(ms, 4), runs_ms=all_ms, points_per_s=npnt / ms * 1e3, gb_per_s=bytes_per_point * npnt / ms * 1e-6,
                          bytes_per_point=bytes_per_point)
        if atomics is not None:
            rows[name].update(atomic_adds=int(atomics), atomic_adds_per_s=atomics / ms * 1e3)
        print("%-10s %8.3f ms  %7.1f Gpoint/s  %7.1f GB/s%s" % (name, ms, npnt / ms * 1e-6, rows[name]["gb_per_s"],
                                                                "" if atomics is None else "  %.2f G atomic adds/s" % (atomics / ms * 1e-6)), flush=True)

    # atomic adds after run merging, counted from the points themselves
    v = torch.round(xyz).long() - 1
    lin = v[:, 0] + 140 * (v[:, 1] + 140 * v[:, 2])
    del v
    head = torch.ones(npnt, dtype=torch.bool, device=dev)
    head[1:] = lin[1:] != lin[:-1]
    head[::64] = True                                                        # mode 0 merges inside a wave's 64 consecutive points
    n_runs64 = int(head.sum())
    del head, lin
    work = torch.empty(fj.str_work_size(nl) // 8 + 1, dtype=torch.int64, device=dev)
    dens = torch.empty(nvox, dtype=torch.uint32, device=dev)
    nout = torch.empty(1, dtype=torch.int64, device=dev)
    d_lines, _ = fj.str_density_device(xyz, npts, shape, "lines")
    n_pairs = int(d_lines.view(torch.int32).long().sum())
    kw = dict(n_outside=nout, work=work)

    def density(mode):
        # (`out=` accumulates; the timed call is the plain form, zero-fill of the 11-MB map included, into a map that exists)
        from fibers_jl_amd import _lib
        from fibers_jl_amd._dev import stream_ptr
        _lib.check(_lib.lib().fibd_str_density(xyz.data_ptr(), npts.data_ptr(), nl, npnt, 140, 140, 140, _lib.DENSITY_MODES[mode], dens.data_ptr(),
                                               nout.data_ptr(), work.data_ptr(), work.numel() * 8, stream_ptr(None)))
    row("points", lambda: density("points"), 12, n_runs64)
    row("lines", lambda: density("lines"), 12, n_pairs)
    row("endpoints", lambda: density("endpoints"), 12, 2 * nl)
    s1 = torch.empty((npnt, 1), dtype=torch.float32, device=dev)
    row("sample1", lambda: fj.str_sample_device(xyz, o["fa"], shape, out=s1), 12 + 4 + 4)
    if not want or "sample3" in want:
        vol3 = torch.stack([o["fa"], o["md"], o["rd"]]).contiguous()
        s3 = torch.empty((npnt, 3), dtype=torch.float32, device=dev)
        row("sample3", lambda: fj.str_sample_device(xyz, vol3, shape, out=s3), 12 + 12 + 12)
        del s3, vol3
    props = torch.empty((nl, 2), dtype=torch.float32, device=dev)
    row("stats", lambda: fj.str_stats_device(xyz, npts, (1.25, 1.25, 1.25), s1, out=props, work=work), 12 + 4)
    if not want or "xfm" in want:
        x = fj.Xform(insize=np.array(shape), outsize=np.array(shape), inres=np.ones(3, np.float32), outres=np.ones(3, np.float32),
                     invox2ras=np.eye(4, dtype=np.float32), outvox2ras=np.eye(4, dtype=np.float32),
                     vox2vox=np.array([[1, 0, 0, 1], [0, 1, 0, 2], [0, 0, 1, 3], [0, 0, 0, 1]], np.float32), ras2ras=np.eye(4, dtype=np.float32))
        moved = torch.empty_like(xyz)
        row("xfm", lambda: fj.xfm_apply(x, xyz, out=moved), 24)
        del moved
    row("trace", lambda: fj.stream_device_run(field, shape, seeds, sub, buffers=bufs), 12)
    res = dict(workload="C4 lines: 140^3 DTI phantom, ball mask, one offset, step 0.5", nlines=nl, npoints=npnt, runs=a.runs, warmups=2,
               lines_g=os.environ.get("FIBERS_TM_LINES_G", "shipped"), library=os.path.basename(fj.LIB_PATH),
               device=torch.cuda.get_device_name(0), rows=rows,
               bytes_note="bytes_per_point: 12 B read per point, plus for the samples 4 B gathered and 4 B written per frame, for the statistics 4 B of scalars")
    os.makedirs(a.out, exist_ok=True)
    name = os.path.join(a.out, "timings%s.json" % (("_" + a.tag) if a.tag else ""))
    with open(name, "w") as fh:
        json.dump(res, fh, indent=1)
    print("wrote", name)


if __name__ == "__main__":
    main()
