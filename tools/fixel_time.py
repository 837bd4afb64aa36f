#!/usr/bin/env python
"""Timing of the tractogram-weight kernels (csrc/fixel.hip) on C4's lines traced on the headline GQI peaks: 140^3 GQI phantom, ball
mask, every mask voxel a seed, one offset, step 0.5 -- device-resident inputs, HIP-event medians of 7 after 2 warm-ups.  Rows:
  assign        fibd_fixel_assign: the fixel id of every point (offset scan included)
  scatter       fibd_fixel_td: zero-fill and one scatter of q along the ids (uint64 vector atomics, one per run inside a round of 16)
  update        fibd_fixel_update: one gather of D_s and the ISRA step of every line
  weights50     fibd_str_weights, the whole call at niter = 50
next to the nearest existing scatter and gather on the same points: fibd_str_density (mode points; uint32 atomics, one per run inside
a wave's 64 points) and fibd_str_sample (one frame).  One process; run it under `timeout`.

    python tools/fixel_time.py --out profiles/fixel [--runs 7] [--size 140] [--niter 50]"""
import argparse
import ctypes as C
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fixel"))
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--size", type=int, default=140)
    ap.add_argument("--niter", type=int, default=50)
    ap.add_argument("--tag", default="")
    a = ap.parse_args()
    assert a.runs >= 5, "a median of at least 5"
    import torch
    import fibers_jl_amd as fj
    from fibers_jl_amd import _lib, fixel, phantom
    dev = torch.device("cuda", 0)
    shape = (a.size,) * 3
    nvox = a.size ** 3
    bval, bvec = phantom.scheme_gqi()
    dwi, _ = phantom.make_dwi_torch(shape, bval, bvec, seed=3, device=dev)
    bm = phantom.ball_mask_torch(shape, dev)
    o = fj.odf_rec_device(fj.OdfPlan("gqi", bval, bvec, fj.sphere_642, device=0), dwi, bm)
    del dwi
    peak, qa = o["peak"], o["qa"]
    del o
    field, mout = fj.stream_field_device(peak, f=qa, f_thresh=0.03, mask=bm)
    seeds = torch.nonzero(mout).flatten()
    sub = torch.tensor([[0.1, -0.2, 0.3]], dtype=torch.float32, device=dev)
    r = fj.stream_device_run(field, shape, seeds, sub, buffers=fj.StreamBuffers(dev))
    xyz, npts = r["xyz"], r["npts"]
    del field
    nl, npnt, nvec = int(npts.numel()), int(xyz.shape[0]), len(peak)
    nfix = nvec * nvox
    L = _lib.lib()
    rows = {}

    def row(name, fn, note="", **extra):
        ms, all_ms = median_ms(fn, a.runs)
        rows[name] = dict(ms=round(ms, 4), runs_ms=all_ms, points_per_s=npnt / ms * 1e3, note=note, **extra)
        print("%-10s %9.3f ms  %7.2f G points/s  %s" % (name, ms, npnt / ms * 1e-6, note), flush=True)

    work = torch.empty(fj.str_work_size(nl) // 8 + 1, dtype=torch.int64, device=dev)
    ids = torch.empty(npnt, dtype=torch.int32, device=dev)
    row("assign", lambda: fixel.fixel_assign_device(xyz, npts, shape, peak, qa, bm, 0.03, 45, out=ids, work=work), "12 B of xyz in, 4 B of id out per point")
    _, counts = fixel.fixel_assign_device(xyz, npts, shape, peak, qa, bm, 0.03, 45, out=ids, work=work)
    assigned = npnt - int(counts[0].item())
    # the atomics of one scatter: a run of equal ids of one line inside a round of 16 points
    off = torch.cumsum(npts.to(torch.int64), 0) - npts
    pos = torch.arange(npnt, device=dev, dtype=torch.int64) - torch.repeat_interleave(off, npts.to(torch.int64))
    del off
    head = (pos % 16 == 0)
    del pos
    head[1:] |= ids[1:] != ids[:-1]
    adds = int((head & (ids >= 0)).sum().item())
    del head
    q = torch.full((nl,), 1 << 20, dtype=torch.uint32, device=dev)
    td = torch.empty(nfix, dtype=torch.int64, device=dev)
    row("scatter", lambda: fixel.fixel_td_device(ids, npts, q, nfix, out=td, work=work), "%d uint64 atomic adds for %d assigned points" % (adds, assigned),
        atomic_adds=adds, assigned_points=assigned)
    rows["scatter"]["adds_per_s"] = adds / rows["scatter"]["ms"] * 1e3
    # one update: Aq, the state and mu as fibd_str_weights makes them, N_s from a first call; the timed calls go on updating q against the
    # same TDq (the gather and the step cost the same whatever q holds)
    aq = torch.empty(nfix, dtype=torch.int64, device=dev)
    state = torch.empty(fixel.STATE_SLOTS, dtype=torch.int64, device=dev)
    nline = torch.empty(nl, dtype=torch.int64, device=dev)
    ov = (C.c_void_p * nvec)(*[t.data_ptr() for t in peak])
    fv = (C.c_void_p * nvec)(*[t.data_ptr() for t in qa])
    sp = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(L.fibd_fixel_quantise(nvec, nvox, ov, fv, bm.data_ptr(), 0.03, aq.data_ptr(), state.data_ptr(), sp))
    fixel.fixel_td_device(ids, npts, q, nfix, out=td, work=work)
    _lib.check(L.fibd_fixel_mu(td.data_ptr(), nfix, state.data_ptr(), sp))
    wb = work.numel() * 8
    _lib.check(L.fibd_fixel_update(ids.data_ptr(), npts.data_ptr(), nl, npnt, aq.data_ptr(), td.data_ptr(), nfix, 1, state.data_ptr(), nline.data_ptr(),
                                   q.data_ptr(), work.data_ptr(), wb, sp))
    row("update", lambda: _lib.check(L.fibd_fixel_update(ids.data_ptr(), npts.data_ptr(), nl, npnt, aq.data_ptr(), td.data_ptr(), nfix, 0, state.data_ptr(),
                                                         nline.data_ptr(), q.data_ptr(), work.data_ptr(), wb, sp)), "4 B of id and one 8-B gather per assigned point")
    del aq, nline, td, q
    big = torch.empty(fixel.str_weights_work_size(nl, npnt, nvec, nvox) // 8 + 1, dtype=torch.int64, device=dev)
    res = {}

    def whole():
        res["r"] = fixel.str_weights_device(xyz, npts, shape, peak, qa, bm, 0.03, 45, niter=a.niter, work=big, check=False)
    row("weights%d" % a.niter, whole, "assign, %d x (update, scatter, cost) and the outputs" % a.niter)
    st = res["r"]["state"].cpu().numpy()
    cost = res["r"]["cost"].cpu().numpy()
    fit = dict(mu=float(st[1:2].view(np.float64)[0]), counts=[int(v) for v in st[5:10]], cost_first=float(cost[0]), cost_last=float(cost[-1]))
    print("fit:", fit, flush=True)
    del big, res
    dens = torch.empty(nvox, dtype=torch.uint32, device=dev)
    nout = torch.empty(1, dtype=torch.int64, device=dev)
    dwork = torch.empty(fj.str_work_size(nl) // 8 + 1, dtype=torch.int64, device=dev)

    def density():
        _lib.check(L.fibd_str_density(xyz.data_ptr(), npts.data_ptr(), nl, npnt, shape[0], shape[1], shape[2], 0, dens.data_ptr(), nout.data_ptr(),
                                      dwork.data_ptr(), dwork.numel() * 8, sp))
    row("density", density, "fibd_str_density, mode points: uint32 atomics, one per run inside 64 points")
    vol = qa[0]
    samp = torch.empty((npnt, 1), dtype=torch.float32, device=dev)
    row("sample", lambda: fj.str_sample_device(xyz, vol, shape, out=samp), "fibd_str_sample, one frame")
    out = dict(workload="C4's lines on the headline GQI peaks: %d^3 GQI phantom, ball mask, one offset, step 0.5, f_thresh 0.03, 45 degrees" % a.size,
               nlines=nl, npoints=npnt, nvec=nvec, nfixels=nfix, niter=a.niter, runs=a.runs, warmups=2, library=os.path.basename(fj.LIB_PATH),
               device=torch.cuda.get_device_name(0), fit=fit, rows=rows)
    os.makedirs(a.out, exist_ok=True)
    name = os.path.join(a.out, "timings%s.json" % (("_" + a.tag) if a.tag else ""))
    with open(name, "w") as fh:
        json.dump(out, fh, indent=1)
    print("wrote", name)


if __name__ == "__main__":
    main()
