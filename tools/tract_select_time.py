#!/usr/bin/env python
"""Timing of the selection / connectome kernels (csrc/tractsel.hip) on C4's packed lines: 140^3 DTI phantom, ~1 M seeds, ~129 M
points, made as tests/test_gpu_fullsize.py makes them (and as tools/tract_maps_time.py does).  HIP-event medians of
  select        with an ROI bit volume packed from 1 and from 32 ROIs (spheres of radius 25 at seeded centres),
  gather        keeping all lines, every second line and every hundredth,
  connectome    with 84 and 2 035 nodes (cubes of 10 voxels dealt round-robin to the nodes), with and without W,
  roi_pack      of the 32 ROIs,
next to their yardsticks on the same points: fibd_str_sample with one frame (12 B/point in plus one 4-byte gather: select's access
pattern), fibd_xfm_apply (the 24-B/point copy a keep-all gather amounts to) and the ENDPOINTS density (two points per line and
their atomics: the connectome without W).  Every row is the whole API call, offset scan and zero-fills included.  One process; run
it under `timeout`.

    python tools/tract_select_time.py --out profiles/tract_select [--runs 7] [--only select1,select32] [--tag g16]

With FIBERS_HIP_LIB pointing at the diagnostic build (libfibers_hip_stamp.so), FIBERS_TS_SELECT_G = 8 | 16 | 32 | 64 selects the
lanes per line of ts_select (the A/B partners of the shipped mapping); the value is recorded in the result."""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tract_select"))
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--only", default="", help="comma-separated rows to time")
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
    r = fj.stream_device_run(field, shape, seeds, sub, buffers=fj.StreamBuffers(dev))
    xyz, npts = r["xyz"], r["npts"]
    nl, npnt = int(npts.numel()), int(xyz.shape[0])
    want = set(x for x in a.only.split(",") if x)
    rows = {}

    def row(name, fn, nbytes, note=""):
        if want and name not in want:
            return
        ms, all_ms = median_ms(fn, a.runs)
        rows[name] = dict(ms=round(ms, 4), runs_ms=all_ms, bytes=int(nbytes), gb_per_s=nbytes / ms * 1e-6, points_per_s=npnt / ms * 1e3, note=note)
        print("%-16s %8.3f ms  %7.1f GB/s on its bytes  %s" % (name, ms, rows[name]["gb_per_s"], note), flush=True)

    # 32 ROIs: spheres of radius 25 voxels at seeded centres inside the ball
    rng = np.random.default_rng(3)
    ax = torch.arange(1, 141, device=dev, dtype=torch.float32)
    rois = torch.empty((32, nvox), dtype=torch.uint8, device=dev)
    for k, c in enumerate(rng.uniform(35, 105, (32, 3))):
        d2 = (ax[None, None, :] - c[0]) ** 2 + (ax[None, :, None] - c[1]) ** 2 + (ax[:, None, None] - c[2]) ** 2          # [z][y][x]: x fastest
        rois[k] = (d2 <= 625).reshape(-1).to(torch.uint8)
    bits32 = fj.str_roi_pack_device(rois)
    bits1 = fj.str_roi_pack_device(rois[:1].contiguous())
    work = torch.empty(fj.str_select_work_size(nl) // 8 + 1, dtype=torch.int64, device=dev)
    line_bytes = 4 + 1 + 12 + 8                                               # npts, keep, hits, the line's offset
    sel_bytes = npnt * (12 + 4) + nl * line_bytes
    kept = {}

    def select(bits, name, **kw):
        keep, hits, counts = fj.str_select_device(xyz, npts, shape, bits, work=work, **kw)
        kept[name] = counts
    row("roi_pack32", lambda: fj.str_roi_pack_device(rois, out=bits32), nvox * (32 + 4))
    row("select1", lambda: select(bits1, "select1", visit_all=1), sel_bytes, "visit_all = ROI 0")
    row("select32", lambda: select(bits32, "select32", visit_all=1 | (1 << 31), visit_none=1 << 7, end_any=1 << 12), sel_bytes, "four masks over 32 ROIs")
    for k, v in kept.items():
        rows[k]["kept_lines"], rows[k]["kept_points"] = (int(x) for x in v.cpu())

    idx = torch.arange(nl, device=dev)
    out = dict(xyz=torch.empty((npnt, 3), dtype=torch.float32, device=dev), npts=torch.empty(nl, dtype=torch.int32, device=dev),
               index=torch.empty(nl, dtype=torch.int64, device=dev), counts=torch.empty(3, dtype=torch.int64, device=dev))
    for name, flags in (("gather_all", idx >= 0), ("gather_half", idx % 2 == 0), ("gather_1pct", idx % 100 == 0)):
        if want and name not in want:
            continue
        fl = flags.to(torch.uint8)
        fj.str_gather_device(xyz, npts, fl, out=out, work=work)
        kl, kp, status = (int(x) for x in out["counts"].cpu())
        assert status == 0
        row(name, lambda: fj.str_gather_device(xyz, npts, fl, out=out, work=work), kp * 24 + nl * (4 + 1 + 24) + kl * 12, "%d lines, %d points kept" % (kl, kp))
        rows[name]["kept_lines"], rows[name]["kept_points"] = kl, kp
    del out

    cube = torch.arange(140, device=dev) // 10
    cubes = (cube[None, None, :] + 14 * (cube[None, :, None] + 14 * cube[:, None, None])).reshape(-1)                      # 2 744 cubes of 10^3 voxels
    for L in (84, 2035):
        lab = (cubes % L + 1).to(torch.int32)
        for with_w in (False, True):
            name = "connectome%d%s" % (L, "_w" if with_w else "")
            if want and name not in want:
                continue
            res = fj.str_connectome_device(xyz, npts, shape, lab, L, volres=(1.25, 1.25, 1.25) if with_w else None, assign=False, work=work)
            acc = dict(counts=res["counts"], lengths=res["lengths"])

            def conn(lab=lab, L=L, with_w=with_w, acc=acc):
                # (`out=` accumulates; the timed call is the plain form, zero-fill of C and W included, into matrices that exist)
                from fibers_jl_amd import _lib
                import ctypes as C
                vr = (C.c_float * 3)(1.25, 1.25, 1.25)
                _lib.check(_lib.lib().fibd_str_connectome(xyz.data_ptr(), npts.data_ptr(), nl, npnt, 140, 140, 140, vr if with_w else None, lab.data_ptr(), None,
                                                          0, L, 0, acc["counts"].data_ptr(), acc["lengths"].data_ptr() if with_w else None, None,
                                                          nlines_dev.data_ptr(), work.data_ptr(), work.numel() * 8, None))
            nlines_dev = torch.empty(1, dtype=torch.int64, device=dev)
            nbytes = (npnt * 12 if with_w else nl * 24) + nl * (4 + 8 + 8) + (L + 1) ** 2 * (12 if with_w else 4)
            cells = int((res["counts"].view(torch.int32) != 0).sum())
            row(name, conn, nbytes, "%d of %d cells non-zero, %d atomic adds" % (cells, (L + 1) ** 2, (4 if with_w else 2) * nl))

    s1 = torch.empty((npnt, 1), dtype=torch.float32, device=dev)
    row("sample1", lambda: fj.str_sample_device(xyz, o["fa"], shape, out=s1), npnt * (12 + 4 + 4), "yardstick of select")
    del s1
    if not want or "xfm" in want:
        x = fj.Xform(insize=np.array(shape), outsize=np.array(shape), inres=np.ones(3, np.float32), outres=np.ones(3, np.float32),
                     invox2ras=np.eye(4, dtype=np.float32), outvox2ras=np.eye(4, dtype=np.float32),
                     vox2vox=np.array([[1, 0, 0, 1], [0, 1, 0, 2], [0, 0, 1, 3], [0, 0, 0, 1]], np.float32), ras2ras=np.eye(4, dtype=np.float32))
        moved = torch.empty_like(xyz)
        row("xfm", lambda: fj.xfm_apply(x, xyz, out=moved), npnt * 24, "yardstick of gather_all")
        del moved
    twork = torch.empty(fj.str_work_size(nl) // 8 + 1, dtype=torch.int64, device=dev)
    dens = torch.zeros(nvox, dtype=torch.int32, device=dev).view(torch.uint32)
    nout = torch.empty(1, dtype=torch.int64, device=dev)

    def ends():
        from fibers_jl_amd import _lib
        _lib.check(_lib.lib().fibd_str_density(xyz.data_ptr(), npts.data_ptr(), nl, npnt, 140, 140, 140, 2, dens.data_ptr(), nout.data_ptr(), twork.data_ptr(),
                                               twork.numel() * 8, None))
    row("endpoints", ends, nl * (24 + 4 + 8 + 8) + nvox * 4, "yardstick of the connectome without W (11-MB zero-fill included)")
    res = dict(workload="C4 lines: 140^3 DTI phantom, ball mask, one offset, step 0.5", nlines=nl, npoints=npnt, runs=a.runs, warmups=2,
               select_g=os.environ.get("FIBERS_TS_SELECT_G", "shipped"), library=os.path.basename(fj.LIB_PATH), device=torch.cuda.get_device_name(0), rows=rows,
               bytes_note="bytes: what the definition reads and writes -- select 12 B + one 4-B gather per point and 25 B per line; gather 24 B per kept "
                          "point and 29 B per line (+ 12 per kept line); connectome 2 points per line (every point with W), 20 B per line, the matrices once")
    os.makedirs(a.out, exist_ok=True)
    name = os.path.join(a.out, "timings%s.json" % (("_" + a.tag) if a.tag else ""))
    with open(name, "w") as fh:
        json.dump(res, fh, indent=1)
    print("wrote", name)


if __name__ == "__main__":
    main()
