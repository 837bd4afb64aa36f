#!/usr/bin/env python3
"""Kernel times of the non-linear warps (csrc/warp.hip), measured as tools/vol_xform_time.py measures: HIP events on the launch stream,
device-resident operands, the median of 7 runs after 2 warm-ups, one process.  The field is a smooth synthetic displacement (3 mm
sines with wavelengths of 38 to 50 mm) on 182 x 218 x 182 at 1 mm: 115 MB packed.
  pack      fibd_warp_pack of that field;
  points    the C4 lines (DTI 140^3 principal eigenvector, ball mask, one sub-voxel offset: tools/xform_time.py) through
            fibd_warp_points, beside fibd_xfm_apply on the same points in the same run;
  volume    140 x 140 x 92 x 1 and x 198 frames pulled onto the field's grid by fibd_warp_volume (trilinear), beside fibd_vol_xform
            onto the same grid through the affine part alone;
  invert    fibd_warp_invert at niter = 20 onto the field's own grid.
Writes timings.json and TIMINGS.md into --out (default profiles/warp).  --small runs the same code on toy sizes (a rehearsal: its
numbers are overheads)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import fibers_jl_amd as fj  # noqa: E402
from fibers_jl_amd import phantom, warp  # noqa: E402

RUNS, WARM = 7, 2


def timed(fn):
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(RUNS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms)


def grid_vox2ras(shape, res, angle_deg=0.0):
    """a grid of `shape` voxels of `res` mm centred on the RAS origin, rotated by angle_deg about the oblique axis (1, 2, 3)"""
    ax = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    t = np.deg2rad(angle_deg)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    M = np.eye(4)
    M[:3, :3] = (np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * (K @ K)) * res
    M[:3, 3] = -M[:3, :3] @ ((np.array(shape) - 1) / 2.0)
    return M.astype(np.float32)


def smooth_field(shape, v2r, dev, amp=3.0):
    """amp * (sin(y/6 + 0.3), 0.8 cos(z/7), 0.6 sin((x + y)/8)) mm at the nodes, planar [3, nvox] on the device"""
    nx, ny, nz = shape
    k, j, i = torch.meshgrid(torch.arange(nz, device=dev, dtype=torch.float32), torch.arange(ny, device=dev, dtype=torch.float32),
                             torch.arange(nx, device=dev, dtype=torch.float32), indexing="ij")
    m = torch.from_numpy(v2r).to(dev)
    x, y, z = (m[r, 0] * i + m[r, 1] * j + m[r, 2] * k + m[r, 3] for r in range(3))
    return torch.stack([amp * torch.sin(y / 6 + 0.3), 0.8 * amp * torch.cos(z / 7), 0.6 * amp * torch.sin((x + y) / 8)]).reshape(3, -1).contiguous()


def c4_points(n, dev):
    """the packed points of the C4 tracking job on an n^3 volume (tools/xform_time.py): 1-based voxel coordinates [npoints, 3]"""
    shape = (n, n, n)
    bval, bvec = phantom.scheme_dti(60, 4, 1000.0, seed=2)
    dwi, _ = phantom.make_dwi_torch(shape, bval, bvec, seed=2, device=dev, nfib=1)
    plan = fj.DtiPlan(bval, bvec)
    o = fj.dti_fit_device(plan, dwi, torch.ones(n ** 3, dtype=torch.uint8, device=dev))
    del dwi
    field, mout = fj.stream_field_device([o["eigvec1"]], fa=o["fa"], fa_thresh=0.1, mask=phantom.ball_mask_torch(shape, dev))
    seeds = torch.nonzero(mout).flatten()
    sub = torch.tensor([[0.1, -0.2, 0.3]], dtype=torch.float32, device=dev)
    r = fj.stream_device(field, shape, seeds, sub)
    plan.close()
    return r["xyz"].reshape(-1, 3).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "warp"))
    ap.add_argument("--frames", type=int, default=198)
    ap.add_argument("--small", action="store_true", help="toy sizes (a rehearsal of the code path, not a measurement)")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    fshape, dshape, nline = ((182, 218, 182), (140, 140, 92), 140) if not a.small else ((23, 27, 22), (14, 14, 9), 16)
    frames = a.frames if not a.small else 5
    stream = torch.cuda.current_stream()
    fv2r = grid_vox2ras(fshape, 1.0)
    nvf = int(np.prod(fshape))
    res = dict(device=torch.cuda.get_device_name(0), lib=os.path.basename(fj.LIB_PATH), runs=RUNS, warmups=WARM, small=a.small,
               field=dict(shape=list(fshape), packed_bytes=16 * nvf))

    # ---- pack ----
    disp = smooth_field(fshape, fv2r, dev)
    packed = torch.empty((nvf, 4), dtype=torch.float32, device=dev)
    t = timed(lambda: warp.warp_pack_device(disp, fshape, out=packed, stream=stream))
    res["pack"] = dict(ms=t, bytes=28 * nvf, tb_per_s=28 * nvf / (t * 1e-3) / 1e12)
    print("pack", json.dumps(res["pack"]), flush=True)

    # ---- points: the C4 lines in a 1.3 mm volume that covers the field's grid, 12 degrees oblique ----
    xyz = c4_points(nline, dev)
    npnt = xyz.shape[0]
    lres = max(fshape) / float(nline)
    lv2r = grid_vox2ras((nline,) * 3, lres, 12.0)
    A, Q, B = warp.point_matrices(fv2r, lv2r, lv2r)
    out = torch.empty_like(xyz)
    t_warp = timed(lambda: warp.warp_points_device(packed, fshape, A, Q, B, xyz, out=out, stream=stream))
    x = fj.Xform(vox2vox=(B.astype(np.float64) @ A.astype(np.float64)).astype(np.float32))
    t_xfm = timed(lambda: fj.xfm_apply(x, xyz, out=out, stream=stream))
    q = torch.from_numpy(Q).to(dev)
    qv = xyz[:: max(1, npnt // 1000000)] @ q[:3, :3].T + q[:3, 3]
    inside = ((qv >= 0) & (qv <= torch.tensor([s - 1.0 for s in fshape], device=dev))).all(dim=1).float().mean().item()
    res["points"] = dict(points=npnt, warp_ms=t_warp, xfm_apply_ms=t_xfm, warp_over_xfm_apply=t_warp / t_xfm, gpoints_per_s=npnt / (t_warp * 1e-3) / 1e9,
                         stream_bytes=24 * npnt, gather_bytes_requested=128 * npnt, fraction_inside_the_field=inside)
    print("points", json.dumps(res["points"]), flush=True)
    del xyz, out, qv

    # ---- volume: a diffusion grid of 1.3 mm (as wide as the field's grid), 12 degrees oblique, pulled onto the field's grid ----
    dv2r = grid_vox2ras(dshape, fshape[0] / float(dshape[0]), 12.0)
    A, Q, B = warp.volume_matrices(fv2r, fv2r, dv2r)
    M = (B.astype(np.float64) @ A.astype(np.float64)).astype(np.float32)                 # the affine part: output voxel -> input voxel
    nvi = int(np.prod(dshape))
    res["volume"] = {}
    for nf in (1, frames):
        g = torch.Generator(device=dev).manual_seed(1)
        vol = torch.randn((nf, nvi), dtype=torch.float32, device=dev, generator=g)
        o = torch.empty((nf, nvf), dtype=torch.float32, device=dev)
        t_w = timed(lambda: warp.warp_volume_device(packed, fshape, A, Q, B, vol, dshape, fshape, outside=0, out=o, stream=stream))
        frac = float((o[0] != 0).float().mean().item())
        t_x = timed(lambda: fj.vol_xform_device(M, vol, dshape, fshape, outside=0, out=o, stream=stream))
        res["volume"]["%d frames" % nf] = dict(nframes=nf, warp_ms=t_w, vol_xform_ms=t_x, warp_over_vol_xform=t_w / t_x, inside_fraction=frac,
                                              in_bytes=4 * nvi * nf, out_bytes=4 * nvf * nf, field_gather_bytes_requested=128 * nvf)
        print("volume", nf, json.dumps(res["volume"]["%d frames" % nf]), flush=True)
        del vol, o

    # ---- invert, niter 20, onto the field's own grid ----
    Y, Qi = warp.invert_matrices(fv2r, fv2r)
    inv = torch.empty((3, nvf), dtype=torch.float32, device=dev)
    err = torch.empty(nvf, dtype=torch.float32, device=dev)
    t20 = timed(lambda: warp.warp_invert_device(packed, fshape, Y, Qi, fshape, niter=20, inv=inv, err=err, stream=stream))
    emax = float(err.max().item())
    t1 = timed(lambda: warp.warp_invert_device(packed, fshape, Y, Qi, fshape, niter=1, inv=inv, err=err, stream=stream))
    res["invert"] = dict(niter=20, ms=t20, niter1_ms=t1, voxels=nvf, err_max_mm=emax, gvoxel_iterations_per_s=21 * nvf / (t20 * 1e-3) / 1e9,
                         invert_over_pack=t20 / res["pack"]["ms"])
    print("invert", json.dumps(res["invert"]), flush=True)

    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "timings.json"), "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    p, v1, vn, iv = res["points"], res["volume"]["1 frames"], res["volume"]["%d frames" % frames], res["invert"]
    lines = ["# Non-linear warps: kernel times", "",
             "Written by tools/warp_time.py (%s, %s%s): HIP events, device-resident operands, the median of %d runs after %d warm-ups."
             % (res["device"], res["lib"], ", TOY SIZES" if a.small else "", RUNS, WARM),
             "Field %d x %d x %d, %.0f MB packed." % (fshape + (16 * nvf / 1e6,)), "",
             "| kernel | work | ms | neighbour | neighbour ms | ratio |", "|---|---|---|---|---|---|",
             "| fibd_warp_pack | %d voxels, 28 B each | %.4f | - | - | %.2f TB/s |" % (nvf, res["pack"]["ms"], res["pack"]["tb_per_s"]),
             "| fibd_warp_points | %d points (%.0f %% inside the field) | %.4f | fibd_xfm_apply | %.4f | %.2f |"
             % (p["points"], 100 * p["fraction_inside_the_field"], p["warp_ms"], p["xfm_apply_ms"], p["warp_over_xfm_apply"]),
             "| fibd_warp_volume | %d x %d x %d x 1 -> the field's grid | %.4f | fibd_vol_xform | %.4f | %.2f |"
             % (dshape + (v1["warp_ms"], v1["vol_xform_ms"], v1["warp_over_vol_xform"])),
             "| fibd_warp_volume | %d x %d x %d x %d -> the field's grid | %.4f | fibd_vol_xform | %.4f | %.2f |"
             % (dshape + (frames, vn["warp_ms"], vn["vol_xform_ms"], vn["warp_over_vol_xform"])),
             "| fibd_warp_invert | niter 20, %d voxels (niter 1: %.4f ms) | %.4f | fibd_warp_pack | %.4f | %.2f |"
             % (nvf, iv["niter1_ms"], iv["ms"], res["pack"]["ms"], iv["invert_over_pack"])]
    with open(os.path.join(a.out, "TIMINGS.md"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
