#!/usr/bin/env python3
"""Times of the non-linear registration (csrc/nlreg.hip) on a 140^3 pair, measured as tools/warp_time.py and tools/register_time.py
measure: HIP events on the launch stream, device-resident inputs, the median of 7 runs after 2 warm-ups, one process.  The fixed volume
is tools/register_time.py's head-like phantom on its grid (140^3 at 1.25 mm); the moving one is that volume pulled through a smooth
synthetic displacement (3 mm sines) by fibd_warp_volume.
  step      one fibd_nlreg_step at level 0 under a smooth current field, beside one fibd_warp_volume of one frame on the same grid and
            beside its HBM floor (the packed field in and out, one read of the fixed volume: 36 bytes a voxel);
  smooth    one fibd_warp_smooth (three passes) at sigma 1, beside a device copy of the packed field;
  upsample  fibd_warp_upsample 70^3 -> 140^3;  jacobian  fibd_warp_jacobian;  unpack  fibd_warp_unpack;
  mri_nlreg the whole estimate at the defaults (device tier: pyramid, ranges, every launch, one wait per level; wall clock), beside
            mri_register (dof 6) of the same pair.
Writes timings.json and README.md into --out (default profiles/nlreg).  --small runs the same code on toy sizes (a rehearsal: its
numbers are overheads)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

import fibers_jl_amd as fj  # noqa: E402
import register_time as rt  # noqa: E402
from warp_time import smooth_field  # noqa: E402

RUNS, WARM = rt.RUNS, rt.WARM
HBM_MEASURED_TBS = 6.29                     # the float4-copy rate of the MI355X, for the floor


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nlreg"))
    ap.add_argument("--small", action="store_true", help="toy sizes (a rehearsal of the code path, not a measurement)")
    a = ap.parse_args()
    if a.small:
        rt.GRID = (28, 24, 20)
    grid, res = rt.GRID, rt.RES
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream()
    nl, reg, warp = fj.nlreg, fj.register, fj.warp
    V = rt.geometry()
    nvox = int(np.prod(grid))
    out = dict(device=torch.cuda.get_device_name(0), lib=os.path.basename(fj.LIB_PATH), runs=RUNS, warmups=WARM, small=a.small, grid=list(grid),
               voxels=nvox)

    fixed = rt.phantom(dev)
    true = warp.warp_pack_device(smooth_field(grid, V, dev, 3.0), grid)
    A, Q, B = warp.volume_matrices(V, V, V)
    moving = warp.warp_volume_device(true, grid, A, Q, B, fixed, grid, grid, outside=0)
    packed = warp.warp_pack_device(smooth_field(grid, V, dev, 1.0), grid)             # a current field for the kernels below
    other, third = torch.empty_like(packed), torch.empty_like(packed)

    # ---- one iteration ----
    rng = [reg.range_table(reg.vol_range_device(v, nvox))[0][0] for v in (fixed, moving)]
    norm = (rng[0][0], np.float32(1) / np.float32(rng[0][1] - rng[0][0]), rng[1][0], np.float32(1) / np.float32(rng[1][1] - rng[1][0]))
    to_ras, from_ras, T, kappa = nl.nlreg_level(V, V, None, 0, min(res))
    cost = torch.zeros(2, dtype=torch.int64, device=dev)
    work = torch.empty(nl.nlreg_step_work_size(grid) // 8, dtype=torch.int64, device=dev)
    t_step = rt.timed(lambda: nl.nlreg_step_device(fixed, grid, moving, grid, norm, to_ras, from_ras, T, kappa, packed, out=other, cost=cost,
                                                   work=work, stream=stream))
    ssd, count = nl.cost_pair(cost)
    frame = torch.empty(nvox, dtype=torch.float32, device=dev)
    t_vol = rt.timed(lambda: warp.warp_volume_device(packed, grid, A, Q, B, moving, grid, grid, outside=0, out=frame, stream=stream))
    floor_ms = 36.0 * nvox / (HBM_MEASURED_TBS * 1e12) * 1e3
    out["step"] = dict(ms=t_step, warp_volume_ms=t_vol, step_over_warp_volume=t_step / t_vol, hbm_floor_ms=floor_ms, step_over_floor=t_step / floor_ms,
                       floor_bytes=36 * nvox, counted_fraction=count / nvox, cost=ssd / max(count, 1))
    print("step", json.dumps(out["step"]), flush=True)

    # ---- regularisation ----
    t_smooth = rt.timed(lambda: nl.warp_smooth_device(other, grid, 1.0, out=packed, work=third, stream=stream))
    t_copy = rt.timed(lambda: third.copy_(other))
    out["smooth"] = dict(sigma=1.0, scheme="three passes", ms=t_smooth, copy_ms=t_copy, smooth_over_copy=t_smooth / t_copy, pass_bytes=32 * nvox,
                         tb_per_s_per_pass=32 * nvox / (t_smooth / 3 * 1e-3) / 1e12)
    print("smooth", json.dumps(out["smooth"]), flush=True)

    # ---- between levels, the Jacobian map, the unpack ----
    half = reg.halved(grid)
    coarse = warp.warp_pack_device(smooth_field(half, V, dev, 1.0), half)
    t_up = rt.timed(lambda: nl.warp_upsample_device(coarse, half, grid, out=other, stream=stream))
    jac = torch.empty(nvox, dtype=torch.float32, device=dev)
    t_jac = rt.timed(lambda: nl.warp_jacobian_device(packed, grid, nl.jacobian_matrix(V), out=jac, stream=stream))
    planar = torch.empty((3, nvox), dtype=torch.float32, device=dev)
    t_unpack = rt.timed(lambda: nl.warp_unpack_device(packed, grid, out=planar, stream=stream))
    out["upsample"] = dict(ms=t_up, out_bytes=16 * nvox)
    out["jacobian"] = dict(ms=t_jac, bytes=20 * nvox, min_det=float(jac.min().item()))
    out["unpack"] = dict(ms=t_unpack, bytes=28 * nvox)
    print(json.dumps(dict(upsample=out["upsample"], jacobian=out["jacobian"], unpack=out["unpack"])), flush=True)

    # ---- the whole estimate at the defaults, beside the rigid registration of the same pair ----
    levels = reg.reg_levels(grid, grid)
    niter = [30] * levels
    wbuf = torch.empty(nl.nlreg_work_size(grid, grid, niter) // 8 + 2, dtype=torch.int64, device=dev)
    field = torch.empty((nvox, 4), dtype=torch.float32, device=dev)
    last = {}

    def whole():
        last["r"] = nl.mri_nlreg_device(moving, grid, V, fixed, grid, V, levels=levels, niter=30, sigma=1.0, step=min(res), out=field, work=wbuf,
                                        stream=stream)
    t_whole = rt.wall(whole, RUNS, WARM)
    cost_first, cost_last = float(last["r"][1][0, 0]), float(last["r"][1][-1, -1])
    nl.warp_jacobian_device(field, grid, nl.jacobian_matrix(V), out=jac)
    warped = warp.warp_volume_device(field, grid, A, Q, B, moving, grid, grid, outside=0)
    ok = (warped != 0) & (moving != 0)
    mse0 = float(((fixed - moving)[ok] ** 2).mean().item())
    mse1 = float(((fixed - warped)[ok] ** 2).mean().item())
    t_reg = rt.wall(lambda: reg.mri_register_device(moving, grid, V, fixed, grid, res, V, dof=6, nbins=32, stream=stream), RUNS, WARM)
    out["mri_nlreg"] = dict(ms=t_whole, levels=levels, niter=30, sigma=1.0, iterations=30 * levels, work_bytes=int(wbuf.numel() * 8),
                            cost_first=cost_first, cost_last=cost_last, mse_before=mse0, mse_after=mse1, mse_ratio=mse0 / mse1,
                            min_det=float(jac.min().item()), mri_register_ms=t_reg, nlreg_over_register=t_whole / t_reg)
    print("mri_nlreg", json.dumps(out["mri_nlreg"]), flush=True)

    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "timings.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    s, m, w = out["step"], out["smooth"], out["mri_nlreg"]
    lines = ["# Non-linear registration: kernel times", "",
             "Written by tools/nlreg_time.py (%s, %s%s): HIP events, device-resident operands, the median of %d runs after %d warm-ups; the whole"
             % (out["device"], out["lib"], ", TOY SIZES" if a.small else "", RUNS, WARM),
             "estimate is wall clock around a call that ends in a device synchronise.  Grid %d x %d x %d." % tuple(grid), "",
             "| what | ms | beside | ms | ratio |", "|---|---|---|---|---|",
             "| fibd_nlreg_step (level 0, %.0f %% of the voxels counted) | %.4f | fibd_warp_volume, 1 frame | %.4f | %.2f |"
             % (100 * s["counted_fraction"], s["ms"], s["warp_volume_ms"], s["step_over_warp_volume"]),
             "| | | HBM floor, 36 B a voxel at %.2f TB/s | %.4f | %.2f |" % (HBM_MEASURED_TBS, s["hbm_floor_ms"], s["step_over_floor"]),
             "| fibd_warp_smooth, sigma 1, three passes | %.4f | a device copy of the packed field | %.4f | %.2f |" % (m["ms"], m["copy_ms"], m["smooth_over_copy"]),
             "| fibd_warp_upsample, to this grid | %.4f | | | |" % out["upsample"]["ms"],
             "| fibd_warp_jacobian | %.4f | | | |" % out["jacobian"]["ms"],
             "| fibd_warp_unpack | %.4f | | | |" % out["unpack"]["ms"],
             "| mri_nlreg, %d levels x %d iterations, sigma 1 (wall) | %.3f | mri_register, dof 6 (wall) | %.3f | %.2f |"
             % (w["levels"], w["niter"], w["ms"], w["mri_register_ms"], w["nlreg_over_register"]), "",
             "The estimate: mean squared difference over the voxels present before and after %.4g -> %.4g (%.1f x), smallest Jacobian"
             % (w["mse_before"], w["mse_after"], w["mse_ratio"]),
             "determinant %.3f, cost %.3g at the first iteration of the coarsest level and %.3g at the last of level 0."
             % (w["min_det"], w["cost_first"], w["cost_last"]), "",
             "The tiled smoothing (a halo tile in LDS, two or three passes in one launch) is not built: there is one scheme to record."]
    with open(os.path.join(a.out, "README.md"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
