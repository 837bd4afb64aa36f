#!/usr/bin/env python3
"""Times of the registration (csrc/register.hip) on the headline 140^3 volume, device-resident inputs, HIP events on the launch stream,
the median of 7 runs after 2 warm-ups:
  reg_hist     one fibd_reg_hist launch of 12 jobs (the candidates theta +- step of a rigid search) at pyramid levels 0, 1 and 2, and at
               nbins 8 / 32 / 64 on level 0; beside it fibd_vol_xform, trilinear, on 12 frames of the same grid: the same gather
               without the count;
  mri_register the whole rigid registration of one frame (device tier: the pyramid, every launch, every read-back, every decision);
  dwi_moco     the whole motion correction of --frames frames (device tier of the search + the resampling; wall clock).
With the diagnostic build of the library (`make stamp`, FIBERS_HIP_LIB) both LDS schemes of the histogram kernel run:
FIBERS_REG_HIST_SCHEME=a is one histogram per workgroup, b a private copy per wave.  Writes timings.json and README.md into --out
(default profiles/register)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import fibers_jl_amd as fj  # noqa: E402

RUNS, WARM = 7, 2
GRID, RES = (140, 140, 140), (1.25, 1.25, 1.25)
reg = fj.register


def timed(fn, runs=RUNS, warm=WARM):
    for _ in range(warm):
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
    return statistics.median(ms)


def wall(fn, runs, warm):
    for _ in range(warm):
        fn()
    ms = []
    for _ in range(runs):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append(1e3 * (time.perf_counter() - t))
    return statistics.median(ms)


def geometry():
    V = np.eye(4)
    V[0, 0], V[1, 1], V[2, 2] = RES
    V[:3, 3] = -np.array(RES) * (np.array(GRID) - 1) / 2
    return V.astype(np.float32)


def phantom(dev):
    """a smooth head-like volume: a soft ellipsoid with off-centre blobs, float32 [nvox] (x fastest)"""
    ax = [torch.linspace(-1, 1, n, device=dev) for n in GRID]
    z, y, x = torch.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    r = torch.sqrt((x / 0.8) ** 2 + (y / 0.9) ** 2 + (z / 0.75) ** 2)
    v = torch.sigmoid((1 - r) * 12)
    for cx, cy, cz, s, w in ((0.3, 0.2, -0.1, 0.15, 0.9), (-0.3, 0.3, 0.1, 0.12, -0.5), (0.1, -0.4, 0.2, 0.2, 0.6), (-0.2, -0.2, -0.3, 0.14, 0.8),
                             (0.45, -0.1, 0.05, 0.1, -0.4), (-0.1, 0.45, -0.2, 0.17, 0.5)):
        v = v + w * torch.exp(-((x - cx) ** 2 + (y - cy) ** 2 + (z - cz) ** 2) / (2 * s * s)) * (r < 1)
    return (1000 * v).reshape(-1).contiguous()


def series(base, nframes, V, dev):
    """nframes frames of the phantom, each moved by a small rigid theta of its own; every 15th frame keeps the contrast (b = 0), the others
    are a non-linear remap of it"""
    rng = np.random.default_rng(7)
    out = torch.empty((nframes, base.numel()), dtype=torch.float32, device=dev)
    thetas = rng.uniform(-1, 1, (nframes, 6)) * np.array([1.5, 1.5, 1.5, 2.0, 2.0, 2.0])
    thetas[0] = 0
    for f in range(nframes):
        fj.vol_xform_device(reg.reg_matrix(thetas[f], V, GRID, V, 0), base, GRID, GRID, "trilinear", 0, out=out[f])
        if f % 15:
            out[f] = 900 * torch.exp(-1.3e-3 * out[f]) * (out[f] > 0) + 0.015 * out[f]
    bval = np.where(np.arange(nframes) % 15 == 0, 0.0, 1000.0).astype(np.float32)
    return out, thetas, bval


def residual_mm(theta, made_with, V):
    """a frame was made as base(G(made_with) x) and registered to the base: G(made_with) G(theta) should be the identity; the largest
    displacement it leaves at the corners of the grid, mm (the frames of the series are registered to a mean of moved frames, which has
    a motion of its own: that figure is an upper bound)"""
    Ga = reg.reg_matrix(made_with, V, GRID, V, 0, with_G=True)[1]
    Gb = reg.reg_matrix(theta, V, GRID, V, 0, with_G=True)[1]
    c = np.array([[i, j, k, 1.0] for i in (0, GRID[0] - 1) for j in (0, GRID[1] - 1) for k in (0, GRID[2] - 1)]) @ V.astype(np.float64).T
    return float(np.sqrt((((c @ (Ga @ Gb).T) - c)[:, :3] ** 2).sum(1)).max())


def write_readme(out):
    """README.md from the timings of the product and, where present, of the diagnostic build"""
    load = lambda n: json.load(open(os.path.join(out, n))) if os.path.exists(os.path.join(out, n)) else None  # noqa: E731
    prod, diag = load("timings.json"), load("timings_stamp.json")
    any_ = prod or diag
    lines = ["# Registration: kernel and whole-run times", "",
             "Written by tools/register_time.py (%s): HIP events, device-resident inputs, the median of %d runs after %d warm-ups, on the"
             % (any_["device"], RUNS, WARM),
             "headline %d^3 volume (a smooth phantom; the moving frames are a non-linear remap of it, each moved by a rigid motion of its own)." % GRID[0],
             "", "## One fibd_reg_hist launch of 12 jobs", "",
             "`a` is one LDS histogram per workgroup, `b` a private copy per wave (diagnostic build, FIBERS_REG_HIST_SCHEME); `shipped` is the",
             "product library.  `vol_xform 12 frames` is fibd_vol_xform, trilinear, on 12 frames of the same grid through one matrix (the same",
             "gather without the count; one launch), `vol_xform x 12` twelve launches of one frame each through the 12 matrices.", "",
             "| level | grid | nbins | a ms | b ms | shipped ms | vol_xform 12 frames ms | vol_xform x 12 ms |", "|---|---|---|---|---|---|---|---|"]
    for key in sorted((prod or diag)["hist"], key=lambda k: ((prod or diag)["hist"][k]["level"], (prod or diag)["hist"][k]["nbins"])):
        p, d = (prod or {}).get("hist", {}).get(key, {}), (diag or {}).get("hist", {}).get(key, {})
        r = p or d
        f = lambda v: "-" if v is None else "%.4f" % v  # noqa: E731
        lines.append("| %d | %s | %d | %s | %s | %s | %s | %s |" % (r["level"], " x ".join(str(v) for v in r["shape"]), r["nbins"], f(d.get("reg_hist_a_ms")),
                     f(d.get("reg_hist_b_ms")), f(p.get("reg_hist_shipped_ms")), f(r.get("vol_xform_12_frames_ms")), f(r.get("vol_xform_1_frame_x12_ms"))))
    if prod and prod.get("whole"):
        w = prod["whole"]
        lines += ["", "## Whole runs (device tier, wall clock with the read-backs and the host decisions)", ""]
        m = w["mri_register"]
        lines.append("- mri_register, dof 6, %d levels: **%.2f ms** for %d iterations (largest corner residual against the motion the frame was made with: %.2f mm)."
                     % (m["levels"], m["ms"], m["iterations"], m["residual_mm"]))
        if "dwi_moco" in w:
            m = w["dwi_moco"]
            lines.append("- dwi_moco of %d frames (searches batched into shared launches, then %d fibd_vol_xform launches): **%.0f ms** (wall clock, median of %d), %d iterations"
                         % (m["frames"], m["frames"], m["ms"], m["runs"], m["iterations_total"]))
            lines.append("  in all, at most %d for a frame; corner residual against each frame's own motion: median %.2f mm, largest %.2f mm (the target is a mean"
                         % (m["iterations_max"], m["residual_mm_median"], m["residual_mm_max"]))
            lines.append("  of moved frames and carries a motion of its own).")
    lines += ["", "NOTES.md beside this file has the comparison of the two LDS schemes over several runs and the accuracy figures that no test asserts."]
    with open(os.path.join(out, "README.md"), "w") as f:
        f.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "register"))
    ap.add_argument("--frames", type=int, default=270)
    ap.add_argument("--moco-runs", type=int, default=RUNS)
    ap.add_argument("--skip-moco", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    diagnostic = "stamp" in os.path.basename(fj.LIB_PATH)
    schemes = [("a", "a"), ("b", "b")] if diagnostic else [("shipped", None)]
    V = geometry()
    base = phantom(dev)
    mov, thetas, bval = series(base, max(12, a.frames if not a.skip_moco else 12), V, dev)
    stream = torch.cuda.current_stream()
    res = dict(device=torch.cuda.get_device_name(0), lib=os.path.basename(fj.LIB_PATH), runs=RUNS, warmups=WARM, grid=list(GRID), hist={}, whole={})

    # ---- one launch of 12 jobs per level, and the same gather without the count ----
    fixed_l, mov_l, shape = base, mov[:12].contiguous(), GRID
    for level in range(3):
        if level:
            fixed_l, mov_l, shape = reg.vol_halve_device(fixed_l, shape), reg.vol_halve_device(mov_l, shape), reg.halved(shape)
        step = 2.0 ** level * min(RES)                             # the candidates of a rigid search's first round at this level
        cands = []
        for i in range(6):
            for sg in (1.0, -1.0):
                th = np.zeros(6)
                th[i] = sg * (step if i < 3 else 1.0)
                cands.append(reg.reg_matrix(th, V, GRID, V, level))
        mats = np.stack(cands)
        for nbins in ((8, 32, 64) if level == 0 else (32,)):
            rf, rm = reg.vol_range_device(fixed_l, fixed_l.numel(), nbins), reg.vol_range_device(mov_l, mov_l.shape[1], nbins)
            out = torch.empty((12, nbins, nbins), dtype=torch.int32, device=dev)
            work = torch.empty(reg.reg_hist_work_size(12) // 8 + 1, dtype=torch.int64, device=dev)
            row = dict(level=level, shape=list(shape), nbins=nbins, njobs=12)
            for label, env in schemes:
                if env is not None:
                    os.environ["FIBERS_REG_HIST_SCHEME"] = env
                row["reg_hist_%s_ms" % label] = timed(lambda: reg.reg_hist_device(fixed_l, shape, rf, mov_l, shape, rm, [0] * 12, mats, nbins, out=out,
                                                                                   work=work, stream=stream))
            os.environ.pop("FIBERS_REG_HIST_SCHEME", None)
            row["counted_fraction"] = float(out[0].sum().item()) / fixed_l.numel()
            if nbins == 32:
                xo = torch.empty_like(mov_l)
                row["vol_xform_12_frames_ms"] = timed(lambda: fj.vol_xform_device(mats[0], mov_l, shape, shape, "trilinear", 0, out=xo, stream=stream))
                xo1 = torch.empty_like(fixed_l)
                row["vol_xform_1_frame_x12_ms"] = timed(lambda: [fj.vol_xform_device(mats[j], mov_l[0], shape, shape, "trilinear", 0, out=xo1, stream=stream)
                                                                 for j in range(12)])
            res["hist"]["level %d nbins %d" % (level, nbins)] = row
            print(json.dumps(row), flush=True)

    # ---- the whole registration of one frame, and of the series ----
    def one():
        return reg.mri_register_device(mov[1], GRID, V, base, GRID, RES, V, dof=6, nbins=32, stream=stream)
    r = one()[0]
    res["whole"]["mri_register"] = dict(ms=wall(one, RUNS, WARM), iterations=int(len(r[2])), levels=reg.reg_levels(GRID, GRID), cost=r[1],
                                        residual_mm=residual_mm(r[0], thetas[1], V))
    print(json.dumps(res["whole"]["mri_register"]), flush=True)
    if not a.skip_moco:
        nf = a.frames
        target = mov[torch.from_numpy(np.flatnonzero(bval[:nf] == 0)).to(dev)].double().mean(0).float().contiguous()
        out = torch.empty((nf, base.numel()), dtype=torch.float32, device=dev)

        def moco():
            rr = reg.mri_register_device(mov[:nf], GRID, V, target, GRID, RES, V, dof=6, nbins=32, stream=stream)
            for f, (th, _, _) in enumerate(rr):
                fj.vol_xform_device(reg.reg_matrix(th, V, GRID, V, 0), mov[f], GRID, GRID, "trilinear", 0, out=out[f], stream=stream)
            return rr
        rr = moco()
        resid = [residual_mm(x[0], thetas[f], V) for f, x in enumerate(rr)]
        res["whole"]["dwi_moco"] = dict(frames=nf, ms=wall(moco, a.moco_runs, WARM - 1), runs=a.moco_runs, iterations_total=int(sum(len(x[2]) for x in rr)),
                                        iterations_max=int(max(len(x[2]) for x in rr)), residual_mm_median=float(np.median(resid)),
                                        residual_mm_max=float(np.max(resid)))
        print(json.dumps(res["whole"]["dwi_moco"]), flush=True)

    os.makedirs(a.out, exist_ok=True)
    name = "timings_stamp.json" if diagnostic else "timings.json"
    with open(os.path.join(a.out, name), "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    write_readme(a.out)


if __name__ == "__main__":
    main()
