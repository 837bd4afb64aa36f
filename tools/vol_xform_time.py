#!/usr/bin/env python3
"""Kernel time of the volume resampling (fibd_vol_xform), device-resident operands, HIP events on the launch stream, the median of 7
runs after 2 warm-ups.  Every case goes through a 12 degree oblique rotation about the grid centre plus a shift:
  anat->diff   256^3 -> 140 x 140 x 92, nearest on int32 labels and trilinear on float32;
  diff->anat   140 x 140 x 92 -> 256^3, trilinear;
  series       140 x 140 x 92 x 198 frames onto the same grid, trilinear.
Beside each case two comparisons: device copies of the bytes the kernel must move (copy_out: a buffer of the output's size, read and
written; floor: the input read once and the output written once, timed as a copy of half their sum) and fibd_str_sample on as many
samples (random points inside the input volume).  With the diagnostic build of the library (`make stamp`, FIBERS_HIP_LIB) the
workgroup's A/B partner runs too: FIBERS_VOL_XFORM_TILE=0 selects the 256 x 1 row segment instead of the 64 x 4 tile.
Writes timings.json and README.md into --out (default profiles/vol_xform)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import fibers_jl_amd as fj  # noqa: E402

RUNS, WARM = 7, 2
ANAT, DIFF = (256, 256, 256), (140, 140, 92)


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


def out2in(inshape, outshape):
    """output -> input: the output grid's centre onto the input grid's, the fields of view matched, rotated by 12 degrees about the
    oblique axis (1, 2, 3) and shifted by (2.5, -1.5, 0.75) input voxels"""
    ax = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    t = np.deg2rad(12.0)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    Rm = np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * (K @ K)
    A = Rm * (np.array(inshape, float) / np.array(outshape, float))
    M = np.eye(4)
    M[:3, :3] = A
    M[:3, 3] = (np.array(inshape) - 1) / 2 - A @ ((np.array(outshape) - 1) / 2) + np.array([2.5, -1.5, 0.75])
    return M.astype(np.float32)


def copy_ms(nbytes, dev):
    n = max(1, nbytes // 4)
    a, b = torch.empty(n, dtype=torch.float32, device=dev), torch.empty(n, dtype=torch.float32, device=dev)
    a.zero_()
    return timed(lambda: b.copy_(a))


def case(name, inshape, outshape, nframes, interp, dtype, dev, variants, with_sample=True):
    nvi, nvo = int(np.prod(inshape)), int(np.prod(outshape))
    g = torch.Generator(device=dev).manual_seed(1)
    if dtype == torch.float32:
        vol = torch.randn((nframes, nvi), dtype=dtype, device=dev, generator=g)
    else:
        vol = torch.randint(0, 2036, (nframes, nvi), dtype=dtype, device=dev, generator=g)
    out = torch.empty((nframes, nvo), dtype=dtype, device=dev)
    M = out2in(inshape, outshape)
    stream = torch.cuda.current_stream()
    in_bytes, out_bytes = 4 * nvi * nframes, 4 * nvo * nframes
    res = dict(inshape=list(inshape), outshape=list(outshape), nframes=nframes, interp=interp, dtype=str(dtype).split(".")[1],
               in_bytes=in_bytes, out_bytes=out_bytes)
    for label, env in variants:
        if env is None:
            os.environ.pop("FIBERS_VOL_XFORM_TILE", None)
        else:
            os.environ["FIBERS_VOL_XFORM_TILE"] = env
        res["kernel_%s_ms" % label] = timed(lambda: fj.vol_xform_device(M, vol, inshape, outshape, interp=interp, outside=0, out=out, stream=stream))
    os.environ.pop("FIBERS_VOL_XFORM_TILE", None)
    res["inside_fraction"] = float((out != 0).float().mean().item())
    res["copy_out_ms"] = copy_ms(out_bytes, dev)
    res["floor_ms"] = copy_ms((in_bytes + out_bytes) // 2, dev)
    if with_sample and dtype == torch.float32:
        xyz = torch.rand((nvo, 3), dtype=torch.float32, device=dev, generator=g) * torch.tensor([s - 1.0 for s in inshape], device=dev) + 1.0
        sc = torch.empty((nvo, nframes), dtype=torch.float32, device=dev)
        res["str_sample_ms"] = timed(lambda: fj.str_sample_device(xyz, vol, inshape, out=sc, stream=stream))
    for label, _ in variants:
        res["kernel_%s_over_copy_out" % label] = res["kernel_%s_ms" % label] / res["copy_out_ms"]
        res["kernel_%s_over_floor" % label] = res["kernel_%s_ms" % label] / res["floor_ms"]
    print(name, json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "vol_xform"))
    ap.add_argument("--frames", type=int, default=198)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    diagnostic = "stamp" in os.path.basename(fj.LIB_PATH)
    variants = [("tile", None)] + ([("row", "0")] if diagnostic else [])
    cases = {}
    cases["anat->diff nearest int32"] = case("anat->diff nearest", ANAT, DIFF, 1, "nearest", torch.int32, dev, variants)
    cases["anat->diff trilinear"] = case("anat->diff trilinear", ANAT, DIFF, 1, "trilinear", torch.float32, dev, variants)
    cases["diff->anat trilinear"] = case("diff->anat trilinear", DIFF, ANAT, 1, "trilinear", torch.float32, dev, variants)
    cases["series %d frames trilinear" % a.frames] = case("series", DIFF, DIFF, a.frames, "trilinear", torch.float32, dev, variants)
    res = dict(device=torch.cuda.get_device_name(0), lib=os.path.basename(fj.LIB_PATH), runs=RUNS, warmups=WARM, cases=cases)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "timings.json"), "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    lines = ["# fibd_vol_xform: kernel times", "",
             "Written by tools/vol_xform_time.py (%s, %s): HIP events, device-resident operands, the median of %d runs after %d warm-ups."
             % (res["device"], res["lib"], RUNS, WARM),
             "Every case is a 12 degree oblique rotation about the grid centre plus a shift.  `copy out` is a device copy of a buffer of the",
             "output's size; `floor` a device copy that moves the input once and the output once; `str_sample` is fibd_str_sample on as many",
             "samples.  `tile` is the 64 x 4 workgroup the library ships, `row` the 256 x 1 one (diagnostic build only).", "",
             "| case | " + " | ".join("%s ms" % v for v, _ in variants) + " | copy out ms | floor ms | str_sample ms | "
             + " | ".join("%s / copy out" % v for v, _ in variants) + " | " + " | ".join("%s / floor" % v for v, _ in variants) + " |",
             "|---|" + "---|" * (3 + 3 * len(variants))]
    for name, c in cases.items():
        lines.append("| %s | " % name + " | ".join("%.4f" % c["kernel_%s_ms" % v] for v, _ in variants)
                     + " | %.4f | %.4f | %s | " % (c["copy_out_ms"], c["floor_ms"], "%.4f" % c["str_sample_ms"] if "str_sample_ms" in c else "-")
                     + " | ".join("%.2f" % c["kernel_%s_over_copy_out" % v] for v, _ in variants) + " | "
                     + " | ".join("%.2f" % c["kernel_%s_over_floor" % v] for v, _ in variants) + " |")
    with open(os.path.join(a.out, "README.md"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
