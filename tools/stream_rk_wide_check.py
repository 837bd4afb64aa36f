#!/usr/bin/env python3
"""The WIDE form (64-bit voxel indices and gather offsets) of the trilinear tracker's RK2 / RK4 integrators (fib_stream_params.interp = 2, 3)
against the 32-bit form on SMALL fields, where the DIAGNOSTIC build can force it (FIBERS_STREAM_WIDE=1), as tools/stream_wide_check.py
does for the other modes: bit-identical lines with 1, 2 and 3 vectors per voxel, and lines that differ from the Euler form's.
Exit code 0 = all identical."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("FIBERS_HIP_LIB", os.path.join(ROOT, "fibers.jl_amd", "libfibers_hip_stamp.so"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import fibers_jl_amd as fj  # noqa: E402
from fibers_jl_amd import phantom  # noqa: E402


def main():
    dev = torch.device("cuda", 0)
    n = 36
    shape = (n, n, n)
    nvox = n ** 3
    g = torch.Generator(device=dev); g.manual_seed(3)
    base = torch.from_numpy(np.ascontiguousarray(phantom.fibre_field(n, n, n).astype(np.float32).reshape(nvox, 3, order="F").T)).to(dev)

    def vecs(k):
        v = base + 0.35 * k * torch.randn(base.shape, device=dev, generator=g)
        return (v / v.norm(dim=0, keepdim=True)).contiguous()
    mask = (torch.rand(nvox, device=dev, generator=g) < 0.95).to(torch.uint8)
    sub = torch.from_numpy(fj.make_sublist(2, np.random.default_rng(4))).to(dev)
    bad = 0
    for nvec in (1, 2, 3):
        field, mout = fj.stream_field_device([vecs(k) for k in range(nvec)], mask=mask)
        seeds = torch.nonzero(mout).flatten()
        os.environ.pop("FIBERS_STREAM_WIDE", None)
        euler = fj.stream_device(field, shape, seeds, sub, len_max=60, interp="trilinear")
        for integrator in ("rk2", "rk4"):
            os.environ.pop("FIBERS_STREAM_WIDE", None)
            a = fj.stream_device(field, shape, seeds, sub, len_max=60, interp="trilinear", integrator=integrator)
            os.environ["FIBERS_STREAM_WIDE"] = "1"
            b = fj.stream_device(field, shape, seeds, sub, len_max=60, interp="trilinear", integrator=integrator)
            os.environ.pop("FIBERS_STREAM_WIDE", None)
            torch.cuda.synchronize()
            same = all(torch.equal(a[k], b[k]) for k in ("npts", "seed_index", "xyz"))
            other = a["xyz"].shape != euler["xyz"].shape or not torch.equal(a["xyz"], euler["xyz"])
            print("%s, %d vector(s)   lines %7d points %9d  wide == 32-bit: %s  differs from Euler: %s"
                  % (integrator, nvec, int(a["npts"].numel()), int(a["xyz"].shape[0]), same, other), flush=True)
            bad += 0 if same and other and int(a["npts"].numel()) > 100 else 1
    print("stream rk wide check:", "ok" if bad == 0 else "%d FAILURES" % bad)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
