#!/usr/bin/env python3
"""Both LDS schemes of the joint-histogram kernel (csrc/register.hip) against the NumPy restatement, bit for bit.  The product library
ships one scheme; the diagnostic build (`make stamp` -> libfibers_hip_stamp.so) forces either through FIBERS_REG_HIST_SCHEME=a|b.  This
script loads the diagnostic build and runs the histogram cases of tests/test_gpu_register.py under both.  Prints "register check: ok"."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
os.environ["FIBERS_HIP_LIB"] = os.path.join(ROOT, "fibers.jl_amd", "libfibers_hip_stamp.so")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import fibers_jl_amd as fj  # noqa: E402
import register_ref as R  # noqa: E402
import volxform_ref as vref  # noqa: E402


def gpu_hist(fixed, moving, jobs, nbins):
    reg = fj.register
    fx = torch.from_numpy(fixed.reshape(-1)).cuda()
    mv = torch.from_numpy(moving.reshape(moving.shape[0], -1)).cuda()
    rf, rm = reg.vol_range_device(fx, fx.numel(), nbins), reg.vol_range_device(mv, mv.shape[1], nbins)
    h = reg.reg_hist_device(fx, fixed.shape[::-1], rf, mv, moving.shape[1:][::-1], rm, [f for f, _ in jobs], np.stack([M for _, M in jobs]), nbins)
    return h.cpu().numpy().view(np.uint32)


def main():
    assert "stamp" in os.path.basename(fj.LIB_PATH)
    cases = []
    fixed, moving = R.hist_volumes((13, 11, 9), (10, 12, 7), 3, seed=4)
    for njobs, nbins in ((1, 32), (12, 8), (13, 64)):
        cases.append((fixed, moving, R.hist_jobs(njobs, 3, vref.out2in(vref.oblique()), projective=True), nbins))
    for fshape in ((3, 2, 2), (70, 6, 10)):
        f2, m2 = R.hist_volumes(fshape, (11, 9, 8), 2, seed=5)
        s = np.diag([10.0 / fshape[0], 8.0 / fshape[1], 7.0 / fshape[2], 1.0]).astype(np.float32)
        cases.append((f2, m2, R.hist_jobs(5, 2, s), 32))
    want = [R.reg_hist(f, R.vol_range(f, nb), m, [R.vol_range(x, nb) for x in m], jobs, nb) for f, m, jobs, nb in cases]
    for scheme in ("a", "b"):
        os.environ["FIBERS_REG_HIST_SCHEME"] = scheme
        for i, ((f, m, jobs, nb), w) in enumerate(zip(cases, want)):
            got = gpu_hist(f, m, jobs, nb)
            if not np.array_equal(got, w):
                print("scheme %s, case %d: %d cells differ" % (scheme, i, int((got != w).sum())))
                return 1
            if got.sum() == 0:
                print("case %d counts nothing" % i)
                return 1
    print("register check: ok")
    return 0


if __name__ == "__main__":
    sys.exit(main())
