#!/usr/bin/env python3
"""fibd_st_recon on a device-resident 512 x 512 x 256 volume at (sigma, rho) = (1, 2) and (2, 4): hipEvent time per call after a
warm-up, Mvoxels/s, and the two byte models against 8 TB/s -- 76 B/voxel for this design (vol 4 + gradients written 12 and read 12
+ eigvec / eigval 48) and the 52 B/voxel floor of any design (vol in, outputs out).  Run it under
`rocprofv3 --kernel-trace --stats -- python tools/st_recon_time.py` for the K1 (st_grad_kernel) / K2 (st_tensor_kernel) split.
Prints one JSON line per setting."""
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import fibers_jl_amd as fj  # noqa: E402

SHAPE = (512, 512, 256)
ROOF = 8e12


def main():
    steps = int(os.environ.get("ST_RECON_STEPS", "20"))
    nx, ny, nz = SHAPE
    n = nx * ny * nz
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(3)
    vol = torch.randn(n, device=dev, generator=g)
    eigvec = torch.empty((9, n), device=dev)
    eigval = torch.empty((3, n), device=dev)
    L = fj.lib()
    for sigma, rho in ((1.0, 2.0), (2.0, 4.0)):
        nb = C.c_uint64()
        fj._lib.check(L.fibd_st_recon_work_size(nx, ny, nz, sigma, rho, C.byref(nb)))
        work = torch.empty(nb.value, dtype=torch.uint8, device=dev)
        st = torch.cuda.current_stream()

        def call():
            fj._lib.check(L.fibd_st_recon(vol.data_ptr(), nx, ny, nz, 0, nz, 0, nz, sigma, rho, eigvec.data_ptr(), eigval.data_ptr(),
                                          None, work.data_ptr(), nb.value, C.c_void_p(st.cuda_stream)))
        for _ in range(5):
            call()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(steps):
            call()
        b.record()
        b.synchronize()
        ms = a.elapsed_time(b) / steps
        sec = ms * 1e-3
        print(json.dumps({"shape": list(SHAPE), "sigma": sigma, "rho": rho, "calls": steps, "ms": round(ms, 4),
                          "mvox_per_s": round(n / sec / 1e6, 1),
                          "bytes_76_TBps": round(76 * n / sec / 1e12, 3), "frac_8TBps_76": round(76 * n / sec / ROOF, 4),
                          "bytes_52_TBps": round(52 * n / sec / 1e12, 3), "frac_8TBps_52": round(52 * n / sec / ROOF, 4),
                          "paper_ms_76_at_8TBps": round(76 * n / ROOF * 1e3, 3)}), flush=True)
        del work


if __name__ == "__main__":
    main()
