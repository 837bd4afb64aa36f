#!/usr/bin/env python3
"""Wall times of the single-device host forms of csrc/api.hip (caller-owned host arrays in and out, blocking copies from pageable
memory): the median of 7 calls after 2 warm-ups, one process, device 0.
  vol_xform, warp_volume   a 128^3 volume of 8 frames onto the same grid, trilinear (the warp under a 128^3 field);
  warp_points              4 M points under that field;
  warp_invert              that field onto its own grid, niter 20;
  st_recon                 a 128^3 volume, sigma 1, rho 2;
  st_eigen                 128^3 tensors;
  find_peaks, find_peaks_work   2 M ODFs on sphere_362 (--odfs).
fib_rumba_rec is left out: a whole-volume iteration of seconds whose host form is two copies around it.
Prints one JSON line per form and writes them all to --out.  --small runs the same calls on toy sizes (a rehearsal); --large on a 256^3
grid and 32 M points (8 x the voxels and points: where the default sizes take only a few milliseconds, a check that time follows size)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import fibers_jl_amd as fj  # noqa: E402

RUNS, WARM = 7, 2
F = np.float32


def timed(fn):
    ms = []
    for i in range(WARM + RUNS):
        t0 = time.perf_counter()
        rc = fn()
        t1 = time.perf_counter()
        if rc != 0:
            raise RuntimeError("error %d: %s" % (rc, fj.lib().fib_last_error().decode()))
        if i >= WARM:
            ms.append((t1 - t0) * 1e3)
    return dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="JSON file for the table")
    ap.add_argument("--odfs", type=int, default=2000000)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--large", action="store_true")
    a = ap.parse_args()
    L = fj.lib()
    n = 12 if a.small else (256 if a.large else 128)
    nframes, npoints, nodf = (3, 1000, 100) if a.small else (8, 32000000 if a.large else 4000000, a.odfs)
    nvox = n ** 3
    rng = np.random.default_rng(7)
    eye = (C.c_float * 16)(*np.eye(4, dtype=F).reshape(-1).tolist())
    shift = np.eye(4, dtype=F)
    shift[:3, 3] = (0.4, -0.3, 0.2)
    shift = (C.c_float * 16)(*shift.reshape(-1).tolist())
    z, y, x = np.meshgrid(*[np.arange(n, dtype=F)] * 3, indexing="ij")
    field = np.ascontiguousarray(np.stack([2 * np.sin(y / 6 + 0.3), 1.6 * np.cos(z / 7), 1.2 * np.sin((x + y) / 8)]), dtype=F)
    del x, y, z
    vol = rng.standard_normal((nframes, nvox)).astype(F)
    out = np.zeros_like(vol)
    pts = rng.uniform(0, n - 1, (npoints, 3)).astype(F)
    pout = np.zeros_like(pts)
    inv, err = np.zeros((3, nvox), F), np.zeros(nvox, F)
    evec, eval_ = np.zeros((9, nvox), F), np.zeros((3, nvox), F)
    S = [rng.standard_normal(nvox).astype(F) for _ in range(6)]
    Sp = (C.c_void_p * 6)(*[s.ctypes.data for s in S])
    verts = np.asfortranarray(fj.sphere_362.vertices, dtype=F)
    faces = np.asfortranarray(fj.sphere_362.faces, dtype=np.int32)
    nvert = fj.sphere_362.nvert
    odf = rng.random((nvert, nodf), dtype=F)
    top, nvalid = np.zeros((3, nodf), np.int32), np.zeros(nodf, np.int32)
    pk, isort = np.zeros((nvert, nodf), F), np.zeros((nvert, nodf), np.int32)
    fp, d = field.ctypes.data, (n, n, n)
    forms = [
        ("vol_xform", lambda: L.fib_vol_xform(0, shift, vol.ctypes.data, *d, nframes, 1, 0, out.ctypes.data, *d)),
        ("warp_volume", lambda: L.fib_warp_volume(0, fp, *d, eye, eye, eye, vol.ctypes.data, *d, nframes, 1, 0, out.ctypes.data, *d)),
        ("warp_points", lambda: L.fib_warp_points(0, fp, *d, eye, eye, eye, pts.ctypes.data, pout.ctypes.data, npoints)),
        ("warp_invert", lambda: L.fib_warp_invert(0, fp, *d, eye, eye, 20, inv.ctypes.data, err.ctypes.data, *d)),
        ("st_recon", lambda: L.fib_st_recon(0, vol.ctypes.data, *d, 1.0, 2.0, evec.ctypes.data, eval_.ctypes.data)),
        ("st_eigen", lambda: L.fib_st_eigen(0, Sp, nvox, evec.ctypes.data, eval_.ctypes.data)),
        ("find_peaks", lambda: L.fib_find_peaks(0, odf.ctypes.data, nodf, verts.ctypes.data, verts.shape[0], faces.ctypes.data, faces.shape[0],
                                                top.ctypes.data, nvalid.ctypes.data)),
        ("find_peaks_work", lambda: L.fib_find_peaks_work(0, odf.ctypes.data, nodf, verts.ctypes.data, verts.shape[0], faces.ctypes.data,
                                                          faces.shape[0], pk.ctypes.data, isort.ctypes.data, nvalid.ctypes.data)),
    ]
    res = dict(lib=os.path.basename(fj.LIB_PATH), runs=RUNS, warmups=WARM, small=a.small, large=a.large,
               sizes=dict(grid=n, frames=nframes, points=npoints, odfs=nodf), forms={})
    for name, fn in forms:
        res["forms"][name] = timed(fn)
        print(name, json.dumps(res["forms"][name]), flush=True)
    # the calls did their work: every output array was written
    for name, arr in (("out", out), ("pout", pout), ("inv", inv), ("evec", evec), ("eval", eval_), ("top", top), ("nvalid", nvalid), ("pk", pk),
                      ("isort", isort)):
        assert arr[-1].any() and arr[0].any(), "%s was not written" % name
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
