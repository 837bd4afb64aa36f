#!/usr/bin/env python3
"""Times of probabilistic ODF tracking (csrc/probtrack.hip), device-resident operands, HIP events, the median of 7 runs after 2 warm-ups,
on the GQI ODF (sphere_642: 321 directions) of the 140^3 x 270-frame phantom:
  table     fibd_prob_table, against a device copy that moves its bytes (1284 B read and 768 B written per voxel);
  prob      fibd_prob_run on the seeds of the ball mask with one sub-voxel offset (the deterministic tracer's benchmark seeds): total
            steps, points, ms; the two passes separately (the library's profile brackets: the count pass alone is what a tracer with
            scratch rows would run, the emit pass is the price of the replay); the row-gather rate steps x pitch x 2 B per pass;
  stream    fibd_stream_run on the same volume's three GQI peaks, the same seeds: the deterministic tracer as it was before this tool;
  host_form fib_prob_stream on the same ODF, mask and offset in pageable host arrays: the wall time of the call (table from chunks of the
            host ODF, both passes, the lines down into arrays the library allocates; fib_tract_free is outside).  --host-form-only
            runs this row alone and writes host_form.json.
With the diagnostic build of the library (`make stamp`, FIBERS_HIP_LIB) both lane mappings run: FIBERS_PROB_LANES=64 selects a wave per
line instead of 16 lanes per line.  Writes timings.json (timings_diagnostic.json under the diagnostic build) into --out (default
profiles/prob_stream); the README.md beside them is written by hand from the two."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time


sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import fibers_jl_amd as fj  # noqa: E402
from fibers_jl_amd import phantom  # noqa: E402

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


def prof_get(name):
    ms, n = C.c_double(0), C.c_int64(0)
    fj.lib().fib_profile_get(name.encode(), C.byref(ms), C.byref(n))
    return ms.value / max(n.value, 1)


def host_form(odf, bm, shape, sph, sub):
    """fib_prob_stream on host copies of the device operands; ms = the median wall time of RUNS calls after WARM"""
    import numpy as np
    from fibers_jl_amd import _lib
    L = fj.lib()
    vol = np.ascontiguousarray(odf.cpu().numpy())                          # [nvert, nvox] planar == MRI.vol memory
    m8 = np.ascontiguousarray(bm.reshape(-1).to(torch.uint8).cpu().numpy())
    U = np.ascontiguousarray(sph.vertices[: sph.nvert], np.float32)
    s = np.ascontiguousarray(sub.cpu().numpy())
    cosang = fj.ProbPlan(sph, 45, 0).cosang_thresh
    ms, res = [], {}
    for i in range(WARM + RUNS):
        out = _lib.TractOut()
        t0 = time.perf_counter()
        rc = L.fib_prob_stream(0, shape[0], shape[1], shape[2], vol.ctypes.data, U.shape[0], U.ctypes.data, m8.ctypes.data, None, s.ctypes.data,
                               s.shape[0], 3, max(shape), cosang, 0.5, 0.1, 1, 1, C.byref(out))
        t = (time.perf_counter() - t0) * 1e3
        _lib.check(rc)
        res = dict(lines=int(out.nlines), points=int(out.npoints))
        L.fib_tract_free(C.byref(out))
        if i >= WARM:
            ms.append(t)
    return dict(ms=statistics.median(ms), all_ms=ms, bytes_in=vol.nbytes + m8.nbytes, bytes_out=12 * res["points"] + 12 * res["lines"], **res)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "prob_stream"))
    ap.add_argument("--size", type=int, default=140)
    ap.add_argument("--runs", type=int, default=RUNS, help="timed runs per figure (1 with --warm 0: a short run to collect counters over)")
    ap.add_argument("--warm", type=int, default=WARM)
    ap.add_argument("--host-form-only", action="store_true", help="the host_form row alone, into host_form.json")
    a = ap.parse_args()
    globals().update(RUNS=a.runs, WARM=a.warm)
    dev = torch.device("cuda", 0)
    shape = (a.size,) * 3
    nvox = a.size ** 3
    sph = fj.sphere_642
    nvert, pitch = sph.nvert, fj.prob_row_pitch(sph.nvert)
    diagnostic = "stamp" in os.path.basename(fj.LIB_PATH)
    bval, bvec = phantom.scheme_gqi()
    dwi, _ = phantom.make_dwi_torch(shape, bval, bvec, seed=3, device=dev)
    bm = phantom.ball_mask_torch(shape, dev)
    o = fj.odf_rec_device(fj.OdfPlan("gqi", bval, bvec, sph, device=0), dwi, bm)
    del dwi
    res = dict(device=torch.cuda.get_device_name(0), lib=os.path.basename(fj.LIB_PATH), runs=RUNS, warmups=WARM, shape=list(shape), nvert=nvert,
               pitch=pitch)

    sub = torch.tensor([[0.1, -0.2, 0.3]], dtype=torch.float32, device=dev)
    if a.host_form_only:
        res["host_form"] = host_form(o["odf"], bm, shape, sph, sub)
        print("host_form", json.dumps(res["host_form"]), flush=True)
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "host_form.json"), "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)
            f.write("\n")
        return

    # ---- table
    table = torch.empty((nvox, pitch), dtype=torch.uint16, device=dev)
    t_tab = timed(lambda: fj.probtrack.prob_table_device(o["odf"], bm, out=table))
    nbytes = nvox * (4 * nvert + 2 * pitch)
    ca, cb = torch.empty(nbytes // 8, dtype=torch.float32, device=dev), torch.empty(nbytes // 8, dtype=torch.float32, device=dev)
    ca.zero_()
    t_copy = timed(lambda: cb.copy_(ca))
    del ca, cb
    res["table"] = dict(ms=t_tab, bytes=nbytes, gbs=nbytes / t_tab / 1e6, copy_same_bytes_ms=t_copy, over_copy=t_tab / t_copy,
                        table_gb=nvox * pitch * 2 / 1e9)
    print("table", json.dumps(res["table"]), flush=True)

    # ---- the deterministic tracer on the three peaks (the code path of the commit before probtrack.hip)
    seeds = torch.nonzero(bm).flatten()
    field, mout = fj.stream_field_device(o["peak"], f=o["qa"], f_thresh=0.03, mask=bm)
    sbuf = fj.StreamBuffers(dev)
    r = {}

    def det():
        r["r"] = fj.stream_device_run(field, shape, seeds, sub, buffers=sbuf)
    t_det = timed(det)
    res["stream_run_3peaks"] = dict(ms=t_det, seeds=int(seeds.numel()), lines=int(r["r"]["npts"].numel()), points=int(r["r"]["xyz"].shape[0]),
                                    mpoints_per_s=int(r["r"]["xyz"].shape[0]) / t_det / 1e3)
    print("stream_run", json.dumps(res["stream_run_3peaks"]), flush=True)
    odf = o["odf"]
    del field, mout, sbuf, o
    r.clear()

    # ---- fibd_prob_run
    plan = fj.ProbPlan(sph, 45, 0)
    pbuf = fj.StreamBuffers(dev)
    work = torch.empty(fj.prob_work_size(seeds.numel()) // 8 + 1, dtype=torch.int64, device=dev)
    L = fj.lib()
    res["prob_run"] = {}
    for label, env in [("lanes16", None)] + ([("lanes64", "64")] if diagnostic else []):
        if env is None:
            os.environ.pop("FIBERS_PROB_LANES", None)
        else:
            os.environ["FIBERS_PROB_LANES"] = env

        def prob():
            r["r"] = fj.probtrack.prob_stream_device(plan, table, shape, seeds, sub, 3, None, 0.5, rng_seed=1, buffers=pbuf, work=work)
        prob()                                                          # (sizes the buffers)
        t = timed(prob)
        L.fib_profile_enable(1)
        L.fib_profile_reset()
        for _ in range(min(3, RUNS)):
            prob()
        torch.cuda.synchronize()
        count_ms, emit_ms = prof_get("prob_trace_count"), prof_get("prob_trace_emit")
        L.fib_profile_enable(0)
        cnt = r["r"]["all_counts"].to(torch.int64)
        pts_all = int(cnt.sum().item())
        live = int((cnt.sum(dim=1) > 0).sum().item())
        steps1 = pts_all + 2 * live                                      # every saved point is a step that drew; each pass of a live line ends on one that did not
        kept = cnt.sum(dim=1) >= 3
        steps2 = int(cnt[kept].sum().item()) + 2 * int(kept.sum().item())
        res["prob_run"][label] = dict(ms=t, seeds=int(seeds.numel()), lines=int(r["r"]["npts"].numel()), points=int(r["r"]["xyz"].shape[0]),
                                      mpoints_per_s=int(r["r"]["xyz"].shape[0]) / t / 1e3, steps_count_pass=steps1, steps_emit_pass=steps2,
                                      count_pass_ms=count_ms, emit_pass_ms=emit_ms,
                                      row_gather_tbs_count_pass=steps1 * pitch * 2 / count_ms / 1e9 if count_ms else None,
                                      row_gather_tbs_emit_pass=steps2 * pitch * 2 / emit_ms / 1e9 if emit_ms else None)
        print(label, json.dumps(res["prob_run"][label]), flush=True)
    os.environ.pop("FIBERS_PROB_LANES", None)
    del table, pbuf, work, r

    res["host_form"] = host_form(odf, bm, shape, sph, sub)
    print("host_form", json.dumps(res["host_form"]), flush=True)

    os.makedirs(a.out, exist_ok=True)
    name = "timings_diagnostic" if diagnostic else "timings"
    with open(os.path.join(a.out, name + ".json"), "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
