#!/usr/bin/env python3
"""Digests of everything the ODF step's launch path writes, with whatever library FIBERS_HIP_LIB names: one JSON line per case with a
SHA-256 of every output tensor.  Each case runs twice in the process; "repeatable" says whether both runs gave the same digests (where
they did not, "maxdiff" holds the largest absolute difference between the two runs of each tensor, and the case cannot be compared by
digest).  Two libraries compute the same bytes iff their lines are identical: run the tool once per library, one process each, and
compare the files (profiles/odf_step/README.md).

    tools/odf_step_digest.py [--no-bench] [--out FILE]

Cases: every configuration of tests/test_gpu_odf.py::test_which_kernels_a_configuration_runs under four flag sets and three masks, with a
NaN, a +Inf and a -Inf sample in known voxels (so the redo and repair lists are not empty); find_peaks_device on the three spheres; the
three forms of qa_normalize_device; rumba_rec_device on 12^3 voxels for 5 iterations (fib::matrix_plan_run with and without
recompaction); the two benchmark shapes (140^3 x 270 GQI, 140^3 x 515 DSI on sphere_642; all-ones mask and ball mask), the only shapes
at which the persistent grids are the CU count and not the item count.  Tensors of more than 64 MiB are hashed on the device first (a
position-weighted wrapping 64-bit sum and a plain one over the raw words) and the SHA-256 is taken of that."""
import hashlib, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import fibers_jl_amd as fj
from fibers_jl_amd import phantom

dev = torch.device("cuda", 0)
BIG = 64 << 20


def digest(t):
    t = t.contiguous()
    if t.numel() * t.element_size() <= BIG:
        return hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()
    w = t.view(-1).view(torch.int32)
    acc = torch.zeros(2, dtype=torch.int64, device=t.device)
    step = 1 << 26
    for i0 in range(0, w.numel(), step):                    # (int64 products wrap: a checksum modulo 2^64)
        x = w[i0:i0 + step].to(torch.int64)
        pos = torch.arange(i0, i0 + x.numel(), dtype=torch.int64, device=t.device)
        acc[0] += (x * (pos * -7046029254386353131 + 1)).sum()
        acc[1] += x.sum()
    return hashlib.sha256(acc.cpu().numpy().tobytes()).hexdigest()


def flat(out):
    """dict of tensors / lists of tensors / floats -> {name: tensor}"""
    r = {}
    for k, v in out.items():
        if isinstance(v, (list, tuple)):
            for i, t in enumerate(v):
                r["%s%d" % (k, i)] = t
        elif torch.is_tensor(v):
            r[k] = v
        else:
            r[k] = torch.tensor([float(v)], dtype=torch.float64)
    return r


def report(fh, name, run):
    """run() -> dict of outputs; called twice"""
    a = {k: v.clone() for k, v in flat(run()).items()}
    torch.cuda.synchronize()
    da = {k: digest(v) for k, v in a.items()}
    b = flat(run())
    torch.cuda.synchronize()
    db = {k: digest(v) for k, v in b.items()}
    line = dict(case=name, repeatable=da == db, sha256=da)
    if da != db:
        nn = lambda t: t.double().nan_to_num(nan=-7.0, posinf=-8.0, neginf=-9.0)      # noqa: E731
        line["maxdiff"] = {k: float((nn(a[k]) - nn(b[k])).abs().max()) for k in a if da[k] != db[k]}
    fh.write(json.dumps(line, sort_keys=True) + "\n")
    fh.flush()


def rec_outputs(plan, nvox, prezeroed):
    fill = (lambda *s: torch.zeros(*s, device=dev)) if prezeroed else (lambda *s: torch.full(s, float("nan"), device=dev))
    out = dict(odf=fill(plan.nvert, nvox), peak=[fill(3, nvox) for _ in range(3)], qa=[fill(nvox) for _ in range(3)], odfmax=fill(2))
    if plan.kind == "dsi":
        out["pdf"] = fill(plan.nvol, nvox)
    return out


FLAGS = dict(norm=dict(normalize=True), nonorm=dict(normalize=False), prezeroed=dict(normalize=True, out_prezeroed=True),
             raw=dict(normalize=False, raw_odfmax=True))

# the table of tests/test_gpu_odf.py::test_which_kernels_a_configuration_runs
ROUTES = [("gqi", "sphere_642", (20, 2), "fp16x2", (8, 8, 8), None), ("gqi", "sphere_642", (20, 2), "bf16x3", (8, 8, 8), None),
          ("gqi", "sphere_642", (20, 2), "fp16x2", (8, 8, 8), "separate"), ("gqi", "sphere_642", (20, 2), "fp16x2", (9, 7, 5), None),
          ("gqi", "sphere_642", (20, 2), "fp16x2", (8, 8, 8), "unaligned"), ("gqi", "sphere_642", (20, 2), "f32", (8, 8, 8), None),
          ("gqi", "sphere_642", (20, 1), "fp16x2", (8, 8, 8), None), ("gqi", "sphere_642", (12, 1), "fp16x2", (8, 8, 8), None),
          ("gqi", "sphere_362", (20, 2), "fp16x2", (8, 8, 8), None), ("dsi", "sphere_642", None, "fp16x2", (8, 8, 8), None),
          ("dsi", "sphere_642", None, "fp16x2", (8, 8, 8), "separate"), ("dsi", "sphere_642", None, "fp16x2", (9, 7, 5), None),
          ("dsi", "sphere_642", None, "f32", (8, 8, 8), None), ("dsi", "sphere_362", None, "fp16x2", (8, 8, 8), None)]


def route_cases(fh):
    for kind, sphere, frames, fmt, shape, extra in ROUTES:
        sph = getattr(fj, sphere)
        nvox = int(np.prod(shape))
        bval, bvec = phantom.scheme_dsi() if kind == "dsi" else phantom.scheme_gqi(1, frames[0], (1000.0, 2000.0)[:frames[1]], 3)
        dwi, _ = phantom.make_dwi_torch(shape, bval, bvec, seed=9, device=dev)
        dwi[3, 5] = float("nan"); dwi[7, 100] = float("inf"); dwi[2, 200] = -float("inf")
        g = torch.Generator(device=dev); g.manual_seed(5)
        masks = dict(ones=torch.ones(nvox, dtype=torch.uint8, device=dev),
                     rand30=(torch.rand(nvox, device=dev, generator=g) < 0.3).to(torch.uint8),
                     empty=torch.zeros(nvox, dtype=torch.uint8, device=dev))
        masks["rand30"][[5, 100, 200]] = 1
        plan = fj.OdfPlan(kind, bval, bvec, sph, hann_width=32, format=fmt)
        for mname, mask in masks.items():
            for fname, kw in FLAGS.items():
                def run():
                    out = rec_outputs(plan, nvox, kw.get("out_prezeroed", False))
                    if extra == "unaligned":
                        big = torch.full((sph.nvert * nvox + 4,), 0.0 if kw.get("out_prezeroed") else float("nan"), device=dev)
                        out["odf"] = big[1:1 + sph.nvert * nvox].view(sph.nvert, nvox)
                    return fj.odf_rec_device(plan, dwi, mask, out=out, separate_peaks=extra == "separate", **kw)
                frm = "dsi515" if kind == "dsi" else "1+%d" % (frames[0] * frames[1])
                report(fh, "rec/%s/%s/%s/%s/%dx%dx%d/%s/%s/%s" % ((kind, sphere, frm, fmt) + shape + (extra or "-", mname, fname)), run)
        plan.close()


def peaks_cases(fh):
    bval, bvec = phantom.scheme_gqi(1, 20, (1000.0, 2000.0), 3)
    for sphere in ("sphere_362", "sphere_642", "sphere_724"):
        sph = getattr(fj, sphere)
        plan = fj.OdfPlan("gqi", bval, bvec, sph)
        g = torch.Generator(device=dev); g.manual_seed(21)
        odf = torch.rand((sph.nvert, 1003), device=dev, generator=g)
        odf[:, 7] = 0.5                                     # a voxel of ties
        odf[3, 9] = float("nan")

        def run():
            top, nvalid = fj.find_peaks_device(plan, odf)
            return dict(top=top, nvalid=nvalid)
        report(fh, "find_peaks/%s" % sphere, run)
        plan.close()


def qa_cases(fh):
    g = torch.Generator(device=dev); g.manual_seed(4)
    base = [torch.rand(100003, device=dev, generator=g) for _ in range(3)]
    forms = dict(scalar=lambda qa: fj.qa_normalize_device(qa, 3.5),
                 dev=lambda qa: fj.qa_normalize_device(qa, torch.tensor([3.5, 0.0], device=dev)),
                 pair=lambda qa: fj.qa_normalize_device(qa, torch.tensor([3.5, 0.0], device=dev), raw=True),
                 pair_nan=lambda qa: fj.qa_normalize_device(qa, torch.tensor([3.5, 1.0], device=dev), raw=True))
    for name, f in forms.items():
        def run():
            qa = [t.clone() for t in base]
            f(qa)
            return dict(qa=qa)
        report(fh, "qa_normalize/%s" % name, run)


def rumba_case(fh):
    shape = (12, 12, 12)
    bval, bvec = phantom.scheme_gqi(3, 20, (1000.0, 2000.0, 3000.0), 3)
    dwi, _ = phantom.make_dwi_torch(shape, bval, bvec, seed=13, device=dev)
    g = torch.Generator(device=dev); g.manual_seed(6)
    mask = (torch.rand(12 ** 3, device=dev, generator=g) < 0.8).to(torch.uint8)
    plan = fj.RumbaPlan(bval, bvec, fj.sphere_724)
    report(fh, "rumba/12x12x12/5it", lambda: fj.rumba_rec_device(plan, dwi, mask, shape, niter=5))
    plan.close()


def bench_cases(fh):
    shape = (140, 140, 140)
    nvox = 140 ** 3
    masks = dict(ones=torch.ones(nvox, dtype=torch.uint8, device=dev), ball=phantom.ball_mask_torch(shape, dev))
    for kind in ("gqi", "dsi"):
        bval, bvec = phantom.scheme_gqi() if kind == "gqi" else phantom.scheme_dsi()
        dwi, _ = phantom.make_dwi_torch(shape, bval, bvec, seed=3, device=dev)
        dwi[3, 5 + 140 * 70 + 19600 * 70] = float("nan"); dwi[7, 100 + 140 * 70 + 19600 * 70] = float("inf")
        plan = fj.OdfPlan(kind, bval, bvec, fj.sphere_642, sigma=1.25, hann_width=32)
        out = rec_outputs(plan, nvox, False)
        for mname, mask in masks.items():
            report(fh, "bench/%s/140x140x140/%s" % (kind, mname), lambda: fj.odf_rec_device(plan, dwi, mask, out=out, normalize=True))
        plan.close()
        del dwi, out
        torch.cuda.empty_cache()


def main():
    args = sys.argv[1:]
    fh = sys.stdout
    if "--out" in args:
        fh = open(args[args.index("--out") + 1], "w")
    route_cases(fh)
    peaks_cases(fh)
    qa_cases(fh)
    rumba_case(fh)
    if "--no-bench" not in args:
        bench_cases(fh)
    if fh is not sys.stdout:
        fh.close()
    print("odf_step_digest: done (%s)" % os.path.basename(os.environ.get("FIBERS_HIP_LIB", "libfibers_hip.so")), flush=True)


if __name__ == "__main__":
    main()
