"""The device tier's argument contract (fibers.jl_amd/_dev.py) on the GPU: every `*_device` function rejects, in Python and before any
launch, a host tensor, a wrong element type, a strided view, a tensor on another device and a tensor that is one element short (or
long) of what the call reads or writes; and one function per family gives the same bytes on the current stream, on another torch
stream and on that stream's raw handle.

The shapes are the smallest the functions take: a 4 x 4 x 4 volume, 7 frames for DTI / ADC, 22 for DKI (1 + 10 + 11 on two shells:
the 22 unknowns), the 362-vertex sphere for the ODF plans, three lines of 5, 1 and 0 points, two models of 4 points.  Every valid
call is an exact fit, so "one short" is the smallest failing size.  An ArgError is the only pass: the library's own FibersError
would mean that the pointers had already left Python."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dki_ref  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPE, NVOX = (4, 4, 4), 64
NPTS = [5, 1, 0]
ONES = (1.0, 1.0, 1.0)


class Arg:
    """one tensor argument of a row: `size` is "exact" (the call fixes the element count: short and long must fail), "unit" (a whole
    multiple of something larger than one element: short and long break it), "min" (at least so many: only short fails) or "free"
    (the length IS a count the call takes from it -- npts, seeds, remap -- so no length is wrong on the host)"""

    def __init__(self, t, size="exact"):
        self.t, self.size = t, size


class Row:
    """a valid call: `call(**tensors)` with the tensors of `args`; `single`: no second tensor and no plan to disagree with"""

    def __init__(self, call, single=False, **args):
        self.call, self.single = call, single
        self.args = {k: v if isinstance(v, Arg) else Arg(v) for k, v in args.items()}

    def run(self, **swap):
        kw = {k: a.t for k, a in self.args.items()}
        kw.update(swap)
        return self.call(**kw)


@pytest.fixture(scope="module")
def torch_():
    import torch
    return torch


def _world(fj, torch, trk):
    """the inputs every row draws from: tables and plans, a fitted volume, a field, three lines, two models"""
    from fibers_jl_amd import phantom
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(11)
    w = dict(dev=dev, trk=trk)

    def up(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    def planar(bval, bvec, seed):
        dwi, _, _ = phantom.make_volume(SHAPE, bval, bvec, seed=seed)
        return up(np.asarray(dwi, np.float32).reshape(NVOX, -1, order="F").T)                      # [nvol, nvox]
    w["up"] = up
    w["mask"] = torch.ones(NVOX, dtype=torch.uint8, device=dev)
    b, g = phantom.scheme_dti(6, 1)
    w["dti"], w["adc"], w["dwi7"] = fj.DtiPlan(b, g), fj.DtiPlan(b), planar(b, g, 1)
    b, g = dki_ref.scheme(22)
    w["dki"], w["dwi22"] = fj.DkiPlan(b, g, fj.sphere_362), planar(b, g, 2)
    b, g = phantom.scheme_gqi(3, 20, (1000.0, 2000.0, 3000.0), 3)
    w["gqi"], w["dwi_gqi"] = fj.OdfPlan("gqi", b, g, fj.sphere_362), planar(b, g, 3)
    b, g = phantom.scheme_dsi()
    w["dsi"], w["dwi_dsi"] = fj.OdfPlan("dsi", b, g, fj.sphere_362, hann_width=32), planar(b, g, 4)
    b, g = phantom.scheme_gqi(3, 30, (1000.0, 2500.0), 3)
    w["rumba"], w["dwi_rumba"] = fj.RumbaPlan(b, g, fj.sphere_362), planar(b, g, 5)
    fit = fj.dti_fit_device(w["dti"], w["dwi7"], w["mask"])
    w["e1"], w["fa"] = fit["eigvec1"], fit["fa"]
    w["field"], w["fmask"] = fj.stream_field_device([w["e1"]], mask=w["mask"])
    w["seeds"] = torch.arange(NVOX, dtype=torch.int64, device=dev)
    w["sub"] = up(np.array([[0.1, -0.2, 0.3]], np.float32))
    w["xyz"] = up(rng.uniform(0.6, 3.4, (sum(NPTS), 3)).astype(np.float32))
    w["npts"] = up(np.array(NPTS, np.int32))
    w["lines"] = up(rng.uniform(0.6, 3.4, (3, 4, 3)).astype(np.float32))
    w["models"] = up(rng.uniform(0.6, 3.4, (2, 4, 3)).astype(np.float32))
    w["vol"] = up(rng.standard_normal(NVOX).astype(np.float32))
    torch.cuda.synchronize()
    return w


@pytest.fixture(scope="module")
def world(fj, torch_, tmp_path_factory):
    w = _world(fj, torch_, str(tmp_path_factory.mktemp("device_args") / "lines.trk"))
    yield w
    for k in ("dti", "adc", "dki", "gqi", "dsi", "rumba"):
        w[k].close()


def _rows(fj, torch, w):
    """name -> Row.  Outputs are passed wherever the function takes them, so that they are checked like the inputs."""
    dev = w["dev"]
    F, F64, I32, I64, U8, U32 = torch.float32, torch.float64, torch.int32, torch.int64, torch.uint8, torch.uint32

    def e(shape, dt=F):
        return torch.zeros(shape, dtype=I32 if dt == U32 else dt, device=dev).view(dt)
    xyz, npts, mask, field, seeds, sub = w["xyz"], w["npts"], w["mask"], w["field"], w["seeds"], w["sub"]
    npnt, nl = sum(NPTS), len(NPTS)
    rows = {}
    # ---- fits (plans) -----------------------------------------------------------------------------------------------------------
    from fibers_jl_amd.dti import DTI_FIELDS
    from fibers_jl_amd.dki import DKI_FIELDS, _nframes

    def dti(dwi, mask, **out):
        return fj.dti_fit_device(w["dti"], dwi, mask, out=out)
    rows["dti_fit_device"] = Row(dti, dwi=w["dwi7"], mask=mask, **{k: e((3, NVOX) if "vec" in k else NVOX) for k in DTI_FIELDS})
    rows["adc_fit_device"] = Row(lambda dwi, mask: fj.adc_fit_device(w["adc"], dwi, mask), dwi=w["dwi7"], mask=mask)

    def dki(dwi, mask, **out):
        return fj.dki_fit_device(w["dki"], dwi, mask, out=out)
    rows["dki_fit_device"] = Row(dki, dwi=w["dwi22"], mask=mask, **{k: e((_nframes(k), NVOX) if _nframes(k) > 1 else NVOX) for k in DKI_FIELDS})
    # ---- ODF plans --------------------------------------------------------------------------------------------------------------
    for kind in ("gqi", "dsi"):
        plan = w[kind]

        def odf(dwi, mask, odf, odfmax, p0, p1, p2, q0, q1, q2, pdf=None, plan=plan):
            out = dict(odf=odf, odfmax=odfmax, peak=[p0, p1, p2], qa=[q0, q1, q2])
            if pdf is not None:
                out["pdf"] = pdf
            return fj.odf_rec_device(plan, dwi, mask, out=out)
        extra = dict(pdf=e((plan.nvol, NVOX))) if kind == "dsi" else {}
        rows["odf_rec_device[%s]" % kind] = Row(odf, dwi=w["dwi_" + kind], mask=mask, odf=e((plan.nvert, NVOX)), odfmax=e(2), p0=e((3, NVOX)),
                                                p1=e((3, NVOX)), p2=e((3, NVOX)), q0=e(NVOX), q1=e(NVOX), q2=e(NVOX), **extra)
    rows["find_peaks_device"] = Row(lambda odf: fj.find_peaks_device(w["gqi"], odf), odf=Arg(e((w["gqi"].nvert, NVOX)) + 1.0, "unit"))
    for raw in (False, True):
        rows["qa_normalize_device[raw=%s]" % raw] = Row(lambda q0, q1, q2, odfmax, raw=raw: fj.qa_normalize_device([q0, q1, q2], odfmax, raw=raw),
                                                        q0=e(NVOX), q1=e(NVOX), q2=e(NVOX),
                                                        odfmax=Arg(e(2) + 1.0, "unit") if raw else Arg(e(1) + 1.0, "min"))

    def rumba(dwi, mask, fodf, fgm, fcsf, gfa, var, k0, k1, k2, k3, k4):
        out = dict(fodf=fodf, fgm=fgm, fcsf=fcsf, gfa=gfa, var=var, peak=[k0, k1, k2, k3, k4])
        return fj.rumba_rec_device(w["rumba"], dwi, mask, SHAPE, niter=2, out=out)
    rows["rumba_rec_device"] = Row(rumba, dwi=w["dwi_rumba"], mask=mask, fodf=e((w["rumba"].nvert, NVOX)), fgm=e(NVOX), fcsf=e(NVOX), gfa=e(NVOX),
                                   var=e(NVOX), **{"k%d" % k: e((3, NVOX)) for k in range(5)})
    # ---- tracer -----------------------------------------------------------------------------------------------------------------
    rows["angles_to_vectors_device"] = Row(lambda ang: fj.angles_to_vectors_device(ang), single=True, ang=Arg(e(NVOX), "free"))
    rows["stream_field_device"] = Row(lambda ovec, f, fa, mask: fj.stream_field_device([ovec], f=[f], fa=fa, mask=mask),
                                      ovec=Arg(w["e1"], "unit"), f=w["fa"], fa=w["fa"], mask=mask)
    kw = dict(len_min=2, len_max=8)
    rows["stream_device"] = Row(lambda field, seeds, sub: fj.stream_device(field, SHAPE, seeds, sub, **kw),
                                field=field, seeds=Arg(seeds, "free"), sub=Arg(sub, "unit"))
    rows["stream_device[lcms]"] = Row(lambda field, seeds, sub, lcms: fj.stream_device(field, SHAPE, seeds, sub, lcms=lcms, **kw),
                                      field=field, seeds=Arg(seeds, "free"), sub=Arg(sub, "unit"), lcms=e((10, NVOX)) + 0.1)
    rows["stream_device[xyz_out]"] = Row(lambda field, seeds, sub, into: fj.stream_device(field, SHAPE, seeds, sub, xyz_out=lambda n: into[:3 * n], **kw),
                                         field=field, seeds=Arg(seeds, "free"), sub=Arg(sub, "unit"), into=Arg(e(3 * NVOX * 64), "free"))
    rows["stream_device_run"] = Row(lambda field, seeds, sub: fj.stream_device_run(field, SHAPE, seeds, sub, **kw),
                                    field=field, seeds=Arg(seeds, "free"), sub=Arg(sub, "unit"))
    bufs = fj.stream_device_run(field, SHAPE, seeds, sub, **kw)["buffers"]
    rows["stream_device_run_enqueue"] = Row(lambda field, seeds, sub, counts: fj.stream_device_run_enqueue(field, SHAPE, seeds, sub, bufs, counts=counts, **kw),
                                            field=field, seeds=Arg(seeds, "free"), sub=Arg(sub, "unit"), counts=e(2, I64))
    ref = fj.MRI(np.zeros(SHAPE + (1,), np.uint8))
    rows["stream_to_trk"] = Row(lambda field, seeds, sub: fj.stream_to_trk(w["trk"], field, SHAPE, seeds, sub, ref, **kw),
                                field=field, seeds=Arg(seeds, "free"), sub=Arg(sub, "unit"))
    # ---- tract maps, selection, bundles -------------------------------------------------------------------------------------------
    nwork, nsel = fj.str_work_size(nl), fj.str_select_work_size(nl)
    assert nwork > 0 and nsel > 0

    def work(nbytes):
        return Arg(e((nbytes + 7) // 8, I64), "min")
    rows["str_density_device"] = Row(lambda xyz, npts, out, n_outside, work: fj.str_density_device(xyz, npts, SHAPE, out=out, n_outside=n_outside, work=work),
                                     xyz=Arg(xyz, "unit"), npts=Arg(npts, "free"), out=e(NVOX, U32), n_outside=e(1, I64), work=work(nwork))
    rows["str_sample_device"] = Row(lambda xyz, vol, out: fj.str_sample_device(xyz, vol, SHAPE, out=out),
                                    xyz=Arg(xyz, "unit"), vol=Arg(w["vol"], "unit"), out=e((npnt, 1)))
    rows["str_stats_device"] = Row(lambda xyz, npts, scalars, out, work: fj.str_stats_device(xyz, npts, ONES, scalars=scalars, out=out, work=work),
                                   xyz=Arg(xyz, "unit"), npts=Arg(npts, "free"), scalars=Arg(e((npnt, 2)), "unit"), out=e((nl, 3)), work=work(nwork))
    rows["str_roi_pack_device"] = Row(lambda rois, out: fj.str_roi_pack_device(rois, out=out), rois=Arg(e((2, NVOX), U8), "unit"), out=e(NVOX, U32))
    rows["str_select_device"] = Row(lambda xyz, npts, roibits, work: fj.str_select_device(xyz, npts, SHAPE, roibits=roibits, visit_all=1, work=work),
                                    xyz=Arg(xyz, "unit"), npts=Arg(npts, "free"), roibits=e(NVOX, U32), work=work(nsel))

    def gather(xyz, npts, keep, scalars, oxyz, onpts, oindex, oscalars, ocounts, work):
        return fj.str_gather_device(xyz, npts, keep, scalars=scalars, out=dict(xyz=oxyz, npts=onpts, index=oindex, scalars=oscalars, counts=ocounts), work=work)
    rows["str_gather_device"] = Row(gather, xyz=Arg(xyz, "unit"), npts=npts, keep=e(nl, U8) + 1, scalars=Arg(e((npnt, 2)), "unit"), oxyz=e((npnt, 3)),
                                    onpts=e(nl, I32), oindex=e(nl, I64), oscalars=e((npnt, 2)), ocounts=e(3, I64), work=work(nsel))

    def connectome(xyz, npts, labels, remap, counts, lengths, work):
        return fj.str_connectome_device(xyz, npts, SHAPE, labels, 2, remap=remap, volres=ONES, out=dict(counts=counts, lengths=lengths), work=work)
    rows["str_connectome_device"] = Row(connectome, xyz=Arg(xyz, "unit"), npts=Arg(npts, "free"), labels=e(NVOX, I32) + 1, remap=Arg(w["up"](np.array([0, 1, 2], np.int32)), "free"),
                                        counts=e((3, 3), U32), lengths=e((3, 3), F64), work=work(nsel))
    rows["str_resample_device"] = Row(lambda xyz, npts, flip, out, status, work: fj.str_resample_device(xyz, npts, ONES, 4, flip=flip, out=out, status=status, work=work),
                                      xyz=Arg(xyz, "unit"), npts=npts, flip=e(nl, U8), out=e((nl, 4, 3)), status=e(1, I64), work=work(nwork))
    rows["str_assign_device"] = Row(lambda lines, models: fj.str_assign_device(lines, models, ONES, 5.0, dist_all=True),
                                    lines=Arg(w["lines"], "unit"), models=Arg(w["models"], "unit"))
    rows["str_centroids_device"] = Row(lambda lines, label, flip, sums, counts: fj.str_centroids_device(lines, label, flip, 2, out=(sums, counts)),
                                       lines=w["lines"], label=e(3, I32), flip=e(3, U8), sums=e((2, 4, 3), F64), counts=e(2, U32))
    # ---- transforms, structure tensor -------------------------------------------------------------------------------------------
    rows["vol_xform_device"] = Row(lambda vol, out: fj.vol_xform_device(np.eye(4, dtype=np.float32), vol, SHAPE, SHAPE, out=out),
                                   vol=Arg(w["vol"], "unit"), out=e(NVOX))
    rows["xfm_apply"] = Row(lambda points, out: fj.xfm_apply(fj.Xform(), points, out=out), points=xyz, out=e((npnt, 3)))
    rows["st_eigen_device"] = Row(lambda s0, s1, s2, s3, s4, s5: fj.st_eigen_device([s0, s1, s2, s3, s4, s5]),
                                  s0=w["vol"], **{"s%d" % c: w["vol"] * (c + 1.0) for c in range(1, 6)})
    rows["st_recon_device"] = Row(lambda vol: fj.st_recon_device(vol, SHAPE, 1.0, 1.0), single=True, vol=Arg(w["vol"], "unit"))
    return rows


NAMES = ["adc_fit_device", "angles_to_vectors_device", "dki_fit_device", "dti_fit_device", "find_peaks_device", "odf_rec_device[dsi]",
         "odf_rec_device[gqi]", "qa_normalize_device[raw=False]", "qa_normalize_device[raw=True]", "rumba_rec_device", "st_eigen_device",
         "st_recon_device", "str_assign_device", "str_centroids_device", "str_connectome_device", "str_density_device", "str_gather_device",
         "str_resample_device", "str_roi_pack_device", "str_sample_device", "str_select_device", "str_stats_device", "stream_device",
         "stream_device[lcms]", "stream_device[xyz_out]", "stream_device_run", "stream_device_run_enqueue", "stream_field_device", "stream_to_trk", "vol_xform_device", "xfm_apply"]


@pytest.fixture(scope="module")
def rows(fj, torch_, world):
    r = _rows(fj, torch_, world)
    assert sorted(r) == NAMES
    return r


def test_the_table_covers_every_device_function(fj):
    """every public *_device name of the package has a row (xfm_apply is the device form of a function that takes both)"""
    public = sorted(n for n in dir(fj) if n.endswith("_device"))
    assert public and not [n for n in public if not any(r == n or r.startswith(n + "[") for r in NAMES)]


def _mutations(torch, a):
    """name -> tensor: what must be refused in place of the valid tensor `a.t`"""
    t = a.t
    other = {torch.float32: torch.float64, torch.float64: torch.float32, torch.int32: torch.int64, torch.int64: torch.int32,
             torch.uint8: torch.int8, torch.uint32: torch.int32}[t.dtype]
    m = {"a host tensor": t.cpu(), "%s for %s" % (other, t.dtype): t.view(torch.int32).to(other) if t.dtype == torch.uint32 else t.to(other)}
    if t.numel() > 1:                                         # (a tensor of one element is contiguous whatever its strides)
        m["a strided view"] = torch.zeros(tuple(t.shape) + (2 * t.element_size(),), dtype=torch.uint8, device=t.device).view(t.dtype)[..., 0]
        assert not m["a strided view"].is_contiguous() and m["a strided view"].shape == t.shape
    if a.size != "free":
        m["one element short"] = t.reshape(-1)[:-1].clone()
    if a.size in ("exact", "unit"):
        b = t.reshape(-1).view(torch.uint8)                   # (bytes: torch.cat does not take every element type)
        m["one element long"] = torch.cat([b, b[:t.element_size()]]).view(t.dtype)
    return m


@pytest.mark.parametrize("name", NAMES)
def test_valid_call_runs_and_every_mutation_is_refused_in_python(fj, torch_, rows, name):
    from fibers_jl_amd._dev import ArgError
    row = rows[name]
    row.run()                                                 # the builder is valid (and an exact fit): what follows fails for the mutation alone
    torch_.cuda.synchronize()
    passed = []
    for arg, a in row.args.items():
        for what, bad in _mutations(torch_, a).items():
            try:
                row.run(**{arg: bad})
            except ArgError:
                continue
            passed.append("%s: %s" % (arg, what))             # (any other exception propagates: it is not a rejection in Python)
    assert not passed, "%s accepted %s" % (name, passed)


def test_a_tensor_on_a_second_device_is_refused(fj, torch_, rows):
    """among the tensors of one call, and against plan.device (every plan here is on device 0)"""
    if torch_.cuda.device_count() < 2:
        pytest.skip("needs two devices")
    from fibers_jl_amd._dev import ArgError
    passed = []
    for name, row in rows.items():
        if row.single:
            continue
        for arg, a in row.args.items():
            try:
                row.run(**{arg: a.t.to("cuda:1")})
            except ArgError:
                continue
            passed.append("%s: %s" % (name, arg))
    assert not passed, passed


def test_buffers_and_a_short_xyz_out_are_refused(fj, torch_, world):
    """what the table cannot mutate as a tensor argument: a caller's StreamBuffers that live elsewhere (here: on the host), and an
    `xyz_out` that returns one element less than the points need"""
    from fibers_jl_amd._dev import ArgError
    field, seeds, sub, kw = world["field"], world["seeds"], world["sub"], dict(len_min=2, len_max=8)
    host = fj.StreamBuffers("cpu", 64, 512)
    with pytest.raises(ArgError):
        fj.stream_device_run(field, SHAPE, seeds, sub, buffers=host, **kw)
    with pytest.raises(ArgError):
        fj.stream_device_run_enqueue(field, SHAPE, seeds, sub, host, **kw)
    npnt = fj.stream_device(field, SHAPE, seeds, sub, **kw)["xyz"].shape[0]
    assert npnt > 0
    fj.stream_device(field, SHAPE, seeds, sub, xyz_out=lambda n: torch_.zeros(3 * n, device=world["dev"]), **kw)          # the exact fit
    with pytest.raises(ArgError):
        fj.stream_device(field, SHAPE, seeds, sub, xyz_out=lambda n: torch_.zeros(3 * n - 1, device=world["dev"]), **kw)


# ---- streams ----------------------------------------------------------------------------------------------------------------------
def _flat(torch, r):
    """the tensors of a result (a tensor, or a tuple / list / dict of them, None and StreamBuffers left out), in a fixed order"""
    if isinstance(r, torch.Tensor):
        return [r]
    if isinstance(r, dict):
        return [t for k in sorted(r) for t in _flat(torch, r[k])]
    if isinstance(r, (tuple, list)):
        return [t for x in r for t in _flat(torch, x)]
    return []


FAMILIES = {"fit": "dti_fit_device", "odf": "odf_rec_device[gqi]", "tracer": "stream_device_run", "tract map": "str_density_device",
            "selection": "str_select_device", "bundle": "str_resample_device", "volume transform": "vol_xform_device",
            "point transform": "xfm_apply", "structure tensor": "st_eigen_device", "structure tensor (scratch)": "st_recon_device"}


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_the_three_kinds_of_stream_give_the_same_bytes(fj, torch_, world, family):
    """stream=None, a torch stream that is not current, and that stream's raw handle.  The functions that take caller's scratch get
    none here, so the raw handle goes through the launch context's wait.  (Bytes, not values: a line without points resamples to
    NaN rows, and torch.equal on the uint8 view compares them too.)"""
    torch = torch_
    name = FAMILIES[family]
    side = torch.cuda.Stream(world["dev"])
    got = []
    for stream in (None, side, C.c_void_p(side.cuda_stream)):
        row = _rows(fj, torch, world)[name]                   # fresh outputs for every kind
        kw = {k: a.t for k, a in row.args.items() if k != "work"}
        torch.cuda.synchronize()                              # the inputs are ready on every stream
        r = _stream_call(fj, torch, world, name, kw, stream)
        torch.cuda.synchronize()
        got.append([t.clone() for t in _flat(torch, r)])
    assert len(got[0]) >= 1 and len(got[0]) == len(got[1]) == len(got[2])
    for k, a in enumerate(got[0]):
        for other in (got[1][k], got[2][k]):
            assert a.dtype == other.dtype and a.shape == other.shape
            assert torch.equal(a.contiguous().view(-1).view(torch.uint8), other.contiguous().view(-1).view(torch.uint8)), (family, k)


def _stream_call(fj, torch, w, name, kw, stream):
    if name == "dti_fit_device":
        return fj.dti_fit_device(w["dti"], kw["dwi"], kw["mask"], stream=stream)
    if name == "odf_rec_device[gqi]":
        return fj.odf_rec_device(w["gqi"], kw["dwi"], kw["mask"], stream=stream)
    if name == "stream_device_run":
        r = fj.stream_device_run(kw["field"], SHAPE, kw["seeds"], kw["sub"], len_min=2, len_max=8, stream=stream)
        return {k: r[k] for k in ("npts", "seed_index", "xyz")}
    if name == "str_density_device":
        return fj.str_density_device(kw["xyz"], kw["npts"], SHAPE, stream=stream)
    if name == "str_select_device":
        return fj.str_select_device(kw["xyz"], kw["npts"], SHAPE, roibits=kw["roibits"], visit_none=1, stream=stream)
    if name == "str_resample_device":
        return fj.str_resample_device(kw["xyz"], kw["npts"], ONES, 4, stream=stream)
    if name == "vol_xform_device":
        M = np.array([[0.9, 0.1, 0, 0.2], [-0.1, 0.9, 0, 0.1], [0, 0, 1, 0.3], [0, 0, 0, 1]], np.float32)
        return fj.vol_xform_device(M, kw["vol"], SHAPE, SHAPE, stream=stream)
    if name == "xfm_apply":
        return fj.xfm_apply(fj.Xform(vox2vox=np.diag([2.0, 0.5, 1.5, 1.0]).astype(np.float32)), kw["points"], stream=stream)
    if name == "st_eigen_device":
        return fj.st_eigen_device([kw["s%d" % c] for c in range(6)], stream=stream)
    assert name == "st_recon_device"
    return fj.st_recon_device(kw["vol"], SHAPE, 1.0, 1.0, stream=stream, S_out=True)
