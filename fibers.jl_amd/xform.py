"""Transforms between volume spaces (util.jl:126-454) and the two `Tract` operations on them, `str_xform` and `str_merge`
(trk.jl:275-347).

An `Xform` holds the reference's nine fields in float32 (`xfm_read`'s default T = Float32).  The matrices this module derives --
inverses, products, the SVD behind `voxrot` -- are computed in float64 from the float32 fields and rounded to float32 once (the
reference does them in Float32 through LAPACK/BLAS, whose operation order is not reproduced).  The per-point apply,
the hot path, is HIP (csrc/xform.hip): a NumPy array goes through the host-buffer entry fib_xfm_apply, a CUDA tensor through
fibd_xfm_apply on the caller's stream.  Only the integer-output form of `xfm_apply!` (round, ties to even) is evaluated here."""
from dataclasses import dataclass, field, replace

import numpy as np

from . import _host, _lib
from ._dev import ArgError, Launch, tensor
from .mri import MRI
from .tract import Tract


def _m4():
    return np.eye(4, dtype=np.float32)


@dataclass
class Xform:
    """`Xform{Float32}` (util.jl:126-137).  Sizes are int vectors of 3, resolutions float32 vectors of 3, matrices float32."""
    insize: np.ndarray = field(default_factory=lambda: np.zeros(3, np.int64))    # input volume dimensions
    outsize: np.ndarray = field(default_factory=lambda: np.zeros(3, np.int64))   # output volume dimensions
    inres: np.ndarray = field(default_factory=lambda: np.ones(3, np.float32))     # input voxel size
    outres: np.ndarray = field(default_factory=lambda: np.ones(3, np.float32))    # output voxel size
    invox2ras: np.ndarray = field(default_factory=_m4)     # voxel -> RAS of the input volume
    outvox2ras: np.ndarray = field(default_factory=_m4)    # voxel -> RAS of the output volume
    vox2vox: np.ndarray = field(default_factory=_m4)       # input voxel -> output voxel
    ras2ras: np.ndarray = field(default_factory=_m4)       # input RAS -> output RAS
    voxrot: np.ndarray = field(default_factory=lambda: np.eye(3, dtype=np.float32))   # rotational component of vox2vox

    def __post_init__(self):
        self.insize = np.asarray(self.insize, np.int64).reshape(3)
        self.outsize = np.asarray(self.outsize, np.int64).reshape(3)
        self.inres = np.asarray(self.inres, np.float32).reshape(3)
        self.outres = np.asarray(self.outres, np.float32).reshape(3)
        for k in ("invox2ras", "outvox2ras", "vox2vox", "ras2ras"):
            setattr(self, k, np.asarray(getattr(self, k), np.float32).reshape(4, 4))
        self.voxrot = np.asarray(self.voxrot, np.float32).reshape(3, 3)


def round32(a):
    """a matrix computed in float64, rounded to float32 once (the rule of every matrix this package derives)"""
    return np.asarray(a, np.float64).astype(np.float32)


def voxrot_of(vox2vox):
    """the rotational component of a vox2vox matrix: U * Vt of the SVD of vox2vox[1:3, 1:3] (util.jl:265-267)"""
    u, _, vt = np.linalg.svd(np.asarray(vox2vox, np.float64)[:3, :3])
    return round32(u @ vt)


# ---- xfm_read ---------------------------------------------------------------------------------------------------------------------
_LTA_FIELDS = (("volume", "dimensions"), ("voxelsize", "resolution"), ("xras", "x_ras"), ("yras", "y_ras"), ("zras", "z_ras"),
               ("cras", "c_ras"))


def _vox2ras(size, res, xras, yras, zras, cras):
    """[xras*r1 yras*r2 zras*r3 | cras - M*size/2] (util.jl:230-248), float64 from the float32 fields, rounded once"""
    M = np.stack([np.float64(xras) * res[0], np.float64(yras) * res[1], np.float64(zras) * res[2]], axis=1)
    out = np.eye(4)
    out[:3, :3] = M
    out[:3, 3] = np.asarray(cras, np.float64) - (M @ np.asarray(size, np.float64)) / 2
    return round32(out)


def _read_lta(ltafile):
    regtype = regmat = None
    info = {"src": {}, "dst": {}}
    side = None
    with open(ltafile) as fh:
        lines = fh.read().splitlines()
    i = 0
    while i < len(lines):
        ln = lines[i].split()
        i += 1
        if not ln:
            continue
        if ln[0] == "type":                                          # transform type
            regtype = int(ln[2])
        elif ln[0] == "1" and len(ln) >= 3 and ln[1] == "4" and ln[2] == "4":   # the matrix: the next 4 lines
            regmat = np.array([[np.float32(v) for v in lines[i + k].split()] for k in range(4)], np.float32)
            i += 4
        elif ln[0] in ("src", "dst"):                                # input / output volume info
            side = ln[0]
        elif ln[0] in dict(_LTA_FIELDS) and side is not None:
            info[side][ln[0]] = np.array([np.float32(v) for v in ln[2:5]], np.float32)
    if regtype is None:
        raise ValueError("Missing transform type in " + ltafile)
    if regmat is None:
        raise ValueError("Missing transform matrix in " + ltafile)
    for key, what in _LTA_FIELDS:
        for side, name in (("src", "source"), ("dst", "destination")):
            if key not in info[side]:
                raise ValueError("Missing %s %s in %s" % (name, what, ltafile))
    return regtype, regmat, info


def xfm_read(xfmfile, inref: MRI = None, outref: MRI = None) -> Xform:
    """xfm_read(ltafile) (util.jl:163-270): a FreeSurfer .lta file; xfm_read(matfile, inref, outref) (util.jl:281-320): an FSL
    .mat file with the reference volumes of its input and output space."""
    if inref is None and outref is None:
        return _xfm_read_lta(xfmfile)
    if inref is None or outref is None:
        raise ValueError("an FSL .mat file needs both reference volumes")
    return _xfm_read_mat(xfmfile, inref, outref)


def _xfm_read_lta(ltafile):
    regtype, regmat, info = _read_lta(ltafile)
    s, d = info["src"], info["dst"]
    x = Xform(insize=s["volume"].astype(np.int64), outsize=d["volume"].astype(np.int64), inres=s["voxelsize"], outres=d["voxelsize"])
    x.invox2ras = _vox2ras(s["volume"], s["voxelsize"], s["xras"], s["yras"], s["zras"], s["cras"])
    x.outvox2ras = _vox2ras(d["volume"], d["voxelsize"], d["xras"], d["yras"], d["zras"], d["cras"])
    A, B, R = x.invox2ras.astype(np.float64), x.outvox2ras.astype(np.float64), regmat.astype(np.float64)
    if regtype == 0:                                                 # LINEAR_VOX_TO_VOX
        x.vox2vox = regmat.copy()
        x.ras2ras = round32(B @ R @ np.linalg.inv(A))
    elif regtype == 1:                                               # LINEAR_RAS_TO_RAS
        x.vox2vox = round32(np.linalg.inv(B) @ R @ A)
        x.ras2ras = regmat.copy()
    else:
        raise ValueError("Invalid transform type %d in %s" % (regtype, ltafile))
    x.voxrot = voxrot_of(x.vox2vox)
    return x


def _fsl_scale(ref: MRI):
    """FSL's scaled-voxel coordinates of a voxel: diag(volres, 1), with x = (nx - 1 - i) * rx when det(vox2ras) > 0 (util.jl:299-311
    as FSL documents it: the reference writes the translation into a `Diagonal` and throws instead)"""
    res = np.asarray(ref.volres, np.float32).astype(np.float64)
    D = np.diag([res[0], res[1], res[2], 1.0])
    if np.linalg.det(np.asarray(ref.vox2ras, np.float64)) > 0:
        D[0, 0] = -res[0]
        D[0, 3] = res[0] * (ref.volsize[0] - 1)
    return D


def _xfm_read_mat(matfile, inref: MRI, outref: MRI):
    mat = np.loadtxt(matfile, dtype=np.float64, ndmin=2)
    if mat.shape != (4, 4):
        raise ValueError("%s does not hold a 4 x 4 matrix" % matfile)
    x = Xform(insize=inref.volsize, outsize=outref.volsize, inres=inref.volres, outres=outref.volres,
              invox2ras=inref.vox2ras, outvox2ras=outref.vox2ras)
    x.vox2vox = round32(np.linalg.inv(_fsl_scale(outref)) @ mat @ _fsl_scale(inref))
    x.ras2ras = round32(x.outvox2ras.astype(np.float64) @ x.vox2vox.astype(np.float64) @ np.linalg.inv(x.invox2ras.astype(np.float64)))
    x.voxrot = voxrot_of(x.vox2vox)
    return x


# ---- inv, compose, rotate ---------------------------------------------------------------------------------------------------------
def xfm_inv(xfm: Xform) -> Xform:
    """Base.inv(xfm) (util.jl:328-343)"""
    return Xform(insize=xfm.outsize.copy(), outsize=xfm.insize.copy(), inres=xfm.outres.copy(), outres=xfm.inres.copy(),
                 invox2ras=xfm.outvox2ras.copy(), outvox2ras=xfm.invox2ras.copy(),
                 vox2vox=round32(np.linalg.inv(xfm.vox2vox.astype(np.float64))), ras2ras=round32(np.linalg.inv(xfm.ras2ras.astype(np.float64))),
                 voxrot=xfm.voxrot.T.copy())


def xfm_compose(xfm1: Xform, *xfms: Xform) -> Xform:
    """xfm_compose(xfm1, xfm2...) (util.jl:356-375): output = xfm1 * xfm2 * ... * input -- the LAST argument is applied first"""
    if not xfms:
        raise TypeError("xfm_compose takes at least two transforms")
    last = xfms[-1]
    v2v, r2r = xfm1.vox2vox.astype(np.float64), xfm1.ras2ras.astype(np.float64)
    for x in xfms:
        v2v = v2v @ x.vox2vox.astype(np.float64)
        r2r = r2r @ x.ras2ras.astype(np.float64)
    out = Xform(insize=last.insize.copy(), outsize=xfm1.outsize.copy(), inres=last.inres.copy(), outres=xfm1.outres.copy(),
                invox2ras=last.invox2ras.copy(), outvox2ras=xfm1.outvox2ras.copy(), vox2vox=round32(v2v), ras2ras=round32(r2r))
    out.voxrot = voxrot_of(out.vox2vox)
    return out


def xfm_rotate(xfm: Xform, point):
    """xfm_rotate(xfm, point) (util.jl:435-454): voxrot * point for one 3-vector, in the point's element type"""
    p = np.asarray(point)
    if p.shape != (3,):
        raise ValueError("xfm_rotate takes one point of 3 coordinates")
    dt = p.dtype if np.issubdtype(p.dtype, np.floating) else np.float32
    return (xfm.voxrot.astype(np.float64) @ p.astype(np.float64)).astype(dt)


# ---- xfm_apply --------------------------------------------------------------------------------------------------------------------
def _apply_int(m, p, out):
    """xfm_apply! into an Integer array (util.jl:423-425): the float32 loop, then round (ties to even); NaN or a value outside the
    integer type raises, as Julia's round(Int, x) does"""
    m = np.asarray(m, np.float32)
    q = np.asarray(p, np.float32).reshape(-1, 3)
    aff = np.float32(0)
    for j in range(3):
        aff = aff + m[3, j] * q[:, j]
    aff = aff + m[3, 3]
    r = np.empty_like(q)
    for i in range(3):
        lin = np.float32(0)
        for j in range(3):
            lin = lin + m[i, j] * q[:, j]
        r[:, i] = (lin + m[i, 3]) / aff
    r = np.rint(r.astype(np.float64))
    info = np.iinfo(out.dtype)
    if not np.all(np.isfinite(r)) or r.min(initial=0) < info.min or r.max(initial=0) > info.max:
        raise OverflowError("InexactError: a transformed coordinate does not round to %s" % out.dtype)
    out.reshape(-1)[:] = r.reshape(-1).astype(out.dtype)
    return out


def xfm_apply(xfm: Xform, points, out=None, device=0, stream=None):
    """xfm_apply(xfm, points) / xfm_apply!(out, xfm, points) (util.jl:385-425): vox2vox applied to N points given as [N, 3] or as a
    flat 3N vector; the result has the input's shape.

    - NumPy input: float32 points through the HIP host-buffer entry fib_xfm_apply (`device`: an index or DEVICE_ALL).  `out` may be
      the input itself (in place).  An integer `out` array is xfm_apply!'s integer form: rounded, ties to even, on the host.
    - CUDA tensor input: contiguous float32, through fibd_xfm_apply on `stream` (a torch stream, a raw hipStream_t, or None = the
      current stream); `out` may be the input tensor (in place).  The call does not wait for the kernel."""
    if hasattr(points, "is_cuda"):
        return _apply_device(xfm, points, out, stream)
    if out is not None and np.issubdtype(np.asarray(out).dtype, np.integer):
        if np.size(out) != np.size(points):
            raise ValueError("out must hold as many coordinates as points")
        return _apply_int(xfm.vox2vox, points, out)
    p = np.ascontiguousarray(points, dtype=np.float32)
    if p.size % 3:
        raise ValueError("points must be [N, 3] or a flat vector of 3N coordinates")
    if out is None:
        out = np.empty_like(p)
    elif not (isinstance(out, np.ndarray) and out.dtype == np.float32 and out.flags.c_contiguous and out.size == p.size):
        raise ValueError("out must be a contiguous float32 array of the input's size")
    _lib.check(_lib.lib().fib_xfm_apply(int(device), _host.m16(xfm.vox2vox), p.ctypes.data, out.ctypes.data, p.size // 3))
    return out


def _apply_device(xfm, points, out, stream):
    import torch
    if tensor(points, torch.float32, "points").numel() % 3:
        raise ArgError("points must be [N, 3] or a flat vector of 3N coordinates")
    with Launch(points, stream) as L:
        out = L.empty(points.shape, torch.float32) if out is None else tensor(out, torch.float32, "out", ref=points, n=points.numel())
        _lib.check(_lib.lib().fibd_xfm_apply(_host.m16(xfm.vox2vox), points.data_ptr(), out.data_ptr(), points.numel() // 3, L.sp))
    return out


# ---- Tract operations -------------------------------------------------------------------------------------------------------------
def str_xform(xfm: Xform, tr: Tract, device=0) -> Tract:
    """str_xform(xfm, tr) (trk.jl:316-347): a new Tract whose points are xfm_apply(xfm, xyz) and whose geometry is the output space
    (dim = outsize, voxel_size = outres, vox_to_ras = outvox2ras; trk_write derives voxel_order and image_orientation_patient from
    them).  Every other field is carried over.  As in the reference, vox2vox is applied to the coordinates as they are: `stream`'s
    1-based voxel coordinates, which trk_write then treats as 0-based (the `+ .5` policy of trk.py)."""
    xyz = xfm_apply(xfm, np.asarray(tr.xyz, np.float32).reshape(-1, 3), device=device)
    return replace(tr, xyz=xyz, volsize=tuple(int(v) for v in xfm.outsize), volres=tuple(float(v) for v in xfm.outres),
                   vox2ras=xfm.outvox2ras.copy())


_HEADER_FIELDS = (("dim", lambda t: tuple(int(v) for v in t.volsize)),
                  ("voxel_size", lambda t: tuple(float(np.float32(v)) for v in t.volres)),
                  ("n_scalars", lambda t: t.n_scalars),
                  ("n_properties", lambda t: t.n_properties),
                  ("vox_to_ras", lambda t: tuple(np.asarray(t.vox2ras, np.float32).reshape(-1).tolist())))


def _cat(parts, n, width):
    """per-point scalars / per-line properties of several tracts back to back ([n] for width 1, else [n, width]); None if width 0"""
    if width == 0:
        return None
    arrs = [np.asarray(p, np.float32).reshape(-1, width) for p in parts]
    out = np.concatenate(arrs) if arrs else np.zeros((n, width), np.float32)
    return out[:, 0] if width == 1 and np.ndim(parts[0]) == 1 else out


def str_merge(tr1: Tract, *trs: Tract) -> Tract:
    """str_merge(tr1, tr2...) (trk.jl:275-308): the streamlines of every tract, in argument order, under tr1's header.  The header
    fields a Tract here carries must match, else the reference's error."""
    allt = (tr1,) + trs
    for t in trs:
        for name, get in _HEADER_FIELDS:
            a, b = get(tr1), get(t)
            if a != b:
                raise ValueError("Mismatch in header field %s between input tracts (%s, %s)" % (name, a, b))
    xyz = np.concatenate([np.asarray(t.xyz, np.float32).reshape(-1, 3) for t in allt])
    npts = np.concatenate([np.asarray(t.npts, np.int32) for t in allt])
    seed = (np.concatenate([np.asarray(t.seed_index, np.int64) for t in allt])
            if all(t.seed_index is not None for t in allt) else None)
    return replace(tr1, xyz=xyz, npts=npts, seed_index=seed, vox2ras=np.array(tr1.vox2ras, np.float32),
                   scalars=_cat([t.scalars for t in allt], 0, tr1.n_scalars),
                   properties=_cat([t.properties for t in allt], 0, tr1.n_properties))
