"""Non-linear warps: a displacement field (`Warp`) applied to streamlines (`str_warp`) and volumes (`mri_warp`), inverted
(`warp_invert`), read and written as the ITK / ANTs vector image (`warp_read`, `warp_write`).  The non-linear sibling of `str_xform`
and `mri_xform`; not in the reference.  The definitions (the field in mm RAS on a grid of its own, the clamped trilinear sample, the
three-matrix warp of a point, the pulled-back volume, the fixed-point inverse) are the "Non-linear warps" section of
include/fibers_hip.h.  All compute is in csrc/warp.hip; there is no NumPy path here.

Host tier: `Tract` / `MRI` in and out, through fib_warp_points / fib_warp_volume / fib_warp_invert.  Device tier: torch tensors in and
out, through the fibd_warp_* entries on `stream`: warp_pack_device, warp_points_device, warp_volume_device, warp_invert_device."""
from dataclasses import replace

import numpy as np

from . import _host, _lib
from ._dev import ArgError, Launch, tensor
from ._host import dims as _dims, m16 as _m16
from .mri import MRI
from .nifti import load_nifti, mri_write
from .tract import Tract
from .xform import Xform, round32

_ITK_VECTOR = 1007                                               # NIFTI_INTENT_VECTOR


class Warp:
    """A displacement field: `field` is an MRI of 3 float32 frames; frame c at voxel (i, j, k) is component c of the displacement in
    mm, RAS, and field.vox2ras places the grid.  phi(x) = x + d(x) takes a RAS point of the field's space A to space B: points
    travel A -> B, volumes are pulled back B -> A."""

    def __init__(self, field: MRI):
        if not isinstance(field, MRI) or field.nframes != 3 or field.vol.dtype != np.float32:
            got = "%s of %d frames" % (field.vol.dtype, field.nframes) if isinstance(field, MRI) else type(field).__name__
            raise ValueError("a Warp takes an MRI of 3 float32 frames (the displacement in mm, RAS), not %s" % got)
        self.field = field

    @property
    def volsize(self):
        return self.field.volsize

    @property
    def vox2ras(self):
        return self.field.vox2ras

    def _planar(self):
        """the field as the C ABI takes it: [3][nz][ny][nx], which is MRI.vol's Fortran order"""
        return np.asfortranarray(self.field.vol)


# ---- files --------------------------------------------------------------------------------------------------------------------------
def _frame(frame):
    if frame not in ("ras", "lps"):
        raise ValueError("frame must be 'ras' or 'lps', not %r" % (frame,))
    return frame


def _to_ras(vol, frame):
    """[nx, ny, nz, 3] in `frame` -> RAS: under "lps" frames 0 and 1 are negated (exact)"""
    out = np.array(vol, np.float32, order="F")
    if frame == "lps":
        out[..., 0] = -out[..., 0]
        out[..., 1] = -out[..., 1]
    return out


def warp_read(path, frame=None) -> Warp:
    """A displacement field from a NIfTI file.  An ITK / ANTs vector image (dim = [5, nx, ny, nz, 1, 3], intent code 1007) holds its
    components in LPS and is read with frame="lps" (the default for that form): frames 0 and 1 are negated, exactly.  A 4-D file of
    3 frames needs an explicit frame="ras" or "lps".  Anything else is a ValueError that says what was found."""
    hdr, vol = load_nifti(path)
    dim, intent = [int(v) for v in hdr["dim"]], int(hdr["intent"][3])
    if vol.dtype != np.float32:
        raise ValueError("%s holds %s elements; a displacement field is float32" % (path, vol.dtype))
    if dim[0] == 5 and dim[4] == 1 and dim[5] == 3 and intent == _ITK_VECTOR:
        frame = _frame("lps" if frame is None else frame)
    elif dim[0] == 4 and dim[4] == 3:
        if frame is None:
            raise ValueError("%s is a 4-D file of 3 frames: say whether its components are frame='ras' or frame='lps'" % path)
        frame = _frame(frame)
    else:
        raise ValueError("%s is not a displacement field: dim = %s, intent code %d (wanted dim = [5, nx, ny, nz, 1, 3] with intent code "
                         "%d, or a 4-D file of 3 frames)" % (path, dim[:dim[0] + 1], intent, _ITK_VECTOR))
    M = hdr["vox2ras"]
    field = MRI(_to_ras(vol.reshape(dim[1], dim[2], dim[3], 3, order="F"), frame),
                volres=tuple(float(v) for v in np.sqrt((M[:3, :3].astype(np.float64) ** 2).sum(axis=0))), vox2ras=M.copy())
    return Warp(field)


def warp_write(warp: Warp, path, frame="lps"):
    """frame="lps": the ITK / ANTs vector image (dim = [5, nx, ny, nz, 1, 3], intent code 1007, components in LPS: frames 0 and 1
    negated); frame="ras": a plain 4-D file of 3 frames.  warp_read(path, frame) returns the field bit for bit.  Returns mri_write's
    error flag."""
    frame = _frame(frame)
    f = warp.field
    out = MRI(_to_ras(f.vol, frame), volres=f.volres, vox2ras=np.array(f.vox2ras, np.float32))      # (negating twice is the identity)
    return mri_write(out, path, vector=frame == "lps")


# ---- matrices -----------------------------------------------------------------------------------------------------------------------
def _f64(m):
    return np.asarray(m, np.float32).astype(np.float64).reshape(4, 4)


def _shift(v):
    T = np.eye(4)
    T[:3, 3] = v
    return T


def _ras2ras(x):
    return np.eye(4) if x is None else _f64(x.ras2ras)


def _inv(m, what):
    try:
        inv = np.linalg.inv(m)
    except np.linalg.LinAlgError:
        raise ValueError("%s is singular" % what) from None
    if not np.all(np.isfinite(inv)):
        raise ValueError("%s is singular" % what)
    return inv


def point_matrices(field_vox2ras, in_vox2ras, out_vox2ras, pre=None, post=None, origin=1):
    """(to_ras, to_field, from_ras) of str_warp, float32 [4, 4] each: made in float64 from the float32 fields and rounded once.
    to_ras = pre.ras2ras . in_vox2ras . T(-origin); to_field = inv(field_vox2ras) . to_ras (the float64 product, not the rounded
    one); from_ras = T(+origin) . inv(out_vox2ras) . post.ras2ras."""
    to_ras = _ras2ras(pre) @ _f64(in_vox2ras) @ _shift(-float(origin))
    to_field = _inv(_f64(field_vox2ras), "the field's vox2ras") @ to_ras
    from_ras = _shift(float(origin)) @ _inv(_f64(out_vox2ras), "the output's vox2ras") @ _ras2ras(post)
    return round32(to_ras), round32(to_field), round32(from_ras)


def volume_matrices(field_vox2ras, out_vox2ras, in_vox2ras, pre=None, post=None):
    """(to_ras, to_field, from_ras) of mri_warp: to_ras = pre.ras2ras . out_vox2ras; to_field = inv(field_vox2ras) . to_ras in
    float64; from_ras = inv(in_vox2ras) . post.ras2ras (in: the volume that is sampled, out: the grid that is filled)"""
    to_ras = _ras2ras(pre) @ _f64(out_vox2ras)
    to_field = _inv(_f64(field_vox2ras), "the field's vox2ras") @ to_ras
    from_ras = _inv(_f64(in_vox2ras), "the volume's vox2ras") @ _ras2ras(post)
    return round32(to_ras), round32(to_field), round32(from_ras)


def invert_matrices(field_vox2ras, out_vox2ras):
    """(out_to_ras, ras_to_field) of warp_invert: the output grid's vox2ras and float32(inv(float64(field_vox2ras)))"""
    return np.array(out_vox2ras, np.float32).reshape(4, 4), round32(_inv(_f64(field_vox2ras), "the field's vox2ras"))


# ---- host tier ----------------------------------------------------------------------------------------------------------------------
def str_warp(warp: Warp, tr: Tract, outref: MRI = None, pre: Xform = None, post: Xform = None, origin=1, device: int = 0) -> Tract:
    """The lines of `tr` moved through the field.  A point travels tract volume -> (pre.ras2ras) -> field space A -> (phi) -> B ->
    (post.ras2ras) -> the output volume; `pre` and `post` are Xforms, each the identity when None.  The points are tr.xyz and
    `origin` is the index of the first voxel's centre in those coordinates: 1 for what `stream` makes, 0 for 0-based lines; the
    result uses the same convention in the output volume.  The output geometry is `outref` (an MRI); without it, it comes from
    post's outsize / outres / outvox2ras; neither given is a ValueError.  npts, seed_index, scalars and properties are carried
    over, as str_xform does."""
    if outref is not None:
        size, res, v2r = _dims(outref.volsize), tuple(float(v) for v in outref.volres), np.array(outref.vox2ras, np.float32)
    elif post is not None:
        size, res, v2r = _dims(post.outsize), tuple(float(v) for v in post.outres), np.array(post.outvox2ras, np.float32)
    else:
        raise ValueError("str_warp needs the output geometry: outref (an MRI) or post (an Xform with outsize / outres / outvox2ras)")
    A, Q, B = point_matrices(warp.vox2ras, tr.vox2ras, v2r, pre, post, origin)
    xyz, _ = _host.packed(tr)
    out = np.empty_like(xyz)
    nx, ny, nz = _dims(warp.volsize)
    disp = warp._planar()
    _lib.check(_lib.lib().fib_warp_points(int(device), disp.ctypes.data, nx, ny, nz, _m16(A), _m16(Q), _m16(B),
                                          xyz.ctypes.data, out.ctypes.data, xyz.shape[0]))
    return replace(tr, xyz=out, volsize=size, volres=res, vox2ras=v2r)


def mri_warp(warp: Warp, mri: MRI, outref: MRI = None, interp: str = "trilinear", outside=0, pre: Xform = None, post: Xform = None,
             device: int = 0) -> MRI:
    """`mri` pulled back through the field onto the grid of `outref` (default: the field's own grid), all frames.  The SAMPLING
    POSITIONS travel with the arrows: output voxel -> (pre.ras2ras) -> field space A -> (phi) -> B -> (post.ras2ras) -> mri's
    voxels, where mri is sampled as mri_xform samples ("nearest" / "trilinear", `outside` where the nearest voxel is not in mri).
    The volume therefore moves AGAINST the arrows, from B onto a grid of A.  With ANTs: the forward field of
    antsRegistration(fixed, moving) is defined on the fixed grid; mri_warp(w, moving) pulls the moving image onto the fixed grid,
    and str_warp(w, lines_in_fixed_space, outref=moving) pushes fixed-space points into moving space -- one field serves volumes
    one way and points the other way (warp_invert makes the field for the other half).

    Element types and the widening of narrow integers are mri_xform's.  `bval` / `bvec` are NOT carried over."""
    grid = warp.field if outref is None else outref
    code, work, bits, out = _host.resample_args(mri, interp, outside, grid.volsize, "mri_warp")
    A, Q, B = volume_matrices(warp.vox2ras, grid.vox2ras, mri.vox2ras, pre, post)
    nx, ny, nz = _dims(warp.volsize)
    (nxi, nyi, nzi, nf), (nxo, nyo, nzo) = work.shape, out.shape[:3]
    disp = warp._planar()
    _lib.check(_lib.lib().fib_warp_volume(int(device), disp.ctypes.data, nx, ny, nz, _m16(A), _m16(Q), _m16(B), work.ctypes.data,
                                          nxi, nyi, nzi, nf, code, bits, out.ctypes.data, nxo, nyo, nzo))
    return _host.resampled(out, mri, grid.volres, grid.vox2ras)


def warp_invert(warp: Warp, outref: MRI, niter: int = 20, device: int = 0):
    """(Warp, err): the field of phi^-1 on the grid of `outref` (a grid in space B) by `niter` fixed-point steps x <- y - d(x) from
    x = y, and err (an MRI of one frame, mm): max_c |x_c + d_c(x) - y_c| at every voxel.  The iteration converges where the field's
    Jacobian norm is below 1; err is the check where the field folds (or leaves the grid it was estimated on)."""
    if int(niter) < 0:
        raise ValueError("niter must not be negative")
    Y, Q = invert_matrices(warp.vox2ras, outref.vox2ras)
    nx, ny, nz = _dims(warp.volsize)
    nxo, nyo, nzo = _dims(outref.volsize)
    inv = np.empty((nxo, nyo, nzo, 3), np.float32, order="F")
    err = np.empty((nxo, nyo, nzo, 1), np.float32, order="F")
    disp = warp._planar()
    _lib.check(_lib.lib().fib_warp_invert(int(device), disp.ctypes.data, nx, ny, nz, _m16(Y), _m16(Q), int(niter), inv.ctypes.data,
                                          err.ctypes.data, nxo, nyo, nzo))
    geo = dict(volres=tuple(float(v) for v in outref.volres), vox2ras=np.array(outref.vox2ras, np.float32))
    return Warp(MRI(inv, **geo)), MRI(err, **geo)


# ---- device tier --------------------------------------------------------------------------------------------------------------------
def _packed(packed, shape):
    import torch
    nx, ny, nz = _dims(shape)
    tensor(packed, torch.float32, "packed [nx*ny*nz, 4]", n=4 * nx * ny * nz)
    if packed.data_ptr() % 16:
        raise ArgError("packed must be 16-byte aligned")
    return nx, ny, nz


def warp_pack_device(disp, shape, out=None, stream=None):
    """fibd_warp_pack: disp the planar float32 field [3, nx*ny*nz] (x fastest; any 4-byte boundary) -> the packed field
    [nx*ny*nz, 4] = (dx, dy, dz, 0) that the other three take (`out` may be given: 16-byte aligned).  Does not wait."""
    import torch
    nx, ny, nz = _dims(shape)
    nvox = nx * ny * nz
    tensor(disp, torch.float32, "disp [3, nx*ny*nz]", n=3 * nvox)
    with Launch(disp, stream) as L:
        if out is None:
            out = L.empty((nvox, 4), torch.float32)
        else:
            tensor(out, torch.float32, "out [nx*ny*nz, 4]", ref=disp, n=4 * nvox)
            if out.data_ptr() % 16:
                raise ArgError("out must be 16-byte aligned")
        _lib.check(_lib.lib().fibd_warp_pack(disp.data_ptr(), nx, ny, nz, out.data_ptr(), L.sp))
    return out


def warp_points_device(packed, shape, to_ras, to_field, from_ras, xyz, out=None, stream=None):
    """fibd_warp_points: the packed field of `shape`, three float32 [4, 4] matrices (point_matrices), xyz float32 [N, 3] or a flat
    3N vector -> the warped points in the input's shape.  `out` may be xyz itself (in place) or a view at any 4-byte boundary.
    Does not wait."""
    import torch
    nx, ny, nz = _packed(packed, shape)
    if tensor(xyz, torch.float32, "xyz", ref=packed).numel() % 3:
        raise ArgError("xyz must be [N, 3] or a flat vector of 3N coordinates")
    with Launch(packed, stream) as L:
        out = L.empty(xyz.shape, torch.float32) if out is None else tensor(out, torch.float32, "out", ref=packed, n=xyz.numel())
        _lib.check(_lib.lib().fibd_warp_points(packed.data_ptr(), nx, ny, nz, _m16(to_ras), _m16(to_field), _m16(from_ras),
                                               xyz.data_ptr(), out.data_ptr(), xyz.numel() // 3, L.sp))
    return out


def warp_volume_device(packed, shape, to_ras, to_field, from_ras, vol, inshape, outshape, interp: str = "trilinear", outside=0, out=None,
                       stream=None):
    """fibd_warp_volume: vol planar [nframes, nxi*nyi*nzi] (or [nvox] for one frame), float32 or -- with "nearest" -- int32, pulled
    back through the packed field onto a grid of `outshape` (volume_matrices) -> [nframes, nxo*nyo*nzo] (or [nvox]) in the input's
    type.  `out` may be given (any 4-byte boundary; it must not overlap vol).  Does not wait."""
    import torch
    code = _host.interp_code(interp)
    nx, ny, nz = _packed(packed, shape)
    nxi, nyi, nzi = _dims(inshape)
    nxo, nyo, nzo = _dims(outshape)
    nvi, nvo = nxi * nyi * nzi, nxo * nyo * nzo
    tensor(vol, (torch.float32, torch.int32), "vol [nframes, nxi*nyi*nzi]", ref=packed, unit=nvi)
    if vol.dtype != torch.float32 and code != _lib.VOL_INTERP["nearest"]:
        raise ArgError("'trilinear' takes float32 volumes, not %s" % vol.dtype)
    nf = vol.numel() // nvi
    bits = _host.bits(outside, np.float32 if vol.dtype == torch.float32 else np.int32)
    with Launch(packed, stream) as L:
        if out is None:
            out = L.empty((nf, nvo) if vol.dim() > 1 else (nvo,), vol.dtype)
        else:
            tensor(out, vol.dtype, "out [nframes, nxo*nyo*nzo]", ref=packed, n=nf * nvo)
        _lib.check(_lib.lib().fibd_warp_volume(packed.data_ptr(), nx, ny, nz, _m16(to_ras), _m16(to_field), _m16(from_ras),
                                               vol.data_ptr(), nxi, nyi, nzi, nf, code, bits, out.data_ptr(), nxo, nyo, nzo, L.sp))
    return out


def warp_invert_device(packed, shape, out_to_ras, ras_to_field, outshape, niter: int = 20, inv=None, err=True, stream=None):
    """fibd_warp_invert: (inv [3, nxo*nyo*nzo], err [nxo*nyo*nzo]) on the grid of `outshape` (invert_matrices).  `inv` may be given;
    `err` is True (allocate it), False / None (not computed: the second result is None) or a tensor.  Does not wait."""
    import torch
    nx, ny, nz = _packed(packed, shape)
    nxo, nyo, nzo = _dims(outshape)
    nvo = nxo * nyo * nzo
    if int(niter) < 0:
        raise ArgError("niter must not be negative")
    with Launch(packed, stream) as L:
        inv = L.empty((3, nvo), torch.float32) if inv is None else tensor(inv, torch.float32, "inv [3, nxo*nyo*nzo]", ref=packed, n=3 * nvo)
        if err is True:
            err = L.empty((nvo,), torch.float32)
        elif err is False or err is None:
            err = None
        else:
            tensor(err, torch.float32, "err [nxo*nyo*nzo]", ref=packed, n=nvo)
        _lib.check(_lib.lib().fibd_warp_invert(packed.data_ptr(), nx, ny, nz, _m16(out_to_ras), _m16(ras_to_field), int(niter),
                                               inv.data_ptr(), None if err is None else err.data_ptr(), nxo, nyo, nzo, L.sp))
    return inv, err
