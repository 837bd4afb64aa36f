"""Volumes moved between spaces: `mri_xform` resamples an `MRI` through an `Xform` (nearest voxel or trilinear), `xfm_header` makes
the header-only transform between two volumes that are already in register (FreeSurfer's --regheader).  Not in the reference; the
definitions (pull-back through the output -> input matrix in float32, the inside rule, the interpolation's operation order) are the
"Volume resampling" section of include/fibers_hip.h.  All compute is in csrc/volxform.hip; there is no NumPy path here.

Host tier: `MRI` in, `MRI` out, through fib_vol_xform.  Device tier: torch tensors in and out, through fibd_vol_xform on `stream`."""
import ctypes as C

import numpy as np

from . import _lib
from ._dev import ArgError, Launch, tensor
from .mri import MRI
from .xform import Xform, _f32, _voxrot

_WIDEN = {np.dtype(np.uint8): np.uint32, np.dtype(np.uint16): np.uint32, np.dtype(np.int8): np.int32, np.dtype(np.int16): np.int32}
_WORDS = (np.dtype(np.float32), np.dtype(np.int32), np.dtype(np.uint32))


def vol_xform_matrix(xfm: Xform) -> np.ndarray:
    """The output -> input voxel matrix that fib(d)_vol_xform takes: float32(inv(float64(xfm.vox2vox))), rounded once (the rule
    xfm_inv follows).  A singular vox2vox raises ValueError."""
    m = np.asarray(xfm.vox2vox, np.float32).astype(np.float64).reshape(4, 4)
    try:
        inv = np.linalg.inv(m)
    except np.linalg.LinAlgError:
        raise ValueError("vox2vox is singular: the volume cannot be pulled back through it") from None
    if not np.all(np.isfinite(inv)):
        raise ValueError("vox2vox is singular: the volume cannot be pulled back through it")
    return _f32(inv)


def _interp(interp):
    if interp not in _lib.VOL_INTERP:
        raise ValueError("interp must be 'nearest' or 'trilinear', not %r" % (interp,))
    return _lib.VOL_INTERP[interp]


def _row_major(m):
    return (C.c_float * 16)(*[float(v) for v in np.ascontiguousarray(m, np.float32).reshape(-1)])


def _bits(outside, dtype, narrow=None):
    """`outside` cast to the volume's element type (`narrow` first, for a volume widened from it), as the int32 that carries its
    32-bit pattern"""
    with np.errstate(invalid="ignore", over="ignore"):
        v = np.array([outside])
        if narrow is not None:
            v = v.astype(narrow)
        return int(v.astype(dtype).view(np.int32)[0])


def _words(mri, interp, who):
    """mri.vol as the 32-bit words the sampler takes: float32 (either interpolation), int32 / uint32 as they are and 8- / 16-bit
    integers widened, with "nearest"; anything else is a ValueError in the name of `who`"""
    dt, nearest = mri.vol.dtype, _interp(interp) == _lib.VOL_INTERP["nearest"]
    if dt in _WIDEN and nearest:
        return np.asfortranarray(mri.vol.astype(_WIDEN[dt]))
    if dt in _WORDS and (dt == np.float32 or nearest):
        return np.asfortranarray(mri.vol)
    raise ValueError("%s takes float32 volumes (either interpolation) or 8- / 16- / 32-bit integer volumes with 'nearest', not %s with %r"
                     % (who, dt, interp))


def xfm_header(inref: MRI, outref: MRI) -> Xform:
    """The header-only transform from `inref`'s voxels to `outref`'s, for volumes that are already in register (FreeSurfer's
    --regheader): ras2ras = I, vox2vox = float32(inv(outref.vox2ras) @ inref.vox2ras) computed in float64; sizes, resolutions and
    vox2ras from the two headers."""
    A, B = np.asarray(inref.vox2ras, np.float32).astype(np.float64), np.asarray(outref.vox2ras, np.float32).astype(np.float64)
    x = Xform(insize=inref.volsize, outsize=outref.volsize, inres=inref.volres, outres=outref.volres,
              invox2ras=np.array(inref.vox2ras, np.float32), outvox2ras=np.array(outref.vox2ras, np.float32))
    x.vox2vox = _f32(np.linalg.inv(B) @ A)
    x.voxrot = _voxrot(x.vox2vox)
    return x


def mri_xform(xfm: Xform, mri: MRI, interp: str = "trilinear", outside=0, device: int = 0) -> MRI:
    """`mri` resampled onto the output grid of `xfm`: an MRI of size xfm.outsize with volres = xfm.outres, vox2ras = xfm.outvox2ras
    and all frames of the input.  Every output voxel is pulled back through inv(xfm.vox2vox) and the input is sampled there:
    "nearest" copies the voxel rint(p) (ties to even), "trilinear" interpolates between the 8 neighbours (indices clamped into the
    volume).  Samples whose nearest voxel is not in the input get `outside` (NaN allowed).

    Element types: float32 takes either interpolation; with "nearest", int32 / uint32 go as they are and uint8 / int8 / int16 /
    uint16 are widened to 32 bits, resampled and narrowed back (exact: words are only copied).  Anything else is a ValueError.

    `bval` / `bvec` are NOT carried over: reorienting gradients through the transform is out of scope, and copying them unrotated
    would be silently wrong.  mri.volsize must equal xfm.insize."""
    code = _interp(interp)
    if tuple(int(v) for v in xfm.insize) != tuple(mri.volsize):
        raise ValueError("the volume is %s but the transform's input space is %s" % (tuple(mri.volsize), tuple(int(v) for v in xfm.insize)))
    dt = mri.vol.dtype
    work = _words(mri, interp, "mri_xform")
    M = vol_xform_matrix(xfm)
    nxi, nyi, nzi = (int(v) for v in mri.volsize)
    nxo, nyo, nzo = (int(v) for v in xfm.outsize)
    nf = mri.nframes
    out = np.empty((nxo, nyo, nzo, nf), work.dtype, order="F")
    _lib.check(_lib.lib().fib_vol_xform(int(device), _row_major(M), work.ctypes.data, nxi, nyi, nzi, nf, code,
                                        _bits(outside, work.dtype, dt if dt in _WIDEN else None), out.ctypes.data, nxo, nyo, nzo))
    if out.dtype != dt:
        out = np.asfortranarray(out.astype(dt))
    res = MRI(out, volres=tuple(float(v) for v in xfm.outres), vox2ras=np.array(xfm.outvox2ras, np.float32))
    res.tr = mri.tr
    return res


def vol_xform_device(out2in, vol, inshape, outshape, interp: str = "trilinear", outside=0, out=None, stream=None):
    """fibd_vol_xform on device tensors: out2in the float32 [4, 4] output -> input matrix (vol_xform_matrix), vol planar
    [nframes, nxi*nyi*nzi] (or [nvox] for one frame; x fastest), float32 or -- with "nearest" -- int32.  Returns the resampled
    volume [nframes, nxo*nyo*nzo] (or [nvox]) in the input's type; `out` may be given (a view at any 4-byte boundary is fine; it
    must not overlap vol).  The call does not wait for the kernel."""
    import torch
    code = _interp(interp)
    nxi, nyi, nzi = (int(v) for v in inshape)
    nxo, nyo, nzo = (int(v) for v in outshape)
    nvi, nvo = nxi * nyi * nzi, nxo * nyo * nzo
    tensor(vol, (torch.float32, torch.int32), "vol [nframes, nxi*nyi*nzi]", unit=nvi)
    if vol.dtype != torch.float32 and code != _lib.VOL_INTERP["nearest"]:
        raise ArgError("'trilinear' takes float32 volumes, not %s" % vol.dtype)
    nf = vol.numel() // nvi
    bits = _bits(outside, np.float32 if vol.dtype == torch.float32 else np.int32)
    with Launch(vol, stream) as L:
        if out is None:
            out = L.empty((nf, nvo) if vol.dim() > 1 else (nvo,), vol.dtype)
        else:
            tensor(out, vol.dtype, "out [nframes, nxo*nyo*nzo]", ref=vol, n=nf * nvo)
        _lib.check(_lib.lib().fibd_vol_xform(_row_major(out2in), vol.data_ptr(), nxi, nyi, nzi, nf, code, bits, out.data_ptr(), nxo, nyo, nzo, L.sp))
    return out
