"""Volumes moved between spaces: `mri_xform` resamples an `MRI` through an `Xform` (nearest voxel or trilinear), `xfm_header` makes
the header-only transform between two volumes that are already in register (FreeSurfer's --regheader).  Not in the reference; the
definitions (pull-back through the output -> input matrix in float32, the inside rule, the interpolation's operation order) are the
"Volume resampling" section of include/fibers_hip.h.  All compute is in csrc/volxform.hip; there is no NumPy path here.

Host tier: `MRI` in, `MRI` out, through fib_vol_xform.  Device tier: torch tensors in and out, through fibd_vol_xform on `stream`."""
import numpy as np

from . import _host, _lib
from ._dev import ArgError, Launch, tensor
from .mri import MRI
from .xform import Xform, round32, voxrot_of


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
    return round32(inv)


def xfm_header(inref: MRI, outref: MRI) -> Xform:
    """The header-only transform from `inref`'s voxels to `outref`'s, for volumes that are already in register (FreeSurfer's
    --regheader): ras2ras = I, vox2vox = float32(inv(outref.vox2ras) @ inref.vox2ras) computed in float64; sizes, resolutions and
    vox2ras from the two headers."""
    A, B = np.asarray(inref.vox2ras, np.float32).astype(np.float64), np.asarray(outref.vox2ras, np.float32).astype(np.float64)
    x = Xform(insize=inref.volsize, outsize=outref.volsize, inres=inref.volres, outres=outref.volres,
              invox2ras=np.array(inref.vox2ras, np.float32), outvox2ras=np.array(outref.vox2ras, np.float32))
    x.vox2vox = round32(np.linalg.inv(B) @ A)
    x.voxrot = voxrot_of(x.vox2vox)
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
    _host.interp_code(interp)                               # (the first refusal, before the sizes are compared)
    if tuple(int(v) for v in xfm.insize) != tuple(mri.volsize):
        raise ValueError("the volume is %s but the transform's input space is %s" % (tuple(mri.volsize), tuple(int(v) for v in xfm.insize)))
    code, work, bits, out = _host.resample_args(mri, interp, outside, xfm.outsize, "mri_xform")
    M = vol_xform_matrix(xfm)
    (nxi, nyi, nzi, nf), (nxo, nyo, nzo) = work.shape, out.shape[:3]
    _lib.check(_lib.lib().fib_vol_xform(int(device), _host.m16(M), work.ctypes.data, nxi, nyi, nzi, nf, code, bits, out.ctypes.data, nxo, nyo, nzo))
    return _host.resampled(out, mri, xfm.outres, xfm.outvox2ras)


def vol_xform_device(out2in, vol, inshape, outshape, interp: str = "trilinear", outside=0, out=None, stream=None):
    """fibd_vol_xform on device tensors: out2in the float32 [4, 4] output -> input matrix (vol_xform_matrix), vol planar
    [nframes, nxi*nyi*nzi] (or [nvox] for one frame; x fastest), float32 or -- with "nearest" -- int32.  Returns the resampled
    volume [nframes, nxo*nyo*nzo] (or [nvox]) in the input's type; `out` may be given (a view at any 4-byte boundary is fine; it
    must not overlap vol).  The call does not wait for the kernel."""
    import torch
    code = _host.interp_code(interp)
    nxi, nyi, nzi = (int(v) for v in inshape)
    nxo, nyo, nzo = (int(v) for v in outshape)
    nvi, nvo = nxi * nyi * nzi, nxo * nyo * nzo
    tensor(vol, (torch.float32, torch.int32), "vol [nframes, nxi*nyi*nzi]", unit=nvi)
    if vol.dtype != torch.float32 and code != _lib.VOL_INTERP["nearest"]:
        raise ArgError("'trilinear' takes float32 volumes, not %s" % vol.dtype)
    nf = vol.numel() // nvi
    bits = _host.bits(outside, np.float32 if vol.dtype == torch.float32 else np.int32)
    with Launch(vol, stream) as L:
        if out is None:
            out = L.empty((nf, nvo) if vol.dim() > 1 else (nvo,), vol.dtype)
        else:
            tensor(out, vol.dtype, "out [nframes, nxo*nyo*nzo]", ref=vol, n=nf * nvo)
        _lib.check(_lib.lib().fibd_vol_xform(_host.m16(out2in), vol.data_ptr(), nxi, nyi, nzi, nf, code, bits, out.data_ptr(), nxo, nyo, nzo, L.sp))
    return out
