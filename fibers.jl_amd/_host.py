"""The host tier's argument contract ("The host tier in Python"), the counterpart of `_dev.py`.  The fib_* entries take
host pointers and read as many elements as the call's sizes say: every wrapper of an `MRI` / `Tract` / NumPy argument makes the array
behind each pointer here -- the element type, the memory order and the shape the ABI reads -- and a volume of another shape is refused
in the caller's words before the library is reached."""
import ctypes as C

import numpy as np

from . import _lib
from .mri import MRI
from .odf import ODF


# ---- tables -------------------------------------------------------------------------------------------------------------------------
def table_args(bval, bvec, need_bvec=True):
    """A b-table as the C ABI reads it: (bval float32 contiguous [nvol], bvec float32 Fortran-ordered [nvol, 3], or None where
    the form needs no gradient table).  A gradient table of another row count would be read past its end: ValueError."""
    bval = np.ascontiguousarray(bval, np.float32).reshape(-1)
    if not need_bvec:
        return bval, None
    bvec = np.asfortranarray(np.asarray(bvec, np.float32).reshape(-1, 3))
    if bvec.shape[0] != bval.shape[0]:
        raise ValueError("gradient table must be [%d x 3], got %s" % (bval.shape[0], bvec.shape))
    return bval, bvec


def check_tables(dwi, need_bvec=True):
    """The reference's table checks (dti.jl:166-168, 223-229) plus the shapes the C ABI relies on.  Returns
    (bval float32 contiguous [nframes], bvec float32 Fortran-ordered [nframes, 3] or None): the arrays whose pointers go
    to the library — `dwi.bvec` itself may have been assigned in any memory order after the MRI was built."""
    if dwi.bval is None or len(dwi.bval) == 0:
        raise RuntimeError("Missing b-value table from input DWI structure")        # dti.jl:167,224
    if need_bvec and (dwi.bvec is None or len(dwi.bvec) == 0):
        raise RuntimeError("Missing gradient table from input DWI structure")       # dti.jl:228
    bval = np.ascontiguousarray(dwi.bval, np.float32).reshape(-1)
    if bval.shape[0] != dwi.nframes:
        raise ValueError("b-value table length %d does not match %d frames" % (bval.shape[0], dwi.nframes))
    bvec = None
    if need_bvec:
        bvec = np.asarray(dwi.bvec, np.float32)
        if bvec.shape != (dwi.nframes, 3):
            raise ValueError("gradient table must be [%d x 3], got %s" % (dwi.nframes, bvec.shape))
        bvec = np.asfortranarray(bvec)
    return bval, bvec


# ---- volumes and masks --------------------------------------------------------------------------------------------------------------
def volume(v, shape=None, dtype=None, frame0=False, series=False, strict=None, refuse="volume shape %s does not match %s", error=ValueError):
    """An `MRI` or an array as the ABI reads a volume: Fortran-ordered (x fastest, frame slowest), of `dtype` (None: its own).
    Of a 4-D input a 3-D volume is frame 0 (frame0=True: the fits' masks, the tracer's volumes) or the input with a singleton fourth axis
    dropped (the default: dwi_denoise, the selection and connectome volumes); series=True takes the input as it is.  `shape` (None: any):
    what the result's shape must be, else error(refuse % (its shape, shape)).  strict: the TypeError sentence for an element type other
    than `dtype` (the fits' DWI); without it the elements are converted."""
    a = v.vol if isinstance(v, MRI) else np.asarray(v)
    if not series and a.ndim == 4 and (frame0 or a.shape[3] == 1):
        a = a[..., 0]
    if shape is not None and tuple(a.shape) != tuple(shape):
        raise error(refuse % (tuple(a.shape), tuple(shape)))
    if strict is not None and a.dtype != dtype:
        raise TypeError(strict)
    return np.asfortranarray(a, dtype=dtype)                 # (no copy of what is in that form already; a memory map stays the file's)


def mask(v, shape=None, rule="own", frame0=True, **refusal):
    """A mask volume (`volume`'s shape rules and refusal) and its DTYPES code.  rule "own": the array in its own element type, float64
    for a type the table lacks -- the test is the library's; "> 0" / "!= 0": that test made here, as uint8."""
    a = volume(v, shape, frame0=frame0, **refusal)
    if rule != "own":
        return np.asfortranarray(a > 0 if rule == "> 0" else a != 0, dtype=np.uint8), _lib.DTYPES["uint8"]
    if a.dtype.name not in _lib.DTYPES:
        a = np.asfortranarray(a, dtype=np.float64)
    return a, _lib.DTYPES[a.dtype.name]


def fit_inputs(dwi, m):
    """the inputs every voxel fit shares: (vol float32 [nx, ny, nz, nvol], mask, its DTYPES code with FIB_MASK_OUTPUTS_ZEROED unset)"""
    # the reference's per-voxel methods dispatch on Vector{Float32} (dti.jl:286): other eltypes are a MethodError
    vol = volume(dwi, dtype=np.float32, series=True, strict="dwi.vol must be float32 (the reference dispatches on Float32 only)")
    return (vol,) + mask(m, vol.shape[:3], refuse="mask shape %s does not match DWI volume %s")


def fit_outputs(dwi, m, nframes):
    """a voxel fit's outputs, one zero-filled MRI per frame count: `MRI.like` of the reference volume, which is the mask if it is an
    MRI, else the DWI"""
    ref = m if isinstance(m, MRI) else dwi
    return [MRI.like(ref, n) for n in nframes]


# ---- directions ---------------------------------------------------------------------------------------------------------------------
def directions(odf_dirs, faces=False, half=False):
    """An `ODF`'s vertex table as the ABI reads it: float32 [nverts, 3] Fortran-ordered (every x, then every y, then every z), with
    faces=True the pair (vertices, faces int32 [nfaces, 3] Fortran-ordered).  half=True: the table of prob_stream / ProbPlan, the first
    half of the vertices (or a [nvert, 3] array given as such) point by point, float32 [nvert, 3] C-ordered."""
    if half:
        v = odf_dirs.vertices[: odf_dirs.nvert] if isinstance(odf_dirs, ODF) else np.asarray(odf_dirs)
        return np.ascontiguousarray(v, np.float32).reshape(-1, 3)
    v = np.asfortranarray(odf_dirs.vertices, dtype=np.float32)
    return (v, np.asfortranarray(odf_dirs.faces, dtype=np.int32)) if faces else v


# ---- small ABI shapes ---------------------------------------------------------------------------------------------------------------
def m16(m):
    """a 4 x 4 matrix as the `const float[16]` of the ABI: float32, row by row (an `Xform` passes its .vox2vox)"""
    return (C.c_float * 16)(*[float(v) for v in np.ascontiguousarray(m, np.float32).reshape(-1)])


def pointers(arrs):
    """the `void *[n]` of the ABI (n = 3: `_lib.P3`) from MRIs (their .vol), arrays or None; an empty list gives one null pointer"""
    return (C.c_void_p * max(1, len(arrs)))(*[None if a is None else (a.vol if isinstance(a, MRI) else a).ctypes.data for a in arrs])


def as_list(x):
    """one MRI or array, or a sequence of them -> the list"""
    return [x] if isinstance(x, (MRI, np.ndarray)) else list(x)


def dims(shape):
    """(nx, ny, nz) as Python ints"""
    return tuple(int(v) for v in shape)


def packed(tr):
    """a Tract's points and counts as the fib_str_* entries take them: float32 [npoints, 3], int32 [nlines]"""
    return np.ascontiguousarray(np.asarray(tr.xyz, np.float32).reshape(-1, 3)), np.ascontiguousarray(tr.npts, dtype=np.int32)


# ---- a tracking result --------------------------------------------------------------------------------------------------------------
def tract_arrays(out, flags=False):
    """A filled `TractOut` -> (npts int32 [nlines], seed_index int64 [nlines], xyz float32 [npoints, 3], flags float32 [npoints] or
    None) as arrays of their own; the library's buffers are freed."""
    try:
        nl, npnt = int(out.nlines), int(out.npoints)
        npts = np.ctypeslib.as_array(out.npts, shape=(max(nl, 1),))[:nl].copy()
        sidx = np.ctypeslib.as_array(out.seed_index, shape=(max(nl, 1),))[:nl].copy()
        xyz = np.ctypeslib.as_array(out.xyz, shape=(max(npnt, 1) * 3,))[: npnt * 3].copy().reshape(-1, 3)
        fl = np.ctypeslib.as_array(out.flags, shape=(max(npnt, 1),))[:npnt].astype(np.float32) if flags else None
    finally:
        _lib.lib().fib_tract_free(C.byref(out))
    return npts, sidx, xyz, fl


# ---- a resampled volume -------------------------------------------------------------------------------------------------------------
WIDEN = {np.dtype(np.uint8): np.uint32, np.dtype(np.uint16): np.uint32, np.dtype(np.int8): np.int32, np.dtype(np.int16): np.int32}
_WORDS = (np.dtype(np.float32), np.dtype(np.int32), np.dtype(np.uint32))


def interp_code(interp):
    """ "nearest" / "trilinear" -> FIB_VOL_NEAREST / FIB_VOL_TRILINEAR"""
    if interp not in _lib.VOL_INTERP:
        raise ValueError("interp must be 'nearest' or 'trilinear', not %r" % (interp,))
    return _lib.VOL_INTERP[interp]


def bits(outside, dtype, narrow=None):
    """`outside` cast to the volume's element type (`narrow` first, for a volume widened from it), as the int32 that carries its
    32-bit pattern"""
    with np.errstate(invalid="ignore", over="ignore"):
        v = np.array([outside])
        if narrow is not None:
            v = v.astype(narrow)
        return int(v.astype(dtype).view(np.int32)[0])


def words(mri, interp, who):
    """mri.vol as the 32-bit words the sampler takes: float32 (either interpolation), int32 / uint32 as they are and 8- / 16-bit
    integers widened, with "nearest"; anything else is a ValueError in the name of `who`"""
    dt, nearest = mri.vol.dtype, interp_code(interp) == _lib.VOL_INTERP["nearest"]
    if dt in WIDEN and nearest:
        return np.asfortranarray(mri.vol.astype(WIDEN[dt]))
    if dt in _WORDS and (dt == np.float32 or nearest):
        return np.asfortranarray(mri.vol)
    raise ValueError("%s takes float32 volumes (either interpolation) or 8- / 16- / 32-bit integer volumes with 'nearest', not %s with %r"
                     % (who, dt, interp))


def resample_args(mri, interp, outside, outsize, who):
    """What a volume resampler (mri_xform, mri_warp) passes besides its matrices: (the interpolation's code, mri.vol as words, the
    bits of `outside` in the words' type, the uninitialised output words [outsize, nframes])"""
    dt = mri.vol.dtype
    work = words(mri, interp, who)
    out = np.empty(dims(outsize) + (mri.nframes,), work.dtype, order="F")
    return interp_code(interp), work, bits(outside, work.dtype, dt if dt in WIDEN else None), out


def resampled(out, mri, volres, vox2ras):
    """the output words narrowed back to mri's element type, as an MRI of the output grid that carries mri's `tr`"""
    if out.dtype != mri.vol.dtype:
        out = np.asfortranarray(out.astype(mri.vol.dtype))
    res = MRI(out, volres=tuple(float(v) for v in volres), vox2ras=np.array(vox2ras, np.float32))
    res.tr = mri.tr
    return res
