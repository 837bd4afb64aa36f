"""dwi_mask: a brain mask from the DWI series itself (median-Otsu: mean of the b0 frames, iterated 3-D median, Otsu threshold, largest
component, filled holes, dilation), with its two pieces that are useful alone: `vol_median` and `mask_components`.  Not in the
reference; the definition is include/fibers_hip.h "Brain mask" (DESIGN.md §5 points there).

`dwi_mask`, `vol_median` and `mask_components` take host `MRI`s or arrays and go through the host-buffer C ABI; the `*_device`
functions are the device-resident forms on torch tensors.  `dwi_mask(dwi).mask` goes straight into every fit and into `dwi_denoise`."""
import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _host, _lib
from ._dev import ArgError, Launch, tensor, work as _work
from .mri import MRI

INFO_FIELDS = tuple(n for n, _ in _lib.MaskInfo._fields_)


@dataclass
class BrainMask:
    """Container for outputs of dwi_mask: the mask (a uint8 MRI like the DWI), the mean of the chosen frames (float32) and `info`
    (status, kstar, lo, hi, threshold, n_above, n_components, n_kept, n_filled, n_mask; include/fibers_hip.h)"""
    mask: MRI
    b0: MRI
    info: dict


def _params(radius, numpass, keep_largest, fill_holes, dilate):
    return _lib.MaskParams(int(radius), int(numpass), _flags(keep_largest, fill_holes), int(dilate))


def _flags(keep_largest, fill_holes):
    return (_lib.FIB_MASK_KEEP_LARGEST if keep_largest else 0) | (_lib.FIB_MASK_FILL_HOLES if fill_holes else 0)


def _info(st):
    return {n: getattr(st, n) for n in INFO_FIELDS}


def default_frames(bval, nframes=None):
    """the frames dwi_mask averages by default: those with bval == minimum(bval) (the rule of dti.jl:117); frame 0 without a b-table"""
    if bval is None or len(bval) == 0:
        return np.zeros(1, np.int32)
    b = np.asarray(bval, np.float32).reshape(-1)
    return np.flatnonzero(b == b.min()).astype(np.int32)


def _frame_list(frames, src):
    return default_frames(src.bval) if frames is None else np.ascontiguousarray(np.asarray(frames).reshape(-1), dtype=np.int32)


def dwi_mask_check(shape, nframes, frames, radius=2, numpass=4, keep_largest=True, fill_holes=True, dilate=0):
    """the library's refusals for a series of `nframes` volumes of `shape` (fib_dwi_mask_check; no device needed): raises FibersError
    as `dwi_mask` would"""
    nx, ny, nz = _host.dims(shape)
    fr = np.ascontiguousarray(np.asarray(frames).reshape(-1), dtype=np.int32)
    p = _params(radius, numpass, keep_largest, fill_holes, dilate)
    _lib.check(_lib.lib().fib_dwi_mask_check(nx, ny, nz, int(nframes), fr.ctypes.data if fr.size else None, int(fr.size), C.byref(p)))


def dwi_mask(dwi, frames=None, radius=2, numpass=4, keep_largest=True, fill_holes=True, dilate=0, device=0) -> BrainMask:
    """The brain mask of `dwi` (an MRI or array [nx,ny,nz,N]).  frames: the frames to average (None: those of the smallest b-value, or
    frame 0 without a b-table); radius (1..3) and numpass: the median; keep_largest, fill_holes, dilate: what follows the threshold."""
    src = dwi if isinstance(dwi, MRI) else MRI(np.asarray(dwi))
    vol = _host.volume(src, dtype=np.float32, series=True)
    nx, ny, nz, nvol = vol.shape
    fr = _frame_list(frames, src)
    p = _params(radius, numpass, keep_largest, fill_holes, dilate)
    mask, b0, info = MRI.like(src, 1, np.uint8), MRI.like(src, 1), _lib.MaskInfo()
    _lib.check(_lib.lib().fib_dwi_mask(int(device), vol.ctypes.data, nx, ny, nz, nvol, fr.ctypes.data if fr.size else None, int(fr.size),
                                       C.byref(p), mask.vol.ctypes.data, b0.vol.ctypes.data, C.byref(info)))
    return BrainMask(mask, b0, _info(info))


def vol_median(mri, radius=1, numpass=1, device=0) -> MRI:
    """The 3-D median of every frame of `mri` (an MRI or array, float32): window (2 radius + 1)^3 with edge replication, `numpass`
    passes; values are ordered by the key of their bit pattern (include/fibers_hip.h), so any pattern has a result"""
    src = mri if isinstance(mri, MRI) else MRI(np.asarray(mri))
    vol = _host.volume(src, dtype=np.float32, series=True)
    nx, ny, nz, nvol = vol.shape
    out = MRI(np.empty(vol.shape, np.float32, order="F"), bval=src.bval, bvec=src.bvec, volres=src.volres, vox2ras=src.vox2ras.copy(), tr=src.tr)
    _lib.check(_lib.lib().fib_vol_median(int(device), vol.ctypes.data, nx, ny, nz, nvol, int(radius), int(numpass), out.vol.ctypes.data))
    return out


def compact_labels(labels):
    """canonical labels (1 + the smallest linear index of the component) renumbered 1..n in ascending order; 0 stays 0"""
    u = np.unique(labels)
    u = u[u != 0]
    return np.searchsorted(u, labels).astype(np.int32) + (labels != 0).astype(np.int32) if u.size else labels


def mask_components(mask, keep_largest=False, fill_holes=False, compact=True, device=0, with_info=False):
    """int32 labels (an MRI like `mask`) of the 6-connected components of `mask` (an MRI or array, nonzero = inside) after the
    selection of the largest and the filling of holes, if asked for.  A label is 1 + the smallest linear index (x fastest) of its
    component; compact=True renumbers them 1..n in that order.  with_info: (labels, info dict)."""
    m, _ = _host.mask(mask, None, "!= 0", frame0=False)
    if m.ndim != 3:
        raise ValueError("mask_components takes one volume, not an array of shape %s" % (m.shape,))
    nx, ny, nz = m.shape
    ref = mask if isinstance(mask, MRI) else MRI(m)
    labels, info = MRI.like(ref, 1, np.int32), _lib.MaskInfo()
    _lib.check(_lib.lib().fib_mask_components(int(device), m.ctypes.data, nx, ny, nz, _flags(keep_largest, fill_holes), labels.vol.ctypes.data,
                                              None, C.byref(info)))
    if compact:
        labels.vol = np.asfortranarray(compact_labels(labels.vol))
    return (labels, _info(info)) if with_info else labels


# ---- device tier ------------------------------------------------------------------------------------------------------------------
def _size(fn, *args):
    b = C.c_uint64()
    _lib.check(getattr(_lib.lib(), fn)(*[int(a) for a in args], C.byref(b)))
    return int(b.value)


def vol_median_work_size(nx, ny, nz, numpass=1):
    """bytes of device workspace vol_median_device needs (fibd_vol_median_work_size)"""
    return _size("fibd_vol_median_work_size", nx, ny, nz, numpass)


def mask_components_work_size(nx, ny, nz):
    """bytes of device workspace mask_components_device needs (fibd_mask_components_work_size)"""
    return _size("fibd_mask_components_work_size", nx, ny, nz)


def dwi_mask_work_size(nx, ny, nz):
    """bytes of device workspace dwi_mask_device needs (fibd_dwi_mask_work_size)"""
    return _size("fibd_dwi_mask_work_size", nx, ny, nz)


def _shape(shape):
    nx, ny, nz = _host.dims(shape)
    if nx <= 0 or ny <= 0 or nz <= 0:
        raise ArgError("shape %s: nx, ny and nz must be positive" % (tuple(shape),))
    return nx, ny, nz


def info_dict(info):
    """the `info` tensor of a device-tier call (int64 [8], the 64 bytes of fib_mask_info) as a dict; waits for the tensor"""
    raw = info.cpu().numpy().tobytes()
    return _info(_lib.MaskInfo.from_buffer_copy(raw))


def vol_median_device(vol, shape, radius=1, numpass=1, out=None, work=None, stream=None):
    """Device tier: vol = a contiguous float32 CUDA tensor of nx*ny*nz elements (x fastest); returns the filtered volume (`out`: such a
    tensor to write into, not `vol` itself).  `work`: at least vol_median_work_size(nx, ny, nz, numpass) bytes; `stream`: _dev.Launch."""
    import torch
    nx, ny, nz = _shape(shape)
    n = nx * ny * nz
    tensor(vol, torch.float32, "vol", n=n)
    if out is not None:
        tensor(out, torch.float32, "out", ref=vol, n=n)
        if out.data_ptr() == vol.data_ptr():
            raise ArgError("out must not be vol itself")
    with Launch(vol, stream) as L:
        if out is None:
            out = L.empty(tuple(vol.shape), torch.float32)
        w, wb = _work(L, work, vol_median_work_size, "vol_median_work_size", nx, ny, nz, numpass)
        _lib.check(_lib.lib().fibd_vol_median(vol.data_ptr(), nx, ny, nz, int(radius), int(numpass), out.data_ptr(), w.data_ptr(), wb, L.sp))
    return out


def mask_components_device(mask, shape, keep_largest=False, fill_holes=False, out=None, work=None, stream=None):
    """Device tier: mask = uint8 (or bool) [nx*ny*nz], nonzero = inside.  Returns dict(labels int32 [n] (canonical, of the result's
    components), mask uint8 [n] (the result), info int64 [8]: `info_dict`); `out`: such a dict to write into."""
    import torch
    nx, ny, nz = _shape(shape)
    n = nx * ny * nz
    mask = tensor(mask, torch.uint8, "mask", n=n, bool_ok=True)
    with Launch(mask, stream) as L:
        if out is None:
            out = dict(labels=L.empty(n, torch.int32), mask=L.empty(n, torch.uint8), info=L.empty(8, torch.int64))
        else:
            for k, dt, cnt in (("labels", torch.int32, n), ("mask", torch.uint8, n), ("info", torch.int64, 8)):
                tensor(out[k], dt, "out[%r]" % k, ref=mask, n=cnt)
        w, wb = _work(L, work, mask_components_work_size, "mask_components_work_size", nx, ny, nz)
        _lib.check(_lib.lib().fibd_mask_components(mask.data_ptr(), nx, ny, nz, _flags(keep_largest, fill_holes), out["labels"].data_ptr(),
                                                   out["mask"].data_ptr(), out["info"].data_ptr(), w.data_ptr(), wb, L.sp))
    return out


def dwi_mask_device(dwi, shape, frames=(0,), radius=2, numpass=4, keep_largest=True, fill_holes=True, dilate=0, out=None, work=None,
                    stream=None):
    """Device tier: dwi = a contiguous float32 CUDA tensor [N, nx*ny*nz] (x fastest); frames: the indices to average, in the order of
    the sum.  Returns dict(mask uint8 [n], b0 float32 [n], info int64 [8]: `info_dict`); `out`: such a dict to write into.  `work`: at
    least dwi_mask_work_size(nx, ny, nz) bytes."""
    import torch
    nx, ny, nz = _shape(shape)
    n = nx * ny * nz
    tensor(dwi, torch.float32, "dwi [N, nvox]", shape=(None, n))
    nvol = int(dwi.shape[0])
    fr = np.ascontiguousarray(np.asarray(frames).reshape(-1), dtype=np.int32)
    p = _params(radius, numpass, keep_largest, fill_holes, dilate)
    _lib.check(_lib.lib().fib_dwi_mask_check(nx, ny, nz, nvol, fr.ctypes.data if fr.size else None, int(fr.size), C.byref(p)))
    with Launch(dwi, stream) as L:
        if out is None:
            out = dict(mask=L.empty(n, torch.uint8), b0=L.empty(n, torch.float32), info=L.empty(8, torch.int64))
        else:
            for k, dt, cnt in (("mask", torch.uint8, n), ("b0", torch.float32, n), ("info", torch.int64, 8)):
                tensor(out[k], dt, "out[%r]" % k, ref=dwi, n=cnt)
        w, wb = _work(L, work, dwi_mask_work_size, "dwi_mask_work_size", nx, ny, nz)
        _lib.check(_lib.lib().fibd_dwi_mask(dwi.data_ptr(), n, nvol, fr.ctypes.data, int(fr.size), nx, ny, nz, C.byref(p), out["mask"].data_ptr(),
                                            out["b0"].data_ptr(), out["info"].data_ptr(), w.data_ptr(), wb, L.sp))
    return out
