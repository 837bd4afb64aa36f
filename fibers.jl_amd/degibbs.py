"""dwi_degibbs: removal of Gibbs ringing from a DWI series by local subvoxel shifts (Kellner et al. 2016; not in the reference; the
definition is include/fibers_hip.h "Gibbs-ringing removal" and DESIGN.md §5).

`dwi_degibbs(dwi)` takes a host `MRI` and goes through the host-buffer C ABI (fib_dwi_degibbs, chunks of whole slices);
`dwi_degibbs_device` is the device-resident form on torch tensors (fibd_dwi_degibbs).  The result's `dwi` keeps the gradient table and
the geometry and goes straight into `dwi_mask`, `dti_fit`, `dki_fit`, `csd_rec`."""
import ctypes as C
from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import _host, _lib
from ._dev import ArgError, Launch, tensor, work as _work
from .mri import MRI

MAX_SIZE = 256                          # FIB_DEGIBBS_MAX_SIZE: the largest in-plane size


@dataclass
class Degibbsed:
    """Container for outputs of dwi_degibbs: the unrung series (with the input's bval / bvec and geometry) and, when asked for, the
    chosen candidate j* of the search along the first and the second in-plane axis per voxel and frame (int8; 0 = no shift)"""
    dwi: MRI
    shift_u: Optional[MRI] = None
    shift_v: Optional[MRI] = None


def _params(slice_axis, nshifts, min_w, max_w):
    return _lib.DegibbsParams(int(slice_axis), int(nshifts), int(min_w), int(max_w))


def dwi_degibbs_check(shape, nframes, slice_axis=2, nshifts=20, min_w=1, max_w=3):
    """the library's refusals for a series of `nframes` volumes of `shape` (fib_dwi_degibbs_check; no device needed): raises
    FibersError as `dwi_degibbs` would"""
    nx, ny, nz = _host.dims(shape)
    p = _params(slice_axis, nshifts, min_w, max_w)
    _lib.check(_lib.lib().fib_dwi_degibbs_check(nx, ny, nz, int(nframes), C.byref(p)))


def degibbs_table(n, nshifts=20):
    """the circulant table the kernels read for rows of length n: float64 [2 nshifts, n], [j - 1, t] = D(t + s_j) (fib_degibbs_table)"""
    out = np.zeros((2 * int(nshifts), int(n)), np.float64)
    _lib.check(_lib.lib().fib_degibbs_table(int(n), int(nshifts), out.ctypes.data))
    return out


def dwi_degibbs(dwi, slice_axis=2, nshifts=20, min_w=1, max_w=3, shifts=False, device=0) -> Degibbsed:
    """Remove the Gibbs ringing of `dwi` (an MRI or array [nx,ny,nz,N]) slice by slice, the slices lying across `slice_axis`:
    `nshifts` subvoxel shifts to either side (1..32), total variation over the windows min_w..max_w (1 <= min_w <= max_w <= 6).
    shifts=True also returns the chosen candidates.  Returns a `Degibbsed` structure."""
    src = dwi if isinstance(dwi, MRI) else MRI(np.asarray(dwi))
    vol = _host.volume(src, dtype=np.float32, series=True)
    nx, ny, nz, nvol = vol.shape
    p = _params(slice_axis, nshifts, min_w, max_w)
    out = MRI(np.zeros(vol.shape, np.float32, order="F"), bval=src.bval, bvec=src.bvec, volres=src.volres, vox2ras=src.vox2ras.copy(), tr=src.tr)
    su, sv = (MRI.like(src, nvol, np.int8), MRI.like(src, nvol, np.int8)) if shifts else (None, None)
    _lib.check(_lib.lib().fib_dwi_degibbs(int(device), vol.ctypes.data, nx, ny, nz, nvol, C.byref(p), out.vol.ctypes.data,
                                          su.vol.ctypes.data if shifts else None, sv.vol.ctypes.data if shifts else None))
    return Degibbsed(out, su, sv)


def dwi_degibbs_work_size(nx, ny, nz, nframes, slice_axis=2, nshifts=20, min_w=1, max_w=3):
    """bytes of device workspace dwi_degibbs_device needs (fibd_dwi_degibbs_work_size)"""
    b = C.c_uint64()
    p = _params(slice_axis, nshifts, min_w, max_w)
    _lib.check(_lib.lib().fibd_dwi_degibbs_work_size(int(nx), int(ny), int(nz), int(nframes), C.byref(p), C.byref(b)))
    return int(b.value)


def dwi_degibbs_device(dwi, shape, slice_axis=2, nshifts=20, min_w=1, max_w=3, shifts=False, out=None, work=None, stream=None):
    """Device tier: dwi = a contiguous float32 CUDA tensor [N, nx*ny*nz] (x fastest) of the volume `shape`.  Returns dict(dwi [N, nvox]
    float32, and with shifts=True shift_u, shift_v int8 [N, nvox]) (`out`: such a dict to write into; its shift tensors, if any, are
    filled whatever `shifts` says).  out["dwi"] must not be `dwi`: there is no in-place form.  `work`: a caller's workspace of at least
    dwi_degibbs_work_size(nx, ny, nz, N, ...) bytes (None: scratch of the launch); `stream`: _dev.Launch."""
    import torch
    nx, ny, nz = (int(n) for n in shape)
    if nx <= 0 or ny <= 0 or nz <= 0:
        raise ArgError("shape %s: nx, ny and nz must be positive" % (tuple(shape),))
    nvox = nx * ny * nz
    tensor(dwi, torch.float32, "dwi", shape=(None, nvox))
    nvol = int(dwi.shape[0])
    if nvol < 1:
        raise ArgError("dwi must hold at least one frame")
    p = _params(slice_axis, nshifts, min_w, max_w)
    with Launch(dwi, stream) as L:
        if out is None:
            out = dict(dwi=L.empty((nvol, nvox), torch.float32))
            if shifts:
                out["shift_u"], out["shift_v"] = L.empty((nvol, nvox), torch.int8), L.empty((nvol, nvox), torch.int8)
        else:
            tensor(out["dwi"], torch.float32, "out['dwi']", ref=dwi, n=nvol * nvox)
            for k in ("shift_u", "shift_v"):
                if out.get(k) is not None:
                    tensor(out[k], torch.int8, "out[%r]" % k, ref=dwi, n=nvol * nvox)
            lo, hi = out["dwi"].data_ptr(), out["dwi"].data_ptr() + 4 * nvol * nvox
            if lo < dwi.data_ptr() + 4 * nvol * nvox and dwi.data_ptr() < hi:
                raise ArgError("out['dwi'] must not overlap dwi (there is no in-place form)")
        ptr = lambda k: out[k].data_ptr() if out.get(k) is not None else None     # noqa: E731
        w, wb = _work(L, work, dwi_degibbs_work_size, "dwi_degibbs_work_size", nx, ny, nz, nvol, slice_axis, nshifts, min_w, max_w)
        _lib.check(_lib.lib().fibd_dwi_degibbs(dwi.data_ptr(), nx, ny, nz, nvol, C.byref(p), ptr("dwi"), ptr("shift_u"), ptr("shift_v"),
                                               w.data_ptr(), wb, L.sp))
    return out
