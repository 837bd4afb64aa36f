"""Tract maps: what a tractogram says about the volume it was traced in -- path-density maps (`str_density`), the scalar maps sampled
along every line (`str_sample` -> `Tract.scalars`) and per-line length / mean (`str_stats` -> `Tract.properties`).  Not in the
reference; the definitions (voxel of a point = rint, ties to even; the three density modes; float64 statistics) are the "Tract maps"
section of include/fibers_hip.h.  All compute is in csrc/tractmap.hip; there is no NumPy path here.

Host tier: `Tract` / `MRI` in, `MRI` / `Tract` out, through fib_str_*.  Device tier: torch tensors in and out, through fibd_str_* on
`stream`, taking the entries of stream_device / stream_device_run's dict as they are (no copy, no host round trip)."""
import ctypes as C
from dataclasses import replace
from typing import Sequence, Union

import numpy as np

from . import _lib
from ._dev import Launch, float3, lines as _lines, points as _points, tensor, work as _work
from ._host import packed as _packed
from .mri import MRI
from .tract import Tract


def _mode(mode, accumulate=False):
    if mode not in _lib.DENSITY_MODES:
        raise ValueError("mode must be 'points', 'lines' or 'endpoints', not %r" % (mode,))
    return _lib.DENSITY_MODES[mode] | (_lib.FIB_DENSITY_ACCUMULATE if accumulate else 0)


def _columns(a, n):
    """per-point scalars / per-line properties as float32 [n, width] (width 0 for None)"""
    if a is None:
        return np.zeros((n, 0), np.float32)
    return np.ascontiguousarray(np.asarray(a, np.float32).reshape(n, -1))


# ---- host tier --------------------------------------------------------------------------------------------------------------------
def str_density(tr: Tract, mode: str = "lines", shape=None, out: MRI = None, device: int = 0) -> MRI:
    """Path density of a tractogram: an `MRI` with a uint32 volume [nx, ny, nz] and the tract's volres / vox2ras (mri_write writes it
    as it is).  mode "points": inside points per voxel; "lines": lines that visit the voxel, each counted once however often it
    samples the voxel or comes back to it; "endpoints": first and last point of every line.  `shape` defaults to tr.volsize.
    `out`: an earlier result to accumulate into (tractograms that arrive in batches sum into one map; integer sums do not depend on
    the order).  The returned MRI carries `n_outside`: the points (line ends for "endpoints") that were not inside the volume,
    summed over the calls that accumulated into it."""
    xyz, npts = _packed(tr)
    if out is not None:
        shape = out.volsize
        d = out.vol
        if not (d.dtype == np.uint32 and d.flags.f_contiguous and d.shape[3] == 1):
            raise ValueError("out must be a result of str_density (one uint32 frame)")
    else:
        shape = tuple(int(v) for v in (tr.volsize if shape is None else shape))
        if len(shape) != 3 or min(shape) < 1:
            raise ValueError("shape must be three positive sizes (the tract's volsize is %s)" % (tuple(tr.volsize),))
        d = np.zeros(shape + (1,), np.uint32, order="F")
    if mode == "points" and xyz.shape[0] >= 2 ** 32:
        raise ValueError("counts are uint32: mode 'points' takes fewer than 2^32 points per call")
    nout = C.c_int64(0)
    _lib.check(_lib.lib().fib_str_density(int(device), xyz.ctypes.data, npts.ctypes.data, npts.size, xyz.shape[0], shape[0], shape[1], shape[2],
                                          _mode(mode, out is not None), d.ctypes.data, C.byref(nout)))
    if out is None:
        out = MRI(d, volres=tuple(tr.volres), vox2ras=np.array(tr.vox2ras, np.float32))
        out.n_outside = 0
    out.n_outside = int(getattr(out, "n_outside", 0)) + nout.value
    return out


def _planar(vols: Union[MRI, Sequence[MRI]]):
    """float32 [nx, ny, nz, nframes] Fortran-ordered = planar [nframes][nvox]: the frames of every volume, concatenated"""
    vols = [vols] if isinstance(vols, MRI) else list(vols)
    if not vols:
        raise ValueError("at least one volume to sample")
    shape = vols[0].volsize
    for v in vols:
        if v.volsize != shape:
            raise ValueError("volumes of different sizes: %s and %s" % (shape, v.volsize))
    if len(vols) == 1 and vols[0].vol.dtype == np.float32:
        return vols[0].vol, shape
    return np.asfortranarray(np.concatenate([np.asarray(v.vol, np.float32) for v in vols], axis=3)), shape


def str_sample(tr: Tract, vols: Union[MRI, Sequence[MRI]], outside: float = 0.0, device: int = 0) -> Tract:
    """The volumes' values along every line: a copy of `tr` whose `scalars` is [npoints, n] -- the columns it had, then one per frame
    of `vols` (an MRI or a list of them).  Nearest voxel (rint, ties to even: the voxel whose vector the tracer followed); points
    outside the volume get `outside` (NaN allowed)."""
    xyz, _ = _packed(tr)
    vol, shape = _planar(vols)
    n, nf = xyz.shape[0], vol.shape[3]
    s = np.empty((n, nf), np.float32)
    _lib.check(_lib.lib().fib_str_sample(int(device), xyz.ctypes.data, n, vol.ctypes.data, shape[0], shape[1], shape[2], nf,
                                         float(outside), s.ctypes.data))
    return replace(tr, scalars=np.concatenate([_columns(tr.scalars, n), s], axis=1))


def str_stats(tr: Tract, device: int = 0) -> Tract:
    """Per-line statistics: a copy of `tr` whose `properties` is [nstr, ...] -- the columns it had, then the length in mm (voxel steps
    scaled by tr.volres) and the mean of every scalar column over the line's points (float64 sums, rounded to float32 once)."""
    xyz, npts = _packed(tr)
    sc = _columns(tr.scalars, xyz.shape[0])
    ns = sc.shape[1]
    p = np.empty((npts.size, 1 + ns), np.float32)
    _lib.check(_lib.lib().fib_str_stats(int(device), xyz.ctypes.data, npts.ctypes.data, npts.size, xyz.shape[0], float3(tr.volres),
                                        sc.ctypes.data if ns else None, ns, p.ctypes.data))
    return replace(tr, properties=np.concatenate([_columns(tr.properties, npts.size), p], axis=1))


# ---- device tier ------------------------------------------------------------------------------------------------------------------
def str_work_size(nlines: int) -> int:
    """bytes of device scratch str_density_device / str_stats_device need for `nlines` lines (fibd_str_work_size)"""
    b = C.c_uint64(0)
    _lib.check(_lib.lib().fibd_str_work_size(int(nlines), C.byref(b)))
    return int(b.value)


def str_density_device(xyz, npts, shape, mode: str = "lines", out=None, n_outside=None, work=None, stream=None):
    """fibd_str_density on device tensors: xyz float32 [npoints, 3], npts int32 [nlines] (e.g. the `xyz` and `npts` entries of
    stream_device_run's dict).  Returns (density, n_outside): density uint32 [nx*ny*nz] (x fastest), n_outside int64 [1] -- both
    device tensors, the call does not wait for the kernels (but see `work`).  `out`: an earlier density to accumulate into.  An
    invalid `npts` (negative count, sum != npoints) adds nothing and sets n_outside to -1.  `stream`, and `work` = None under a raw
    handle: _dev.Launch."""
    import torch
    npnt, nl = _lines(xyz, npts)
    nx, ny, nz = (int(v) for v in shape)
    if mode == "points" and npnt >= 2 ** 32:
        raise ValueError("counts are uint32: mode 'points' takes fewer than 2^32 points per call")
    with Launch(xyz, stream) as L:
        dens = L.empty(nx * ny * nz, torch.uint32) if out is None else tensor(out, torch.uint32, "out", ref=xyz, n=nx * ny * nz)
        n_outside = L.empty(1, torch.int64) if n_outside is None else tensor(n_outside, torch.int64, "n_outside", ref=xyz, n=1)
        work, wb = _work(L, work, str_work_size, "str_work_size(nlines)", nl)
        _lib.check(_lib.lib().fibd_str_density(xyz.data_ptr(), npts.data_ptr(), nl, npnt, nx, ny, nz, _mode(mode, out is not None),
                                               dens.data_ptr(), n_outside.data_ptr(), work.data_ptr(), wb, L.sp))
    return dens, n_outside


def str_sample_device(xyz, vol, shape, outside: float = 0.0, out=None, stream=None):
    """fibd_str_sample: vol float32 planar [nframes, nx*ny*nz] (or [nx*ny*nz] for one frame) -> scalars float32 [npoints, nframes]"""
    import torch
    npnt = _points(xyz)
    nx, ny, nz = (int(v) for v in shape)
    nf = tensor(vol, torch.float32, "vol", ref=xyz, unit=nx * ny * nz).numel() // (nx * ny * nz)
    with Launch(xyz, stream) as L:
        out = L.empty((npnt, nf), torch.float32) if out is None else tensor(out, torch.float32, "out", ref=xyz, n=npnt * nf)
        _lib.check(_lib.lib().fibd_str_sample(xyz.data_ptr(), npnt, vol.data_ptr(), nx, ny, nz, nf, float(outside), out.data_ptr(), L.sp))
    return out


def str_stats_device(xyz, npts, volres, scalars=None, out=None, work=None, stream=None):
    """fibd_str_stats: properties float32 [nlines, 1 + n] -- length in mm, then the mean of each of the n columns of `scalars`
    (float32 [npoints, n] or [npoints]; None: lengths only).  Rows are left unwritten when `npts` is invalid."""
    import torch
    npnt, nl = _lines(xyz, npts)
    ns = 0
    if scalars is not None:
        if tensor(scalars, torch.float32, "scalars", ref=xyz).numel():          # (no elements: no columns)
            tensor(scalars, torch.float32, "scalars", ref=xyz, unit=npnt)
        ns = scalars.numel() // npnt if npnt else (scalars.shape[1] if scalars.dim() == 2 else 0)
    with Launch(xyz, stream) as L:
        out = L.empty((nl, 1 + ns), torch.float32) if out is None else tensor(out, torch.float32, "out", ref=xyz, n=nl * (1 + ns))
        work, wb = _work(L, work, str_work_size, "str_work_size(nlines)", nl)
        _lib.check(_lib.lib().fibd_str_stats(xyz.data_ptr(), npts.data_ptr(), nl, npnt, float3(volres), scalars.data_ptr() if ns else None, ns,
                                             out.data_ptr(), work.data_ptr(), wb, L.sp))
    return out
