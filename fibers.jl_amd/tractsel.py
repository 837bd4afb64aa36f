"""Tract selection and connectomes: the lines of a tractogram chosen by regions of interest (`str_select`) and the region-by-region
matrix of line counts and mean lengths from a label volume (`str_connectome`).  Not in the reference; the definitions (ROI bit
volume, per-line predicates and the keep rule, stable compaction, node of a line end, C and W) are the "Tract selection and
connectomes" section of include/fibers_hip.h.  All compute is in csrc/tractsel.hip; there is no NumPy path here (compacting HOST
arrays by the flags the GPU returned is a host copy and is done here, as the header says).

Host tier: `Tract` / `MRI` in, `Tract` / `Connectome` out, through fib_str_*.  Device tier: torch tensors in and out, through
fibd_str_* on `stream`, taking the entries of stream_device / stream_device_run's dict as they are."""
import ctypes as C
from dataclasses import dataclass, replace
from typing import Optional

import numpy as np

from . import _host, _lib
from .tract import Tract
from ._dev import ArgError, Launch, float3, lines as _lines, points as _points, tensor, work as _work
from ._host import packed as _packed


_SIZE = " has size %s, the tract's volume %s"


def _take(a, idx):
    return None if a is None else np.ascontiguousarray(np.asarray(a)[idx])


# ---- host tier --------------------------------------------------------------------------------------------------------------------
def str_select(tr: Tract, include=(), exclude=(), end_in=(), both_ends_in=(), min_npts: int = 0, max_npts: int = 0, device: int = 0) -> Tract:
    """The lines of `tr` that pass through EVERY region of `include` and through none of `exclude`, have at least one end in every
    region of `end_in` and both ends in every region of `both_ends_in`, and min_npts <= npts (<= max_npts unless that is 0): a
    compacted copy in the input's order that carries the kept lines' `scalars`, `properties` and `seed_index`.  A region is an `MRI`
    or an array of the tract's volume size, non-zero inside; 32 regions in all.  The result has `hits` (uint32 [nkept, 3] = the
    OR of the regions' bits over the line, at its first and at its last point; bit r = the r-th region in the order include, exclude,
    end_in, both_ends_in) and `index` (int64 [nkept]: the line's index in `tr`) as attributes."""
    groups = [_host.as_list(g) for g in (include, exclude, end_in, both_ends_in)]
    shape = _host.dims(tr.volsize)
    rois = [_host.mask(r, shape, "!= 0", frame0=False, refuse="a region" + _SIZE)[0] for g in groups for r in g]
    if len(rois) > 32:
        raise ValueError("%d regions: one call takes 32" % len(rois))
    masks, bit = [], 0
    for g in groups:
        masks.append(sum(1 << (bit + k) for k in range(len(g))))
        bit += len(g)
    xyz, npts = _packed(tr)
    keep = np.empty(npts.size, np.uint8)
    hits = np.empty((npts.size, 3), np.uint32)
    counts = (C.c_int64 * 2)()
    ptrs = _host.pointers(rois)
    _lib.check(_lib.lib().fib_str_select(int(device), xyz.ctypes.data, npts.ctypes.data, npts.size, xyz.shape[0], shape[0], shape[1], shape[2],
                                         ptrs, len(rois), masks[0], masks[1], masks[2], masks[3], int(min_npts), int(max_npts),
                                         keep.ctypes.data, hits.ctypes.data, counts))
    out = str_take(tr, keep)
    assert out.nstr == counts[0] and out.xyz.shape[0] == counts[1]
    out.hits = hits[keep != 0]
    return out


def str_take(tr: Tract, keep) -> Tract:
    """the lines of `tr` whose flag is non-zero, in order (a host copy): xyz, npts, seed_index, scalars and properties of the kept lines;
    `index` holds their indices in `tr`"""
    keep = np.asarray(keep).reshape(-1) != 0
    if keep.size != tr.nstr:
        raise ValueError("%d flags for %d lines" % (keep.size, tr.nstr))
    rows = np.repeat(keep, np.asarray(tr.npts, np.int64))
    out = replace(tr, xyz=np.ascontiguousarray(np.asarray(tr.xyz, np.float32).reshape(-1, 3)[rows]), npts=np.ascontiguousarray(tr.npts, dtype=np.int32)[keep],
                  seed_index=_take(tr.seed_index, keep), scalars=_take(tr.scalars, rows), properties=_take(tr.properties, keep))
    out.index = np.flatnonzero(keep).astype(np.int64)
    return out


@dataclass
class Connectome:
    counts: np.ndarray                    # uint32 [L+1, L+1]: lines between node i and node j; row / column 0 = unassigned ends
    mean_length: Optional[np.ndarray]     # float64 [L+1, L+1]: W / C in mm where C > 0, else 0 (None without lengths)
    ids: np.ndarray                       # int64 [L]: the label value of node 1..L
    assign: np.ndarray                    # int32 [nstr, 2]: node of every line's first and last point
    total_length: Optional[np.ndarray] = None   # float64 [L+1, L+1]: W itself
    n_lines: int = 0                      # lines counted (npts >= 1)


def _remap(ids):
    """remap[label] = node (1-based position in ids), 0 elsewhere"""
    ids = np.asarray(ids, np.int64).reshape(-1)
    if ids.size < 1 or (ids < 0).any() or np.unique(ids).size != ids.size:
        raise ValueError("ids must be distinct non-negative label values, at least one")
    if int(ids.max()) >= 1 << 26:
        raise ValueError("label values of 2^26 and more are not supported")
    remap = np.zeros(int(ids.max()) + 1, np.int32)
    remap[ids] = np.arange(1, ids.size + 1, dtype=np.int32)
    return ids, remap


def str_connectome(tr: Tract, labels, ids=None, lengths: bool = True, device: int = 0) -> Connectome:
    """The connectome of a tractogram: `labels` (an `MRI` or an integer array of the tract's volume size, e.g. aparc+aseg) gives every
    line end a node; counts[i, j] is the number of lines between nodes i and j, mean_length[i, j] their mean length in mm.  `ids`:
    the label values that are nodes, in node order (node k = ids[k - 1]); default: the sorted unique positive values of `labels`.
    Ends outside the volume or in a voxel whose label is no node go to row / column 0."""
    shape = _host.dims(tr.volsize)
    lab = _host.volume(labels, shape, refuse="labels" + _SIZE)
    if not np.issubdtype(lab.dtype, np.integer) and not np.array_equal(lab, np.rint(lab)):
        raise ValueError("labels must hold integers")
    lab = np.asfortranarray(lab, dtype=np.int32)
    if ids is None:
        ids = np.unique(lab[lab > 0])
    ids, remap = _remap(ids)
    L = int(ids.size)
    xyz, npts = _packed(tr)
    cmat = np.zeros((L + 1, L + 1), np.uint32)
    wmat = np.zeros((L + 1, L + 1), np.float64) if lengths else None
    assign = np.zeros((npts.size, 2), np.int32)
    n = C.c_int64(0)
    _lib.check(_lib.lib().fib_str_connectome(int(device), xyz.ctypes.data, npts.ctypes.data, npts.size, xyz.shape[0], shape[0], shape[1], shape[2],
                                             float3(tr.volres), lab.ctypes.data, remap.ctypes.data, remap.size, L, 0, cmat.ctypes.data,
                                             wmat.ctypes.data if lengths else None, assign.ctypes.data, C.byref(n)))
    mean = None
    if lengths:
        mean = np.zeros_like(wmat)
        np.divide(wmat, cmat, out=mean, where=cmat > 0)
    return Connectome(counts=cmat, mean_length=mean, ids=ids, assign=assign, total_length=wmat, n_lines=int(n.value))


# ---- device tier ------------------------------------------------------------------------------------------------------------------
def str_select_work_size(nlines: int) -> int:
    """bytes of device scratch str_select_device / str_gather_device / str_connectome_device need for `nlines` lines"""
    b = C.c_uint64(0)
    _lib.check(_lib.lib().fibd_str_select_work_size(int(nlines), C.byref(b)))
    return int(b.value)


_WORK = "str_select_work_size(nlines)"


def str_roi_pack_device(rois, out=None, stream=None):
    """fibd_str_roi_pack: rois uint8 (or bool) [nroi, nvox] -> roibits uint32 [nvox], bit r = (rois[r] != 0)"""
    import torch
    rois = tensor(rois, torch.uint8, "rois", shape=(None, None), bool_ok=True)
    nroi, nvox = int(rois.shape[0]), int(rois.shape[1])
    if nroi > 32:
        raise ArgError("rois must be [nroi <= 32, nvox], not %d regions" % nroi)
    with Launch(rois, stream) as L:
        out = L.empty(nvox, torch.uint32) if out is None else tensor(out, torch.uint32, "out", ref=rois, n=nvox)
        _lib.check(_lib.lib().fibd_str_roi_pack(rois.data_ptr(), nroi, nvox, out.data_ptr(), L.sp))
    return out


def str_select_device(xyz, npts, shape, roibits=None, visit_all: int = 0, visit_none: int = 0, end_any: int = 0, end_both: int = 0,
                      min_npts: int = 0, max_npts: int = 0, hits: bool = True, work=None, stream=None):
    """fibd_str_select on device tensors: xyz float32 [npoints, 3], npts int32 [nlines], roibits uint32 [nx*ny*nz].  Returns (keep uint8
    [nlines], hits uint32 [nlines, 3] or None, counts int64 [2] = kept lines, kept points) -- device tensors, the call does not wait
    (`stream`, and `work` = None under a raw handle: _dev.Launch).  An invalid `npts` gives keep = 0, counts = (-1, -1) and leaves
    hits unwritten."""
    import torch
    npnt, nl = _lines(xyz, npts)
    nx, ny, nz = (int(v) for v in shape)
    if roibits is not None:
        tensor(roibits, torch.uint32, "roibits", ref=xyz, n=nx * ny * nz)
    with Launch(xyz, stream) as L:
        keep = L.empty(nl, torch.uint8)
        h = L.empty((nl, 3), torch.uint32) if hits else None
        counts = L.empty(2, torch.int64)
        work, wb = _work(L, work, str_select_work_size, _WORK, nl)
        _lib.check(_lib.lib().fibd_str_select(xyz.data_ptr(), npts.data_ptr(), nl, npnt, nx, ny, nz, roibits.data_ptr() if roibits is not None else None,
                                              int(visit_all), int(visit_none), int(end_any), int(end_both), int(min_npts), int(max_npts),
                                              keep.data_ptr(), h.data_ptr() if hits else None, counts.data_ptr(), work.data_ptr(), wb, L.sp))
    return keep, h, counts


def str_gather_device(xyz, npts, keep, scalars=None, cap_lines=None, cap_points=None, out=None, index: bool = True, work=None, stream=None):
    """fibd_str_gather: the lines with keep != 0 (uint8 or bool [nlines]; ANY flags), in order.  Returns a dict: `xyz` [cap_points, 3],
    `npts` [cap_lines], `index` int64 [cap_lines] (None with index=False), `scalars` [cap_points, n] (None without scalars) and
    `counts` int64 [3] = (kept lines, kept points, status) on the device.  The capacities default to the input's sizes, which always
    suffice; the first counts[0] lines and counts[1] points of the outputs are the result.  If a capacity is exceeded (status -1) or
    `npts` is invalid (counts -1, -1) nothing is written.  `out`: a dict of an earlier call whose tensors are written again."""
    import torch
    npnt, nl = _lines(xyz, npts)
    keep = tensor(keep, torch.uint8, "keep", ref=xyz, n=nl, bool_ok=True)
    ns = 0
    if scalars is not None:
        ns = tensor(scalars, torch.float32, "scalars [npoints, n >= 1]", ref=xyz, unit=npnt).numel() // npnt
    with Launch(xyz, stream) as L:
        if out is None:
            cl = nl if cap_lines is None else int(cap_lines)
            cp = npnt if cap_points is None else int(cap_points)
            out = dict(xyz=L.empty((cp, 3), torch.float32), npts=L.empty(cl, torch.int32), index=L.empty(cl, torch.int64) if index else None,
                       scalars=L.empty((cp, ns), torch.float32) if ns else None, counts=L.empty(3, torch.int64))
        cl = tensor(out["npts"], torch.int32, "out npts", ref=xyz).numel()
        cp = _points(out["xyz"], "out xyz", xyz)
        tensor(out["counts"], torch.int64, "out counts", ref=xyz, n=3)
        if out.get("index") is not None:
            tensor(out["index"], torch.int64, "out index", ref=xyz, n=cl)
        if ns:
            tensor(out.get("scalars"), torch.float32, "out scalars", ref=xyz, n=cp * ns)
        work, wb = _work(L, work, str_select_work_size, _WORK, nl)
        _lib.check(_lib.lib().fibd_str_gather(xyz.data_ptr(), npts.data_ptr(), nl, npnt, keep.data_ptr(), scalars.data_ptr() if ns else None, ns, cl, cp,
                                              out["xyz"].data_ptr(), out["npts"].data_ptr(),
                                              out["index"].data_ptr() if out.get("index") is not None else None,
                                              out["scalars"].data_ptr() if ns else None, out["counts"].data_ptr(), work.data_ptr(), wb, L.sp))
    return out


def str_connectome_device(xyz, npts, shape, labels, nnodes: int, remap=None, volres=None, out=None, assign: bool = True, work=None, stream=None):
    """fibd_str_connectome: labels int32 [nx*ny*nz], remap int32 [nremap] or None (identity), nnodes = L.  Returns a dict: `counts` uint32
    [L+1, L+1], `lengths` float64 [L+1, L+1] = W (None unless `volres` is given: no length is computed without it), `assign` int32
    [nlines, 2] (None with assign=False) and `n_lines` int64 [1] (-1 for an invalid `npts`, and then nothing was added).  `out`: the
    dict of an earlier call to accumulate into (tractograms that arrive in batches; the counts do not depend on the order)."""
    import torch
    npnt, nl = _lines(xyz, npts)
    nx, ny, nz = (int(v) for v in shape)
    nn = int(nnodes)
    tensor(labels, torch.int32, "labels", ref=xyz, n=nx * ny * nz)
    if remap is not None:
        tensor(remap, torch.int32, "remap", ref=xyz)
    res = None if volres is None else float3(volres)
    with Launch(xyz, stream) as L:
        flags = 0
        if out is None:
            out = dict(counts=L.empty((nn + 1, nn + 1), torch.uint32), lengths=L.empty((nn + 1, nn + 1), torch.float64) if volres is not None else None)
        else:
            flags = _lib.FIB_CONNECTOME_ACCUMULATE
            out = dict(counts=tensor(out["counts"], torch.uint32, "out counts", ref=xyz, n=(nn + 1) ** 2), lengths=out.get("lengths"))
            if (out["lengths"] is None) != (volres is None):
                raise ValueError("lengths are accumulated iff volres is given and the earlier call had them")
            if volres is not None:
                tensor(out["lengths"], torch.float64, "out lengths", ref=xyz, n=(nn + 1) ** 2)
        out["assign"] = L.empty((nl, 2), torch.int32) if assign else None
        out["n_lines"] = L.empty(1, torch.int64)
        work, wb = _work(L, work, str_select_work_size, _WORK, nl)
        _lib.check(_lib.lib().fibd_str_connectome(xyz.data_ptr(), npts.data_ptr(), nl, npnt, nx, ny, nz, res, labels.data_ptr(),
                                                  remap.data_ptr() if remap is not None else None, remap.numel() if remap is not None else 0, nn, flags,
                                                  out["counts"].data_ptr(), out["lengths"].data_ptr() if volres is not None else None,
                                                  out["assign"].data_ptr() if assign else None, out["n_lines"].data_ptr(), work.data_ptr(), wb, L.sp))
    return out
