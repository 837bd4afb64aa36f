"""Bundle tools: every line of a tractogram brought to the same number of points (`str_resample`), its MDF distance to a set of model
bundles with the nearest model and the orientation (`str_bundles`), the mean line of every bundle (`str_centroids`) and the profile of
a volume along every bundle (`str_profile`).  Not in the reference; the definitions (arc-length resampling in mm, the sequential
float64 MDF sums, first minimum, the oriented sums) are the "Bundle tools" section of include/fibers_hip.h.  All compute is in
csrc/bundle.hip; there is no NumPy path here (the per-node mean of `str_profile` is arithmetic on the kernels' results, not a kernel).

Host tier: `Tract` / `MRI` in, `Tract` / `Bundles` / arrays out, through fib_str_*.  Device tier: torch tensors in and out, through
fibd_str_* on `stream`, taking the entries of stream_device / stream_device_run's dict as they are."""
from dataclasses import dataclass, replace
from typing import Optional

import numpy as np

from . import _lib
from .tract import Tract
from ._dev import ArgError, Launch, float3 as _res, lines as _lines, tensor, work as _work
from ._host import packed as _packed
from .tractmap import str_sample, str_work_size


@dataclass
class Bundles:
    label: np.ndarray                     # int32 [nstr]: the nearest model if its distance is <= thresh_mm, else -1
    dist: np.ndarray                      # float32 [nstr]: the MDF distance to the nearest model in mm, whatever the threshold says
    flip: np.ndarray                      # uint8 [nstr]: 1 where the line runs against its nearest model
    counts: np.ndarray                    # uint32 [nmodels]: lines per bundle
    npoints: int = 0                      # points per line the distances were computed on
    lines: Optional[np.ndarray] = None    # float32 [nstr, npoints, 3]: the resampled lines (as stored, not flipped)


def _equal_length(tr: Tract, npoints, device):
    """the lines of `tr` as float32 [nstr, K, 3]: as they are if every line has `npoints` points already, else resampled"""
    npts = np.asarray(tr.npts)
    if npoints is None:
        if npts.size == 0 or (npts != npts[0]).any():
            raise ValueError("npoints=None takes lines that all have the same number of points")
        npoints = int(npts[0])
    K = int(npoints)
    if npts.size and (npts == K).all():
        return np.ascontiguousarray(np.asarray(tr.xyz, np.float32).reshape(-1, K, 3)), K
    return _resample_host(tr, K, None, device), K


def _resample_host(tr, K, flip, device):
    xyz, npts = _packed(tr)
    out = np.empty((npts.size, K, 3), np.float32)
    if flip is not None:
        flip = np.ascontiguousarray(np.asarray(flip).reshape(-1) != 0, dtype=np.uint8)
        if flip.size != npts.size:
            raise ValueError("%d flip flags for %d lines" % (flip.size, npts.size))
    _lib.check(_lib.lib().fib_str_resample(int(device), xyz.ctypes.data, npts.ctypes.data, npts.size, xyz.shape[0], _res(tr.volres), K,
                                           flip.ctypes.data if flip is not None else None, out.ctypes.data))
    return out


# ---- host tier --------------------------------------------------------------------------------------------------------------------
def str_resample(tr: Tract, npoints: int = 20, flip=None, device: int = 0) -> Tract:
    """Every line of `tr` with `npoints` points (2 to 256), equidistant in arc length measured in mm (voxel steps scaled by tr.volres);
    the first and the last point are kept as they are.  `flip`: per-line flags, a flagged line comes out reversed.  `seed_index` and
    `properties` are carried; `scalars` are DROPPED (they belong to the points that were there; sample the result again with
    str_sample).  Lines without points, or with a NaN / Inf coordinate, come out as NaN rows."""
    out = _resample_host(tr, int(npoints), flip, device)
    return replace(tr, xyz=out.reshape(-1, 3), npts=np.full(out.shape[0], int(npoints), np.int32), scalars=None)


def str_bundles(tr: Tract, models: Tract, thresh_mm: float, npoints: Optional[int] = None, device: int = 0) -> Bundles:
    """The nearest of the model lines in `models` for every line of `tr`, by MDF distance in mm (tr.volres): `label` is the model's
    index, or -1 where the distance exceeds `thresh_mm`; `flip` is 1 where the line runs against its model.  Lines and models are
    resampled to `npoints` points by the same kernel unless they have that many already (npoints=None: the models' own count)."""
    if npoints is None:
        mn = np.asarray(models.npts)
        if mn.size == 0 or (mn != mn[0]).any():
            raise ValueError("npoints=None takes models that all have the same number of points")
        npoints = int(mn[0])
    m, K = _equal_length(replace(models, volres=tr.volres), npoints, device)
    a, _ = _equal_length(tr, K, device)
    if m.shape[0] < 1:
        raise ValueError("at least one model")
    nl = a.shape[0]
    label, dist, flip = np.empty(nl, np.int32), np.empty(nl, np.float32), np.empty(nl, np.uint8)
    _lib.check(_lib.lib().fib_str_assign(int(device), a.ctypes.data, nl, K, m.ctypes.data, m.shape[0], _res(tr.volres), float(thresh_mm),
                                         label.ctypes.data, dist.ctypes.data, flip.ctypes.data, None))
    counts = np.bincount(label[label >= 0], minlength=m.shape[0]).astype(np.uint32)
    return Bundles(label=label, dist=dist, flip=flip, counts=counts, npoints=K, lines=a)


def str_centroids(tr: Tract, bundles: Bundles, device: int = 0) -> Tract:
    """The mean line of every bundle: a `Tract` of len(bundles.counts) lines of bundles.npoints points, every line oriented as its model
    before it is added (float64 sums divided by the count in float64, rounded to float32 once; NaN for a bundle without lines).  The
    per-bundle counts are its `properties`."""
    a = bundles.lines if bundles.lines is not None else _equal_length(tr, bundles.npoints, device)[0]
    nl, K = a.shape[0], a.shape[1]
    nm = int(np.asarray(bundles.counts).size)
    label = np.ascontiguousarray(bundles.label, dtype=np.int32)
    flip = np.ascontiguousarray(bundles.flip, dtype=np.uint8)
    sums, counts = np.zeros((nm, K, 3), np.float64), np.zeros(nm, np.uint32)
    _lib.check(_lib.lib().fib_str_centroids(int(device), a.ctypes.data, nl, K, label.ctypes.data, flip.ctypes.data, nm, 0, sums.ctypes.data,
                                            counts.ctypes.data))
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = (sums / counts.astype(np.float64)[:, None, None]).astype(np.float32)
    return replace(tr, xyz=mean.reshape(-1, 3), npts=np.full(nm, K, np.int32), seed_index=None, scalars=None, properties=counts.astype(np.float32))


def str_profile(tr: Tract, vols, models: Tract, thresh_mm: float, npoints: int = 20, device: int = 0) -> np.ndarray:
    """Along-tract profiles, float32 [nmodels, npoints, nframes]: the lines of `tr` are assigned to `models` (str_bundles), resampled to
    `npoints` points in their model's orientation, sampled in `vols` (str_sample: nearest voxel, NaN outside the volume), and the
    samples of every bundle averaged node by node (float64).  Lines with label -1 are left out; a bundle without lines is NaN."""
    b = str_bundles(tr, models, thresh_mm, npoints, device)
    K = b.npoints
    lines = _resample_host(tr, K, b.flip, device)
    nl = lines.shape[0]
    probe = Tract(lines.reshape(-1, 3), np.full(nl, K, np.int32), volsize=tr.volsize, volres=tr.volres, vox2ras=tr.vox2ras)
    s = str_sample(probe, vols, outside=float("nan"), device=device).scalars
    nf = s.shape[1]
    s = s.reshape(nl, K, nf).astype(np.float64)
    nm = int(b.counts.size)
    out = np.full((nm, K, nf), np.nan, np.float32)
    for m in np.flatnonzero(b.counts):
        out[m] = s[b.label == m].mean(axis=0).astype(np.float32)
    return out


# ---- device tier ------------------------------------------------------------------------------------------------------------------
def _rows(t, ref, what):
    import torch
    tensor(t, torch.float32, what, ref=ref, shape=(None, None, 3))
    return int(t.shape[0]), int(t.shape[1])


def _flip(flip, nl, ref):
    import torch
    return None if flip is None else tensor(flip, torch.uint8, "flip", ref=ref, n=nl, bool_ok=True)


def str_resample_device(xyz, npts, volres, npoints: int = 20, flip=None, out=None, status=None, work=None, stream=None):
    """fibd_str_resample on device tensors: xyz float32 [npoints, 3], npts int32 [nlines], flip uint8 / bool [nlines] or None.  Returns
    (out float32 [nlines, K, 3], status int64 [1]) -- device tensors, the call does not wait (`stream`, and `work` = None under a raw
    handle: _dev.Launch).  An invalid `npts` leaves `out` unwritten and sets status to -1; otherwise status is the number of lines."""
    import torch
    npnt, nl = _lines(xyz, npts)
    K = int(npoints)
    flip = _flip(flip, nl, xyz)
    with Launch(xyz, stream) as L:
        out = L.empty((nl, K, 3), torch.float32) if out is None else tensor(out, torch.float32, "out", ref=xyz, n=nl * K * 3)
        status = L.empty(1, torch.int64) if status is None else tensor(status, torch.int64, "status", ref=xyz, n=1)
        work, wb = _work(L, work, str_work_size, "str_work_size(nlines)", nl)
        _lib.check(_lib.lib().fibd_str_resample(xyz.data_ptr(), npts.data_ptr(), nl, npnt, _res(volres), K, flip.data_ptr() if flip is not None else None,
                                                out.data_ptr(), status.data_ptr(), work.data_ptr(), wb, L.sp))
    return out, status


def str_assign_device(lines, models, volres, thresh_mm: float, dist_all: bool = False, stream=None):
    """fibd_str_assign: lines float32 [nlines, K, 3], models float32 [nmodels, K, 3].  Returns a dict of device tensors: `label` int32
    [nlines], `dist` float32 [nlines], `flip` uint8 [nlines] and `dist_all` float32 [nlines, nmodels] (None unless asked for)."""
    import torch
    nl, K = _rows(lines, None, "lines")
    nm, Km = _rows(models, lines, "models")
    if Km != K or nm < 1:
        raise ArgError("models must be [nmodels >= 1, %d, 3] like the lines" % K)
    with Launch(lines, stream) as L:
        r = dict(label=L.empty(nl, torch.int32), dist=L.empty(nl, torch.float32), flip=L.empty(nl, torch.uint8),
                 dist_all=L.empty((nl, nm), torch.float32) if dist_all else None)
        _lib.check(_lib.lib().fibd_str_assign(lines.data_ptr(), nl, K, models.data_ptr(), nm, _res(volres), float(thresh_mm), r["label"].data_ptr(),
                                              r["dist"].data_ptr(), r["flip"].data_ptr(), r["dist_all"].data_ptr() if dist_all else None, L.sp))
    return r


def str_centroids_device(lines, label, flip, nmodels: int, out=None, stream=None):
    """fibd_str_centroids: returns (sums float64 [nmodels, K, 3], counts uint32 [nmodels]) on the device; `flip` may be None.  `out`: the
    pair of an earlier call to accumulate into (lines that arrive in batches).  sums / counts is the centroid; as float32 it is the
    `models` of the next str_assign_device."""
    import torch
    nl, K = _rows(lines, None, "lines")
    nm = int(nmodels)
    tensor(label, torch.int32, "label", ref=lines, n=nl)
    flip = _flip(flip, nl, lines)
    with Launch(lines, stream) as L:
        flags = 0
        if out is None:
            sums, counts = L.empty((nm, K, 3), torch.float64), L.empty(nm, torch.uint32)
        else:
            flags = _lib.FIB_CENTROIDS_ACCUMULATE
            sums, counts = out
            tensor(sums, torch.float64, "out sums", ref=lines, n=nm * K * 3)
            tensor(counts, torch.uint32, "out counts", ref=lines, n=nm)
        _lib.check(_lib.lib().fibd_str_centroids(lines.data_ptr(), nl, K, label.data_ptr(), flip.data_ptr() if flip is not None else None, nm, flags,
                                                 sums.data_ptr(), counts.data_ptr(), L.sp))
    return sums, counts
