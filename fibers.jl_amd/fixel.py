"""Tractogram weights: a weight per line, fitted so that the weighted track density of every fibre population ("fixel": one peak in
one voxel) matches that peak's amplitude (`str_weights`), and the weighted connectome that follows from it (`connectome_weighted`).
Not in the reference; the definitions (existence of a fixel, the fixel of a point, the fixed-point weights and the ISRA update) are
the "Tractogram weights" section of include/fibers_hip.h.  All compute is in csrc/fixel.hip; there is no NumPy path here but the
weighted matrix, which is host code by definition.

Bit-exact: the fixel ids, q, weights, td, mu and every count (integer sums, float64 operations in a stated order).  Bounded: `cost`
(a float64 sum whose order is free).  The fit is a fixed number of ISRA steps, not SIFT2's line search.

Host tier: `Tract` / `MRI` in, `TractWeights` out, through fib_str_weights.  Device tier: torch tensors in and out, through
fibd_fixel_* / fibd_str_weights on `stream`, taking the entries of stream_device_run's dict and of odf_rec_device's as they are."""
import ctypes as C
import math
from dataclasses import dataclass
from typing import List

import numpy as np

from . import _host, _lib
from ._dev import ArgError, Launch, lines as _lines, sync as _sync, tensor, work as _work
from ._host import packed as _packed
from .mri import MRI
from .tract import Tract

STATE_SLOTS = 16                    # FIB_FIXEL_STATE_SLOTS
Q_ONE = 1 << 20                     # the weight 1 in units of 2^-20
COUNTS = ("points_unassigned", "lines_unassigned", "lines_clamped", "lines_zero", "overflow")


class FixelOverflow(ArithmeticError):
    """a track density reached 2^44 units: the integer sums of the fit are no longer exact"""


@dataclass
class TractWeights:
    weights: np.ndarray               # float32 [nstr]: q * 2^-20
    q: np.ndarray                     # uint32 [nstr]: the weights in units of 2^-20
    td: List[MRI]                     # nvec volumes: the fitted density on the scale of f, 0 where no fixel exists
    mu: float                         # the scale between track density and amplitude, from the initial weights
    cost: np.ndarray                  # float64 [niter + 1]: the squared misfit over the fixels before the first and after every update
    counts: dict                      # points_unassigned, lines_unassigned, lines_clamped, lines_zero, overflow


def cos2_of(ang_thresh) -> float:
    """the float32 cos^2 of an angle threshold in degrees, as the ABI takes it (made in float64, rounded once)"""
    return float(np.float32(math.cos(math.radians(float(ang_thresh))) ** 2))


def _raise_on_overflow(n):
    if n:
        raise FixelOverflow("%d gathered track densities reached 2^44 units: the fit's integer sums are no longer exact "
                            "(fewer lines per fixel, or smaller start weights)" % n)


def _field(peak, f):
    """(peak list, f list) from lists of MRI / arrays, or from a GQI / DSI / CSD / MSMT result (its .peak and .qa / .f)"""
    if f is None:
        res = peak
        peak = res.peak
        f = res.qa if hasattr(res, "qa") else res.f
    return _host.as_list(peak), _host.as_list(f)


# ---- host tier --------------------------------------------------------------------------------------------------------------------
def str_weights(tr: Tract, peak, f=None, mask=None, f_thresh: float = 0.03, ang_thresh: float = 45, niter: int = 50, q0=None,
                device: int = 0) -> TractWeights:
    """A weight for every line of `tr` such that the weighted track density of every fixel matches its amplitude.  `peak` / `f`: lists
    of `MRI` (orientation volumes [nx, ny, nz, 3] and their amplitudes, as `stream` takes them; at most 3), or a `GQI` / `DSI` / `CSD`
    / `MSMT` result as `peak` alone, whose `.peak` and `.qa` / `.f` are used.  A fixel exists where the mask is non-zero, the amplitude is
    finite and above `f_thresh` and the direction is finite and not zero; a point belongs to the fixel of its voxel best aligned with
    the line's tangent if that lies within `ang_thresh` degrees.  Point counts stand for lengths: the lines must have a UNIFORM STEP
    (`stream`, `prob_stream` and `str_resample` write uniform steps).  The fit is `niter` steps of ISRA (the multiplicative update of
    non-negative least squares) from the weight 1, or from `q0` (uint32 [nstr], units of 2^-20); it is not SIFT2's line search.
    Raises `FixelOverflow` when a track density left the range in which the integer sums are exact."""
    peaks, fs = _field(peak, f)
    nvec = len(peaks)
    if not 1 <= nvec <= 3 or len(fs) != nvec:
        raise ValueError("one to three orientation volumes and one amplitude volume for each, not %d and %d" % (nvec, len(fs)))
    shape = _host.dims(tr.volsize)
    vols = [_host.volume(p, shape + (3,), np.float32, series=True, refuse="peak shape %s does not match the tract's volume %s") for p in peaks]
    fvols = [_host.volume(x, shape, np.float32, frame0=True, refuse="f shape %s does not match the tract's volume %s") for x in fs]
    m = None if mask is None else _host.mask(mask, shape, "!= 0", refuse="mask shape %s does not match the tract's volume %s")[0]
    xyz, npts = _packed(tr)
    nl, niter = int(npts.size), int(niter)
    if niter < 0:
        raise ValueError("niter must not be negative")
    start = None
    if q0 is not None:
        start = np.ascontiguousarray(q0, dtype=np.uint32).reshape(-1)
        if start.size != nl:
            raise ValueError("q0 holds %d weights for %d lines" % (start.size, nl))
    q = np.empty(nl, np.uint32)
    w = np.empty(nl, np.float32)
    td = np.empty(shape + (nvec,), np.float32, order="F")
    cost = np.empty(niter + 1, np.float64)
    mu = C.c_double(0.0)
    counts = (C.c_int64 * 5)()
    _lib.check(_lib.lib().fib_str_weights(int(device), xyz.ctypes.data, npts.ctypes.data, nl, xyz.shape[0], shape[0], shape[1], shape[2], nvec,
                                          _host.pointers(vols), _host.pointers(fvols), None if m is None else m.ctypes.data,
                                          float(np.float32(f_thresh)), cos2_of(ang_thresh), niter, None if start is None else start.ctypes.data,
                                          q.ctypes.data, w.ctypes.data, td.ctypes.data, C.byref(mu), cost.ctypes.data, counts))
    cnt = dict(zip(COUNTS, (int(v) for v in counts)))
    _raise_on_overflow(cnt["overflow"])
    ref = peaks[0] if isinstance(peaks[0], MRI) else None
    maps = [MRI(np.asfortranarray(td[..., k]), volres=tuple(tr.volres) if ref is None else ref.volres,
                vox2ras=np.array(tr.vox2ras if ref is None else ref.vox2ras, np.float32)) for k in range(nvec)]
    return TractWeights(weights=w, q=q, td=maps, mu=float(mu.value), cost=cost, counts=cnt)


def connectome_weighted(assign, weights, nnodes: int) -> np.ndarray:
    """The weighted connectome from the node pairs `str_connectome` returns (`Connectome.assign`, int32 [nstr, 2]) and the weights of
    `str_weights`: W float64 [nnodes + 1, nnodes + 1], symmetric, W[i, j] = the sum of the weights of the lines between nodes i and j
    (i <= j; a self-connection counts once, on the diagonal; row / column 0 holds the unassigned ends).  A float64 sum in line
    order.  `connectome_weighted(str_connectome(tr, labels).assign, str_weights(tr, g).weights, L)` is the whole chain."""
    a = np.asarray(assign, np.int64).reshape(-1, 2)
    w = np.asarray(weights, np.float64).reshape(-1)
    n = int(nnodes)
    if a.shape[0] != w.size:
        raise ValueError("%d node pairs for %d weights" % (a.shape[0], w.size))
    if a.size and (a.min() < 0 or a.max() > n):
        raise ValueError("a node outside 0 .. %d" % n)
    i, j = a.min(axis=1), a.max(axis=1)
    W = np.zeros((n + 1, n + 1), np.float64)
    np.add.at(W, (i, j), w)
    off = i != j
    np.add.at(W, (j[off], i[off]), w[off])
    return W


# ---- device tier ------------------------------------------------------------------------------------------------------------------
def _size(entry, *args):
    b = C.c_uint64(0)
    _lib.check(getattr(_lib.lib(), entry)(*args, C.byref(b)))
    return int(b.value)


def str_weights_work_size(nlines: int, npoints: int, nvec: int, nvox: int) -> int:
    """bytes of device scratch str_weights_device needs (fibd_str_weights_work_size)"""
    return _size("fibd_str_weights_work_size", int(nlines), int(npoints), int(nvec), int(nvox))


def _str_work(nlines):
    return _size("fibd_str_work_size", int(nlines))


def _field_device(ovec, f, mask, shape, ref):
    """the checks of a device peak field: ovec[k] float32 [3, nvox], f[k] float32 [nvox], mask uint8 / bool [nvox] or None, all on
    the device of `ref` -> (nvec, nvox, pointer arrays, mask pointer, the tensors kept alive)"""
    import torch
    nx, ny, nz = (int(v) for v in shape)
    nvox = nx * ny * nz
    ovec, f = list(ovec), list(f)
    nvec = len(ovec)
    if not 1 <= nvec <= 3 or len(f) != nvec:
        raise ArgError("one to three orientation tensors and one amplitude tensor for each, not %d and %d" % (nvec, len(f)))
    for k in range(nvec):
        tensor(ovec[k], torch.float32, "ovec[%d] [3, nvox]" % k, ref=ref, n=3 * nvox)
        tensor(f[k], torch.float32, "f[%d] [nvox]" % k, ref=ref, n=nvox)
    if mask is not None:
        mask = tensor(mask, torch.uint8, "mask", ref=ref, n=nvox, bool_ok=True)
    ov = (C.c_void_p * nvec)(*[t.data_ptr() for t in ovec])
    fv = (C.c_void_p * nvec)(*[t.data_ptr() for t in f])
    return nvec, nvox, ov, fv, (mask.data_ptr() if mask is not None else None), (ovec, f, mask)


def fixel_assign_device(xyz, npts, shape, ovec, f, mask=None, f_thresh: float = 0.03, ang_thresh: float = 45, cos2=None, out=None, work=None,
                        stream=None):
    """fibd_fixel_assign on device tensors: xyz float32 [npoints, 3], npts int32 [nlines], ovec[k] float32 [3, nvox], f[k] float32
    [nvox].  Returns (ids int32 [npoints]: k * nvox + voxel or -1, counts int64 [2] = points unassigned (-1 for an invalid `npts`),
    lines without an assigned point).  `cos2`: the float32 threshold itself, in place of `ang_thresh` degrees."""
    import torch
    npnt, nl = _lines(xyz, npts)
    nvec, nvox, ov, fv, mp, keep = _field_device(ovec, f, mask, shape, xyz)
    c2 = cos2_of(ang_thresh) if cos2 is None else float(np.float32(cos2))
    with Launch(xyz, stream) as L:
        ids = L.empty(npnt, torch.int32) if out is None else tensor(out, torch.int32, "out", ref=xyz, n=npnt)
        counts = L.empty(2, torch.int64)
        work, wb = _work(L, work, _str_work, "str_work_size(nlines)", nl)
        _lib.check(_lib.lib().fibd_fixel_assign(xyz.data_ptr(), npts.data_ptr(), nl, npnt, int(shape[0]), int(shape[1]), int(shape[2]), nvec, ov, fv, mp,
                                                float(np.float32(f_thresh)), c2, ids.data_ptr(), counts.data_ptr(), work.data_ptr(), wb, L.sp))
    del keep
    return ids, counts


def fixel_td_device(ids, npts, q, nfixels: int, out=None, work=None, stream=None):
    """fibd_fixel_td: the track density of the weights q (uint32 [nlines], units of 2^-20) along the ids of fixel_assign_device:
    uint64 [nfixels] in units of 2^-20, as an int64 tensor (the same bits)."""
    import torch
    npnt = tensor(ids, torch.int32, "ids", ref=npts).numel()
    nl = tensor(npts, torch.int32, "npts").numel()
    tensor(q, torch.uint32, "q", ref=npts, n=nl)
    nf = int(nfixels)
    with Launch(npts, stream) as L:
        td = L.empty(nf, torch.int64) if out is None else tensor(out, torch.int64, "out", ref=npts, n=nf)
        work, wb = _work(L, work, _str_work, "str_work_size(nlines)", nl)
        _lib.check(_lib.lib().fibd_fixel_td(ids.data_ptr(), npts.data_ptr(), nl, npnt, q.data_ptr(), nf, td.data_ptr(), work.data_ptr(), wb, L.sp))
    return td


def str_weights_device(xyz, npts, shape, ovec, f, mask=None, f_thresh: float = 0.03, ang_thresh: float = 45, niter: int = 50, q0=None, cos2=None,
                       work=None, stream=None, check: bool = True):
    """fibd_str_weights on device tensors (arguments as fixel_assign_device; q0 uint32 [nlines] or None).  Returns a dict of device
    tensors: `weights` float32 [nlines], `q` uint32 [nlines], `td` float32 [nvec, nvox], `cost` float64 [niter + 1] and `state` int64
    [16] (the header's slots: mu = state[1:2].view(torch.float64), counts = state[5:10]).  check=True waits for the result and raises
    `FixelOverflow` when the overflow counter is not zero; check=False does not wait and leaves the counter to the caller."""
    import torch
    npnt, nl = _lines(xyz, npts)
    nvec, nvox, ov, fv, mp, keep = _field_device(ovec, f, mask, shape, xyz)
    niter = int(niter)
    if niter < 0:
        raise ArgError("niter must not be negative")
    if q0 is not None:
        tensor(q0, torch.uint32, "q0", ref=xyz, n=nl)
    c2 = cos2_of(ang_thresh) if cos2 is None else float(np.float32(cos2))
    with Launch(xyz, stream) as L:
        out = dict(weights=L.empty(nl, torch.float32), q=L.empty(nl, torch.uint32), td=L.empty((nvec, nvox), torch.float32),
                   cost=L.empty(niter + 1, torch.float64), state=L.empty(STATE_SLOTS, torch.int64))
        work, wb = _work(L, work, str_weights_work_size, "str_weights_work_size(nlines, npoints, nvec, nvox)", nl, npnt, nvec, nvox)
        _lib.check(_lib.lib().fibd_str_weights(xyz.data_ptr(), npts.data_ptr(), nl, npnt, int(shape[0]), int(shape[1]), int(shape[2]), nvec, ov, fv, mp,
                                               float(np.float32(f_thresh)), c2, niter, q0.data_ptr() if q0 is not None else None,
                                               out["q"].data_ptr(), out["weights"].data_ptr(), out["td"].data_ptr(), out["cost"].data_ptr(),
                                               out["state"].data_ptr(), work.data_ptr(), wb, L.sp))
    del keep
    if check:
        _sync(stream)
        _raise_on_overflow(int(out["state"][9].item()))
    return out
