"""mri_register and dwi_moco: intensity-based rigid / affine registration by normalised mutual information, and the motion correction
of a DWI series built on it.  Not in the reference; the definitions (pyramid, range, binning, joint histogram, matrices, cost,
pattern search) are the "Registration" section of include/fibers_hip.h, restated in tests/register_ref.py.

The hot path is csrc/register.hip: fibd_reg_hist counts the joint histograms of every candidate matrix of every live frame in one
launch.  The decisions are the library's host code (fib_reg_search_*: float64, no GPU needed), and fibd_reg_run moves histograms
between the two, once per round.  There is no NumPy path for the compute; what this module computes itself are the float64 matrices of
a result (`reg_xform`), the mean that is dwi_moco's default target and the rotation of `bvec`.

Host tier: `mri_register(moving, fixed)`, `dwi_moco(dwi)` take `MRI`s and go through fib_mri_register on one device.  Device tier:
`vol_halve_device`, `vol_range_device`, `reg_hist_device`, `reg_run_device`, `mri_register_device` on torch tensors."""
import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _host, _lib
from ._dev import ArgError, Launch, tensor, work as _work
from .mask import default_frames
from .mri import MRI
from .xform import Xform, round32, voxrot_of

TRACE_ROW = 29                      # FIB_REG_TRACE_ROW


@dataclass
class Registration:
    """Container for outputs of mri_register: `xfm` (an Xform, in = moving, out = fixed: mri_xform(xfm, moving) lands on the fixed grid),
    `theta` (float64 [dof]), `cost` (the NMI of theta at level 0) and `trace` (one dict per iteration: level, ndof, index, moved, cost,
    costs)"""
    xfm: Xform
    theta: np.ndarray
    cost: float
    trace: list


@dataclass
class Moco:
    """Container for outputs of dwi_moco: `dwi` (the corrected series on the target's grid, bvec reoriented), `theta` [nframes, 6], `xfm`
    (one Xform per frame), `cost` [nframes] and `trace` (one list per frame)"""
    dwi: MRI
    theta: np.ndarray
    xfm: list
    cost: np.ndarray
    trace: list


# ---- the library's host code ------------------------------------------------------------------------------------------------------
def _i3(v):
    return (C.c_int32 * 3)(*[int(x) for x in v])


def _f3(v):
    return (C.c_float * 3)(*[float(x) for x in v])


def reg_levels(fixed_size, moving_size):
    """the default number of pyramid levels (fib_reg_levels)"""
    n = C.c_int()
    _lib.check(_lib.lib().fib_reg_levels(_i3(fixed_size), _i3(moving_size), C.byref(n)))
    return int(n.value)


def reg_matrix(theta, fixed_vox2ras, fixed_size, moving_vox2ras, level=0, with_G=False):
    """out2in of a level (fib_reg_matrix): float32 [4, 4], fixed voxel -> moving voxel; with_G: (out2in, G float64 [4, 4])"""
    th = np.ascontiguousarray(theta, np.float64).reshape(-1)
    M, G = (C.c_float * 16)(), (C.c_double * 16)()
    _lib.check(_lib.lib().fib_reg_matrix(th.ctypes.data, int(th.size), _host.m16(fixed_vox2ras), _i3(fixed_size), _host.m16(moving_vox2ras), int(level),
                                         M, G))
    M = np.array(M, np.float32).reshape(4, 4)
    return (M, np.array(G, np.float64).reshape(4, 4)) if with_G else M


def reg_nmi(hist, nfinite, min_overlap=0.5):
    """the cost of one joint histogram [nbins, nbins] (fib_reg_nmi)"""
    h = np.ascontiguousarray(hist).astype(np.uint32)
    if h.ndim != 2 or h.shape[0] != h.shape[1]:
        raise ValueError("hist must be [nbins, nbins], not %s" % (h.shape,))
    c = C.c_double()
    _lib.check(_lib.lib().fib_reg_nmi(h.ctypes.data, int(h.shape[0]), int(nfinite), float(min_overlap), C.byref(c)))
    return float(c.value)


class Search:
    """fib_reg_search: the pattern search as the library's state machine.  `jobs()` -> (level, matrices float32 [n, 16]; n == 0 when it
    has finished), `feed(hist, nfinite)` takes their histograms, `result()` -> (theta [dof], cost, trace)."""

    def __init__(self, dof, fixed_size, fixed_res, fixed_vox2ras, moving_size, moving_vox2ras, levels=0, halvings=4, maxit=80, min_overlap=0.5,
                 theta0=None):
        self._h, self.dof = C.c_void_p(), int(dof)
        t0 = None if theta0 is None else np.ascontiguousarray(theta0, np.float64).reshape(-1)
        if t0 is not None and t0.size != self.dof:
            raise ValueError("theta0 must hold %d values" % self.dof)
        _lib.check(_lib.lib().fib_reg_search_create(self.dof, _i3(fixed_size), _f3(fixed_res), _host.m16(fixed_vox2ras), _i3(moving_size),
                                                    _host.m16(moving_vox2ras), int(levels or 0), int(halvings), int(maxit), float(min_overlap),
                                                    None if t0 is None else t0.ctypes.data, C.byref(self._h)))

    def jobs(self):
        lv, n, m = C.c_int(), C.c_int(), np.empty((24, 16), np.float32)
        _lib.check(_lib.lib().fib_reg_search_jobs(self._h, C.byref(lv), C.byref(n), m.ctypes.data))
        return int(lv.value), m[: n.value]

    def feed(self, hist, nfinite):
        h = np.ascontiguousarray(hist).astype(np.uint32)
        _lib.check(_lib.lib().fib_reg_search_feed(self._h, h.ctypes.data, int(h.shape[-1]), int(nfinite)))

    def result(self):
        th, c, n = np.zeros(12), C.c_double(), C.c_int()
        _lib.check(_lib.lib().fib_reg_search_result(self._h, th.ctypes.data, C.byref(c), C.byref(n), None, 0))
        tr = np.empty((max(1, n.value), TRACE_ROW))
        _lib.check(_lib.lib().fib_reg_search_result(self._h, None, None, None, tr.ctypes.data, int(n.value)))
        return th[: self.dof].copy(), float(c.value), tr[: n.value]

    def close(self):
        if self._h:
            _lib.lib().fib_reg_search_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def trace_list(rows):
    """trace rows [niter, 29] -> one dict per iteration"""
    return [dict(level=int(r[0]), ndof=int(r[1]), index=int(r[2]), moved=bool(r[3]), cost=float(r[4]), costs=r[5:5 + 2 * int(r[1])].copy())
            for r in np.asarray(rows).reshape(-1, TRACE_ROW)]


def reg_xform(theta, moving_size, moving_res, moving_vox2ras, fixed_size, fixed_res, fixed_vox2ras) -> Xform:
    """the Xform of a result, in = moving, out = fixed: ras2ras = float32(inv(G)), vox2vox = float32(inv(V_fix) inv(G) V_mov)"""
    _, G = reg_matrix(theta, fixed_vox2ras, fixed_size, moving_vox2ras, 0, with_G=True)
    Gi = np.linalg.inv(G)
    Vf, Vm = (np.asarray(v, np.float32).astype(np.float64).reshape(4, 4) for v in (fixed_vox2ras, moving_vox2ras))
    x = Xform(insize=moving_size, outsize=fixed_size, inres=moving_res, outres=fixed_res, invox2ras=np.array(moving_vox2ras, np.float32),
              outvox2ras=np.array(fixed_vox2ras, np.float32))
    x.ras2ras = round32(Gi)
    x.vox2vox = round32(np.linalg.inv(Vf) @ Gi @ Vm)
    x.voxrot = voxrot_of(x.vox2vox)
    return x


# ---- device tier ------------------------------------------------------------------------------------------------------------------
def _shape(shape):
    nx, ny, nz = _host.dims(shape)
    if nx <= 0 or ny <= 0 or nz <= 0:
        raise ArgError("shape %s: nx, ny and nz must be positive" % (tuple(shape),))
    return nx, ny, nz


def halved(shape):
    """the size of the next pyramid level: ceil(n / 2) per axis"""
    return tuple((int(n) + 1) // 2 for n in shape)


def vol_halve_device(vol, shape, out=None, stream=None):
    """fibd_vol_halve: vol float32 [nframes, nx*ny*nz] (or [nvox]; x fastest) -> the next pyramid level [nframes, prod(halved(shape))]
    (or [nvox']).  `out`: such a tensor to write into (not overlapping vol).  The call does not wait for the kernel."""
    import torch
    nx, ny, nz = _shape(shape)
    nvi, nvo = nx * ny * nz, int(np.prod(halved(shape)))
    tensor(vol, torch.float32, "vol [nframes, nx*ny*nz]", unit=nvi)
    nf = vol.numel() // nvi
    with Launch(vol, stream) as L:
        if out is None:
            out = L.empty((nf, nvo) if vol.dim() > 1 else (nvo,), torch.float32)
        else:
            tensor(out, torch.float32, "out [nframes, nvox']", ref=vol, n=nf * nvo)
        _lib.check(_lib.lib().fibd_vol_halve(vol.data_ptr(), nx, ny, nz, nf, out.data_ptr(), L.sp))
    return out


def vol_range_device(vol, nvox, nbins=32, out=None, stream=None):
    """fibd_vol_range: vol float32 [nframes, nvox] (or [nvox]) -> float32 [nframes, 4]: lo, hi, scale and, as the bits of a uint32, the
    number of finite values (`range_table` reads it on the host).  The call does not wait for the kernel."""
    import torch
    nvox = int(nvox)
    tensor(vol, torch.float32, "vol [nframes, nvox]", unit=nvox)
    nf = vol.numel() // nvox
    with Launch(vol, stream) as L:
        if out is None:
            out = L.empty((nf, 4), torch.float32)
        else:
            tensor(out, torch.float32, "out [nframes, 4]", ref=vol, n=4 * nf)
        _lib.check(_lib.lib().fibd_vol_range(vol.data_ptr(), nvox, nf, int(nbins), out.data_ptr(), L.sp))
    return out


def range_table(rng):
    """a range tensor on the host: (float32 [nframes, 3] = lo, hi, scale; int64 [nframes] = finite values); waits for the tensor"""
    r = rng.cpu().numpy().reshape(-1, 4)
    return r[:, :3].copy(), r[:, 3].copy().view(np.uint32).astype(np.int64)


def reg_hist_work_size(njobs):
    """bytes of device workspace reg_hist_device needs (fibd_reg_hist_work_size)"""
    b = C.c_uint64()
    _lib.check(_lib.lib().fibd_reg_hist_work_size(int(njobs), C.byref(b)))
    return int(b.value)


def reg_hist_device(fixed, fixed_shape, fixed_range, moving, moving_shape, moving_range, job_frame, job_out2in, nbins=32, out=None, work=None,
                    stream=None):
    """fibd_reg_hist: the joint histograms int32 [njobs, nbins, nbins] of `fixed` (float32 [nvox_f]) against the frames of `moving`
    (float32 [nframes, nvox_m]) for the jobs (job_frame[j], job_out2in[j] float32 [4, 4]: fixed voxel -> moving voxel; host arrays).
    fixed_range [1, 4] and moving_range [nframes, 4] are vol_range_device's tensors.  `out`, `work`: buffers to use (work: at least
    reg_hist_work_size(njobs) bytes).  The call does not wait for the kernel."""
    import torch
    nxf, nyf, nzf = _shape(fixed_shape)
    nxm, nym, nzm = _shape(moving_shape)
    nvm = nxm * nym * nzm
    tensor(fixed, torch.float32, "fixed", n=nxf * nyf * nzf)
    tensor(moving, torch.float32, "moving [nframes, nvox]", ref=fixed, unit=nvm)
    nf = moving.numel() // nvm
    tensor(fixed_range, torch.float32, "fixed_range [1, 4]", ref=fixed, n=4)
    tensor(moving_range, torch.float32, "moving_range [nframes, 4]", ref=fixed, n=4 * nf)
    fr = np.ascontiguousarray(np.asarray(job_frame).reshape(-1), dtype=np.int32)
    mats = np.ascontiguousarray(job_out2in, np.float32).reshape(-1, 16)
    if fr.size == 0 or fr.size != mats.shape[0]:
        raise ArgError("job_frame [njobs] and job_out2in [njobs, 4, 4] must name the same, positive number of jobs")
    nj, nb = int(fr.size), int(nbins)
    with Launch(fixed, stream) as L:
        if out is None:
            out = L.empty((nj, max(nb, 0), max(nb, 0)), torch.int32)
        else:
            tensor(out, torch.int32, "out [njobs, nbins, nbins]", ref=fixed, n=nj * nb * nb)
        w, wb = _work(L, work, reg_hist_work_size, "reg_hist_work_size", nj)
        _lib.check(_lib.lib().fibd_reg_hist(fixed.data_ptr(), nxf, nyf, nzf, fixed_range.data_ptr(), moving.data_ptr(), nxm, nym, nzm, nf,
                                            moving_range.data_ptr(), fr.ctypes.data, mats.ctypes.data, nj, nb, out.data_ptr(), w.data_ptr(), wb, L.sp))
    return out


def reg_run_work_size(fixed_shape, moving_shape, nframes, nsearch, levels, nbins=32):
    """bytes of device workspace reg_run_device needs (fibd_reg_run_work_size)"""
    b = C.c_uint64()
    _lib.check(_lib.lib().fibd_reg_run_work_size(_i3(fixed_shape), _i3(moving_shape), int(nframes), int(nsearch), int(levels), int(nbins), C.byref(b)))
    return int(b.value)


def reg_run_device(searches, frames, fixed, fixed_shape, moving, moving_shape, levels, nbins=32, work=None, stream=None):
    """fibd_reg_run: every `Search` of `searches` (search s against frame frames[s] of moving float32 [nframes, nvox_m]; fixed float32
    [nvox_f]) run to its end.  The pyramids and the ranges are made in `work`; every round the searches that wait at the coarsest pending
    level share ONE joint-histogram launch, and the call waits for the histograms once per round.  Results: `Search.result()`."""
    import torch
    fs, ms = _shape(fixed_shape), _shape(moving_shape)
    tensor(fixed, torch.float32, "fixed", n=int(np.prod(fs)))
    tensor(moving, torch.float32, "moving [nframes, nvox]", ref=fixed, unit=int(np.prod(ms)))
    nf = moving.numel() // int(np.prod(ms))
    fr = np.ascontiguousarray(np.asarray(frames).reshape(-1), dtype=np.int32)
    if fr.size == 0 or fr.size != len(searches):
        raise ArgError("frames must name one frame per search")
    handles = (C.c_void_p * len(searches))(*[s._h for s in searches])
    with Launch(fixed, stream) as L:
        w, wb = _work(L, work, reg_run_work_size, "reg_run_work_size", fs, ms, nf, len(searches), levels, nbins)
        if w.data_ptr() % 16:
            raise ArgError("work must be 16-byte aligned")
        _lib.check(_lib.lib().fibd_reg_run(handles, fr.ctypes.data, len(searches), fixed.data_ptr(), _i3(fs), moving.data_ptr(), _i3(ms), nf, int(levels),
                                           int(nbins), w.data_ptr(), wb, L.sp))


def _levels(levels, fshape, mshape):
    return reg_levels(fshape, mshape) if not levels else int(levels)


def mri_register_device(moving, moving_shape, moving_vox2ras, fixed, fixed_shape, fixed_res, fixed_vox2ras, dof=6, nbins=32, levels=None,
                        halvings=4, maxit=80, min_overlap=0.5, theta0=None, work=None, stream=None):
    """Device tier of mri_register: every frame of moving float32 [nframes, nvox_m] (or [nvox_m]) registered to fixed float32 [nvox_f] (x
    fastest), with their sizes and vox2ras and the fixed voxel size.  Returns a list of (theta float64 [dof], cost, trace rows [niter, 29]),
    one per frame.  Waits for the histograms once per round."""
    import torch
    fs, ms = _shape(fixed_shape), _shape(moving_shape)
    nf = tensor(moving, torch.float32, "moving [nframes, nvox]", unit=int(np.prod(ms))).numel() // int(np.prod(ms))
    nl = _levels(levels, fs, ms)
    searches = []
    try:
        for _ in range(nf):
            searches.append(Search(dof, fs, fixed_res, fixed_vox2ras, ms, moving_vox2ras, nl, halvings, maxit, min_overlap, theta0))
        reg_run_device(searches, range(nf), fixed, fs, moving, ms, nl, nbins, work=work, stream=stream)
        return [s.result() for s in searches]
    finally:
        for s in searches:
            s.close()


# ---- host tier --------------------------------------------------------------------------------------------------------------------
def _as_mri(v):
    return v if isinstance(v, MRI) else MRI(np.asarray(v))


def _register(moving, moving_vox2ras, fixed, dof, nbins, levels, device, resample, halvings=4, maxit=80, min_overlap=0.5):
    """fib_mri_register: every frame of the float32 series `moving` [nx, ny, nz, N] (Fortran order) to frame 0 of the MRI `fixed` ->
    (theta [N, dof], cost [N], [trace rows], resampled [fixed size, N] or None)"""
    fix = _host.volume(fixed, dtype=np.float32, frame0=True)
    nf, ms, fs = int(moving.shape[3]), moving.shape[:3], fix.shape
    rows = 5 * int(maxit) if maxit > 0 else 1
    theta, cost, niter = np.zeros((nf, 12)), np.zeros(nf), np.zeros(nf, np.int32)
    trace = np.empty((nf, rows, TRACE_ROW))
    out = np.empty(tuple(fs) + (nf,), np.float32, order="F") if resample else None
    _lib.check(_lib.lib().fib_mri_register(int(device), moving.ctypes.data, _i3(ms), _host.m16(moving_vox2ras), nf, fix.ctypes.data, _i3(fs),
                                           _f3(fixed.volres), _host.m16(fixed.vox2ras), int(dof), int(nbins), int(levels or 0), int(halvings), int(maxit),
                                           float(min_overlap), theta.ctypes.data, cost.ctypes.data, niter.ctypes.data, trace.ctypes.data, rows,
                                           None if out is None else out.ctypes.data))
    return theta[:, :dof].copy(), cost, [trace[f, :niter[f]].copy() for f in range(nf)], out


def mri_register(moving, fixed, dof=6, nbins=32, levels=None, frame=0, device=0) -> Registration:
    """Register frame `frame` of `moving` to frame 0 of `fixed` (MRIs): dof 6 (rigid) or 12 (affine), NMI of an nbins x nbins joint
    histogram, a pyramid of `levels` levels (None: as many, up to 4, as keep every dimension >= 8).  The result's `xfm` takes the
    moving volume onto the fixed grid: mri_xform(r.xfm, moving)."""
    moving, fixed = _as_mri(moving), _as_mri(fixed)
    vol = _host.volume(moving, dtype=np.float32, series=True)
    if not 0 <= int(frame) < vol.shape[3]:
        raise ValueError("frame %d of a moving series of %d frames" % (frame, vol.shape[3]))
    theta, cost, rows, _ = _register(vol[..., int(frame):int(frame) + 1], moving.vox2ras, fixed, dof, nbins, levels, device, False)
    x = reg_xform(theta[0], moving.volsize, moving.volres, moving.vox2ras, fixed.volsize, fixed.volres, fixed.vox2ras)
    return Registration(x, theta[0], float(cost[0]), trace_list(rows[0]))


def frame_mean(dwi: MRI, frames):
    """dwi_mask's mean of the listed frames ("Brain mask", include/fibers_hip.h): the float64 sequential sum of the float32 samples in
    the list's order from +0, divided by the count in float64, rounded to float32 once"""
    acc = np.zeros(dwi.volsize, np.float64, order="F")
    for f in frames:
        acc = acc + np.asarray(dwi.vol[..., int(f)], np.float32).astype(np.float64)
    return np.asfortranarray((acc / float(len(frames))).astype(np.float32))


def rotate_bvec(bvec, vox2vox):
    """bvec reoriented through the rotational part of a vox2vox (voxrot_of's U Vt, kept in float64), applied in float64, rounded once"""
    u, _, vt = np.linalg.svd(np.asarray(vox2vox, np.float32).astype(np.float64).reshape(4, 4)[:3, :3])
    return (np.asarray(bvec, np.float32).astype(np.float64).reshape(-1, 3) @ (u @ vt).T).astype(np.float32)


def dwi_moco(dwi, target=None, nbins=32, levels=None, device=0) -> Moco:
    """Motion correction of a DWI series: every frame is registered (dof 6, from theta = 0) to `target` (an MRI; None: the mean of the
    frames of the smallest b-value, dwi_mask's b0 mean) and resampled onto the target's grid, trilinear, 0 outside; bvec rows are rotated
    by the rotational part of their frame's transform, bval is carried.  The frames share their launches."""
    dwi = _as_mri(dwi)
    if target is None:
        target = MRI(frame_mean(dwi, default_frames(dwi.bval)), volres=dwi.volres, vox2ras=dwi.vox2ras.copy())
    target = _as_mri(target)
    vol = _host.volume(dwi, dtype=np.float32, series=True)
    nf = vol.shape[3]
    theta, cost, rows, out = _register(vol, dwi.vox2ras, target, 6, nbins, levels, device, True)
    xfms = [reg_xform(theta[f], dwi.volsize, dwi.volres, dwi.vox2ras, target.volsize, target.volres, target.vox2ras) for f in range(nf)]
    bvec = None
    if dwi.bvec is not None and len(dwi.bvec):
        bvec = np.stack([rotate_bvec(dwi.bvec[f], x.vox2vox)[0] for f, x in enumerate(xfms)])
    moved = MRI(out, bval=None if dwi.bval is None else dwi.bval.copy(), bvec=bvec, volres=target.volres, vox2ras=target.vox2ras.copy(), tr=dwi.tr)
    return Moco(moved, theta, xfms, cost, [trace_list(r) for r in rows])
