"""csd_rec: constrained spherical deconvolution, the fibre ODF of single-shell data (not in the reference; the definition is
include/fibers_hip.h "Constrained spherical deconvolution" and DESIGN.md §5).

`csd_rec(dwi, mask, response)` takes host `MRI`s and goes through the host-buffer C ABI (fib_csd_rec); `CsdPlan` + `csd_rec_device`
are the device-resident form on torch tensors (fibd_csd_rec).  `csd_design` builds the tables on the host (no GPU needed);
`csd_response` estimates the response from a tensor fit.  The result feeds `prob_stream(csd, odf_dirs)` and
`stream(csd.peak, f=csd.f)`."""
import ctypes as C
from dataclasses import dataclass
from typing import List

import numpy as np

from . import _host, _lib
from ._dev import ArgError, Launch, Plan, fit_args, tensor
from .mri import MRI
from .nifti import csd_write  # noqa: F401
from .odf import ODF, sphere_724

DEFAULTS = dict(lmax=8, b0_thresh=50.0, shell=None, b_tol=0.05, lam=1.0, tau=0.1, niter=50)


@dataclass
class CSD:
    """Container for outputs of a CSD reconstruction: the harmonic coefficients (n frames), the fibre ODF on the half sphere of
    `odf_dirs`, its three largest peaks (unit vectors, 3 frames each) with their amplitudes, and the solves each voxel took"""
    sh: MRI
    odf: MRI
    peak: List[MRI]
    f: List[MRI]
    niter: MRI


def ncoef(lmax):
    """columns of the even harmonic basis up to lmax"""
    return (int(lmax) + 1) * (int(lmax) + 2) // 2


def _params(response, lmax, b0_thresh, shell, b_tol, lam, tau, niter):
    lpar, lperp, s0 = (float(v) for v in response)
    return _lib.CsdParams(int(lmax), lpar, lperp, s0, float(b0_thresh), 0.0 if shell is None else float(shell), float(b_tol), float(lam),
                          float(tau), int(niter))


def csd_response(dti, mask, fa_thresh: float = 0.7):
    """The single-fibre response from a tensor fit: (mean eigval1, mean (eigval2 + eigval3) / 2, mean s0) over the voxels inside the
    mask whose fa exceeds fa_thresh, summed in float64 on the host.  Raises when no voxel qualifies."""
    m, _ = _host.mask(mask)
    fa = dti.fa.vol[..., 0] if dti.fa.vol.ndim == 4 else dti.fa.vol
    sel = (m != 0) & (fa > fa_thresh)
    if not sel.any():
        raise ValueError("no voxel inside the mask has fa > %g: the response cannot be estimated" % fa_thresh)

    def mean(x):
        v = x.vol[..., 0] if x.vol.ndim == 4 else x.vol
        return float(np.mean(v[sel], dtype=np.float64))
    return mean(dti.eigval1), 0.5 * (mean(dti.eigval2) + mean(dti.eigval3)), mean(dti.s0)


def csd_design(bval, bvec, response, odf_dirs: ODF = sphere_724, lmax: int = DEFAULTS["lmax"], b0_thresh: float = DEFAULTS["b0_thresh"],
               shell=DEFAULTS["shell"], b_tol: float = DEFAULTS["b_tol"], lam: float = DEFAULTS["lam"]):
    """The reconstruction's tables, built on the host in float64 and rounded once: dict(frames int32 [nshell] (0-based), R float32
    [lmax / 2 + 1], X [nshell, n], B [nreg, n], Y [nreg, n], rank).  response = (lambda_para, lambda_perp, s0).  A shell of fewer than n
    frames, or one whose kernel matrix has a rank below n, raises FibersError (code -1)."""
    bval, bv = _host.table_args(bval, bvec)
    nvol, n, nreg = int(bval.shape[0]), ncoef(lmax), odf_dirs.nvert
    v = _host.directions(odf_dirs)
    p = _params(response, lmax, b0_thresh, shell, b_tol, lam, DEFAULTS["tau"], DEFAULTS["niter"])
    frames = np.zeros(nvol, np.int32)
    R = np.zeros(5, np.float32)
    X = np.zeros(nvol * max(n, 1), np.float32)
    B = np.zeros((nreg, max(n, 1)), np.float32, order="F")
    Y = np.zeros((nreg, max(n, 1)), np.float32, order="F")
    nshell, rank = C.c_int(0), C.c_int(0)
    _lib.check(_lib.lib().fib_csd_design(bval.ctypes.data, bv.ctypes.data, nvol, v.ctypes.data, v.shape[0], C.byref(p), frames.ctypes.data,
                                         C.byref(nshell), R.ctypes.data, X.ctypes.data, B.ctypes.data, Y.ctypes.data, C.byref(rank)))
    ns = int(nshell.value)
    return dict(frames=frames[:ns].copy(), R=R[:int(lmax) // 2 + 1].copy(), X=X[:ns * n].reshape((ns, n), order="F").copy(order="F"),
                B=B, Y=Y, rank=int(rank.value))


def csd_rec(dwi: MRI, mask: MRI, response, odf_dirs: ODF = sphere_724, lmax: int = DEFAULTS["lmax"],
            b0_thresh: float = DEFAULTS["b0_thresh"], shell=DEFAULTS["shell"], b_tol: float = DEFAULTS["b_tol"], lam: float = DEFAULTS["lam"],
            tau: float = DEFAULTS["tau"], niter: int = DEFAULTS["niter"], device: int = 0) -> CSD:
    """Constrained spherical deconvolution of one shell of `dwi` and return a `CSD` structure.  response = (lambda_para, lambda_perp,
    s0), e.g. from `csd_response`.  device: a GPU index, or _lib.DEVICE_ALL for the device set declared with fibers_jl_amd.init()."""
    bval, bvec = _host.check_tables(dwi)
    vol, m, mdt = _host.fit_inputs(dwi, mask)
    nx, ny, nz, nvol = vol.shape
    v, fc = _host.directions(odf_dirs, faces=True)
    p = _params(response, lmax, b0_thresh, shell, b_tol, lam, tau, niter)
    if int(lmax) not in (2, 4, 6, 8):
        raise ValueError("lmax must be 2, 4, 6 or 8")
    sh, odf, nit, *pf = _host.fit_outputs(dwi, mask, [ncoef(lmax), odf_dirs.nvert, 1, 3, 3, 3, 1, 1, 1])
    peak, f = pf[:3], pf[3:]
    o = _lib.CsdOut(sh.vol.ctypes.data, odf.vol.ctypes.data, nit.vol.ctypes.data, _host.pointers(peak), _host.pointers(f))
    _lib.check(_lib.lib().fib_csd_rec(device, vol.ctypes.data, nx, ny, nz, nvol, m.ctypes.data, mdt | _lib.FIB_MASK_OUTPUTS_ZEROED,
                                      bval.ctypes.data, bvec.ctypes.data, v.ctypes.data, v.shape[0], fc.ctypes.data, fc.shape[0],
                                      C.byref(p), C.byref(o)))
    return CSD(sh, odf, peak, f, nit)


class CsdPlan(Plan):
    """The CSD tables (shell frames, kernel matrix, constraint rows, basis) and the tessellation's neighbour table resident on one GPU"""
    _destroy = "fib_csd_plan_destroy"

    def __init__(self, bval, bvec, response, odf_dirs: ODF = sphere_724, lmax: int = DEFAULTS["lmax"],
                 b0_thresh: float = DEFAULTS["b0_thresh"], shell=DEFAULTS["shell"], b_tol: float = DEFAULTS["b_tol"],
                 lam: float = DEFAULTS["lam"], tau: float = DEFAULTS["tau"], niter: int = DEFAULTS["niter"], device: int = 0):
        Plan.__init__(self, device)
        bval, bv = _host.table_args(bval, bvec)
        self.nvol, self.lmax, self.n, self.nreg = int(bval.shape[0]), int(lmax), ncoef(lmax), odf_dirs.nvert
        v, fc = _host.directions(odf_dirs, faces=True)
        p = _params(response, lmax, b0_thresh, shell, b_tol, lam, tau, niter)
        _lib.check(_lib.lib().fib_csd_plan_create(device, bval.ctypes.data, bv.ctypes.data, self.nvol, v.ctypes.data, v.shape[0],
                                                  fc.ctypes.data, fc.shape[0], C.byref(p), C.byref(self._h)))
        ns = C.c_int(0)
        _lib.check(_lib.lib().fib_csd_plan_tables(self._h, None, C.byref(ns), None, None, None, None))
        self.nshell = int(ns.value)

    def tables(self):
        """dict(frames [nshell], R [lmax / 2 + 1], X [nshell, n], B [nreg, n], Y [nreg, n]) as `csd_design` returns them"""
        frames = np.zeros(self.nshell, np.int32)
        R = np.zeros(self.lmax // 2 + 1, np.float32)
        X = np.zeros((self.nshell, self.n), np.float32, order="F")
        B = np.zeros((self.nreg, self.n), np.float32, order="F")
        Y = np.zeros((self.nreg, self.n), np.float32, order="F")
        _lib.check(_lib.lib().fib_csd_plan_tables(self._h, frames.ctypes.data, None, R.ctypes.data, X.ctypes.data, B.ctypes.data,
                                                  Y.ctypes.data))
        return dict(frames=frames, R=R, X=X, B=B, Y=Y)


def csd_rec_device(plan: CsdPlan, dwi, mask, out=None, stream=None):
    """dwi: float32 CUDA tensor [nvol, nvox] (planar, every frame of the scheme), mask: uint8 CUDA tensor [nvox].  Returns a dict of
    tensors: sh [n, nvox], odf [nreg, nvox], niter [nvox], peak [3][3, nvox], f [3][nvox] (`out`: such a dict to write into)."""
    import torch
    nvox = fit_args(plan, dwi, mask)
    with Launch(dwi, stream) as L:
        if out is None:
            out = dict(sh=L.empty((plan.n, nvox), torch.float32), odf=L.empty((plan.nreg, nvox), torch.float32),
                       niter=L.empty(nvox, torch.float32), peak=[L.empty((3, nvox), torch.float32) for _ in range(3)],
                       f=[L.empty(nvox, torch.float32) for _ in range(3)])
        else:
            for k, cnt in (("sh", plan.n * nvox), ("odf", plan.nreg * nvox), ("niter", nvox)):
                tensor(out[k], torch.float32, "out[%r]" % k, ref=plan, n=cnt)
            for k, cnt in (("peak", 3 * nvox), ("f", nvox)):
                if len(out[k]) != 3:
                    raise ArgError("out[%r] must be three tensors" % k)
                for t in out[k]:
                    tensor(t, torch.float32, "out[%r]" % k, ref=plan, n=cnt)
        o = _lib.CsdOut(out["sh"].data_ptr(), out["odf"].data_ptr(), out["niter"].data_ptr(),
                        _lib.P3(*[t.data_ptr() for t in out["peak"]]), _lib.P3(*[t.data_ptr() for t in out["f"]]))
        _lib.check(_lib.lib().fibd_csd_rec(plan._h, dwi.data_ptr(), mask.data_ptr(), nvox, C.byref(o), L.sp))
    return out

