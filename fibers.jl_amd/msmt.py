"""msmt_rec: multi-shell multi-tissue constrained spherical deconvolution, the white-matter fODF and the isotropic (GM, CSF) fractions
of a multi-shell series (not in the reference; the definition is include/fibers_hip.h "Multi-shell multi-tissue deconvolution" and
DESIGN.md §5).

`msmt_rec(dwi, mask, response)` takes host `MRI`s and goes through the host-buffer C ABI (fib_msmt_rec); `MsmtPlan` +
`msmt_rec_device` are the device-resident form on torch tensors (fibd_msmt_rec).  `msmt_shells` walks the b-values into shells,
`msmt_design` builds the tables on the host (no GPU needed); `msmt_response` estimates the three tissue responses from a tensor fit.
The result has `CSD`'s field names and feeds `prob_stream(m, odf_dirs)`, `stream(m.peak, f=m.f)` and `str_weights(tr, m)`."""
import ctypes as C
from dataclasses import dataclass
from typing import List

import numpy as np

from . import _host, _lib
from ._dev import ArgError, Launch, Plan, fit_args, tensor
from .csd import csd_response, ncoef
from .mri import MRI
from .nifti import msmt_write  # noqa: F401
from .odf import ODF, sphere_724

DEFAULTS = dict(lmax=8, b0_thresh=50.0, b_tol=0.05, lam=1.0, lam_iso=1.0, tau=0.0, niter=50)
MAX_SHELLS = 9       # shell 0 and eight above it


@dataclass
class MSMT:
    """Container for outputs of a multi-tissue deconvolution: the WM harmonic coefficients (n_wm frames), the isotropic fractions (one
    volume per isotropic tissue: GM, then CSF; not clamped), the WM fibre ODF on the half sphere of `odf_dirs`, its three largest peaks
    (unit vectors, 3 frames each) with their amplitudes, and the solves each voxel took"""
    sh: MRI
    iso: List[MRI]
    odf: MRI
    peak: List[MRI]
    f: List[MRI]
    niter: MRI


@dataclass
class MsmtResponse:
    """The tissue responses as tables: shells float64 [nshells] (the mean b of every shell, shell 0 = the b <= b0_thresh frames first),
    wm_R float32 [nshells, lmax / 2 + 1] (R_l of the white-matter response per shell), iso_r float32 [niso, nshells] (the mean signal of
    every isotropic tissue per shell: GM, then CSF)"""
    shells: np.ndarray
    wm_R: np.ndarray
    iso_r: np.ndarray


def _params(lmax, niso, b0_thresh, b_tol, lam, lam_iso, tau, niter):
    return _lib.MsmtParams(int(lmax), int(niso), float(b0_thresh), float(b_tol), float(lam), float(lam_iso), float(tau), int(niter))


def _response(response, lmax):
    """(wm_R float32 [nshells, lmax / 2 + 1] C-ordered, iso_r float32 [niso, nshells] C-ordered, nshells, niso)"""
    if int(lmax) not in (2, 4, 6, 8):
        raise ValueError("lmax must be 2, 4, 6 or 8")
    nl = int(lmax) // 2 + 1
    wm = np.ascontiguousarray(response.wm_R, np.float32)
    if wm.ndim != 2 or wm.shape[1] < nl:
        raise ValueError("response.wm_R must be [nshells, at least %d] for lmax %d, not %s" % (nl, lmax, wm.shape))
    wm = np.ascontiguousarray(wm[:, :nl])
    iso = np.ascontiguousarray(response.iso_r, np.float32).reshape(-1, wm.shape[0]) if np.size(response.iso_r) else np.zeros((0, wm.shape[0]), np.float32)
    if iso.shape[0] > 2:
        raise ValueError("at most two isotropic tissues, not %d" % iso.shape[0])
    return wm, iso, int(wm.shape[0]), int(iso.shape[0])


def msmt_shells(bval, b0_thresh: float = DEFAULTS["b0_thresh"], b_tol: float = DEFAULTS["b_tol"]):
    """The shell walk alone: (shell int32 [nvol], bbar float64 [nshells]); shell 0 holds the frames with b <= b0_thresh"""
    bval = np.ascontiguousarray(bval, np.float32).reshape(-1)
    nvol = int(bval.shape[0])
    bv = np.asfortranarray(np.ones((nvol, 3), np.float32))
    p = _params(DEFAULTS["lmax"], 0, b0_thresh, b_tol, 1.0, 1.0, 0.0, 1)
    shell, bbar, ns = np.zeros(nvol, np.int32), np.zeros(MAX_SHELLS, np.float64), C.c_int(0)
    _lib.check(_lib.lib().fib_msmt_design(bval.ctypes.data, bv.ctypes.data, nvol, None, 0, C.byref(p), None, None, 0, shell.ctypes.data,
                                          C.byref(ns), bbar.ctypes.data, None, None, None, None))
    return shell, bbar[:int(ns.value)].copy()


def msmt_wm_response(lambda_para, lambda_perp, s0, shells, lmax: int = DEFAULTS["lmax"]):
    """wm_R float32 [nshells, lmax / 2 + 1] of a prolate tensor at the mean b of every shell (fib_msmt_wm_response)"""
    bbar = np.ascontiguousarray(shells, np.float64).reshape(-1)
    R = np.zeros((bbar.shape[0], int(lmax) // 2 + 1), np.float32)
    _lib.check(_lib.lib().fib_msmt_wm_response(float(lambda_para), float(lambda_perp), float(s0), bbar.ctypes.data, bbar.shape[0], int(lmax),
                                               R.ctypes.data))
    return R


def msmt_response(dwi: MRI, dti, mask, wm_fa: float = 0.7, iso_fa: float = 0.2, gm_md=(0.6e-3, 1.1e-3), csf_md: float = 2.0e-3,
                  lmax: int = DEFAULTS["lmax"], b0_thresh: float = DEFAULTS["b0_thresh"], b_tol: float = DEFAULTS["b_tol"]) -> MsmtResponse:
    """The three tissue responses from a tensor fit, on the host in float64.  WM: `csd_response`'s prolate tensor (voxels with
    fa > wm_fa) evaluated at every shell.  GM: the per-shell mean signal of the voxels with fa < iso_fa and md inside gm_md; CSF: of
    those with fa < iso_fa and md > csf_md.  An empty class raises ValueError naming it.  A shell without frames (shell 0 of a series
    without b <= b0_thresh frames) holds 0 in iso_r: no row of the design reads it."""
    bval, _ = _host.check_tables(dwi, need_bvec=False)
    shell, bbar = msmt_shells(bval, b0_thresh, b_tol)
    lpar, lperp, s0 = csd_response(dti, mask, wm_fa)
    wm_R = msmt_wm_response(lpar, lperp, s0, bbar, lmax)
    m, _ = _host.mask(mask)

    def vol3(x):
        return x.vol[..., 0] if x.vol.ndim == 4 else x.vol
    fa, md = vol3(dti.fa), vol3(dti.md)
    low = (m != 0) & (fa < iso_fa)
    classes = (("GM", low & (md >= gm_md[0]) & (md <= gm_md[1]), "fa < %g and md in [%g, %g]" % (iso_fa, gm_md[0], gm_md[1])),
               ("CSF", low & (md > csf_md), "fa < %g and md > %g" % (iso_fa, csf_md)))
    iso_r = np.zeros((2, len(bbar)), np.float64)
    for t, (name, sel, rule) in enumerate(classes):
        if not sel.any():
            raise ValueError("no voxel inside the mask has %s: the %s response cannot be estimated" % (rule, name))
        s = np.asarray(dwi.vol)[sel].astype(np.float64)                       # [nsel, nvol]
        for k in range(len(bbar)):
            fr = shell == k
            iso_r[t, k] = s[:, fr].mean() if fr.any() else 0.0
    return MsmtResponse(bbar, wm_R, iso_r.astype(np.float32))


def msmt_design(bval, bvec, response: MsmtResponse, odf_dirs: ODF = sphere_724, lmax: int = DEFAULTS["lmax"],
                b0_thresh: float = DEFAULTS["b0_thresh"], b_tol: float = DEFAULTS["b_tol"], lam: float = DEFAULTS["lam"],
                lam_iso: float = DEFAULTS["lam_iso"]):
    """The reconstruction's tables, built on the host in float64 and rounded once: dict(shell int32 [nvol], bbar float64 [nshells],
    X [nvol, n], B [nreg + niso, n], Y [nreg, n], rank), n = n_wm + niso.  A series the unknowns cannot be determined from (fewer than n
    frames, a rank below n: two isotropic tissues on fewer than three shells) raises FibersError (code -1); more than 8 shells or 512
    frames -7."""
    bval, bv = _host.table_args(bval, bvec)
    wm, iso, nshells, niso = _response(response, lmax)
    nvol, n, nreg = int(bval.shape[0]), ncoef(lmax) + niso, odf_dirs.nvert
    v = _host.directions(odf_dirs)
    p = _params(lmax, niso, b0_thresh, b_tol, lam, lam_iso, DEFAULTS["tau"], DEFAULTS["niter"])
    shell, bbar = np.zeros(nvol, np.int32), np.zeros(MAX_SHELLS, np.float64)
    X = np.zeros((nvol, n), np.float32, order="F")
    B = np.zeros((nreg + niso, n), np.float32, order="F")
    Y = np.zeros((nreg, n), np.float32, order="F")
    ns, rank = C.c_int(0), C.c_int(0)
    _lib.check(_lib.lib().fib_msmt_design(bval.ctypes.data, bv.ctypes.data, nvol, v.ctypes.data, v.shape[0], C.byref(p), wm.ctypes.data,
                                          iso.ctypes.data if niso else None, nshells, shell.ctypes.data, C.byref(ns), bbar.ctypes.data,
                                          X.ctypes.data, B.ctypes.data, Y.ctypes.data, C.byref(rank)))
    return dict(shell=shell, bbar=bbar[:int(ns.value)].copy(), X=X, B=B, Y=Y, rank=int(rank.value))


def msmt_rec(dwi: MRI, mask: MRI, response: MsmtResponse, odf_dirs: ODF = sphere_724, lmax: int = DEFAULTS["lmax"],
             b0_thresh: float = DEFAULTS["b0_thresh"], b_tol: float = DEFAULTS["b_tol"], lam: float = DEFAULTS["lam"],
             lam_iso: float = DEFAULTS["lam_iso"], tau: float = DEFAULTS["tau"], niter: int = DEFAULTS["niter"], device: int = 0) -> MSMT:
    """Multi-shell multi-tissue deconvolution of every frame of `dwi` and return an `MSMT` structure.  response: an `MsmtResponse`,
    from `msmt_response` or built by hand; the rows of its iso_r are the isotropic tissues.  device: a GPU index, or _lib.DEVICE_ALL
    for the device set declared with fibers_jl_amd.init()."""
    bval, bvec = _host.check_tables(dwi)
    vol, m, mdt = _host.fit_inputs(dwi, mask)
    nx, ny, nz, nvol = vol.shape
    v, fc = _host.directions(odf_dirs, faces=True)
    wm, iso_r, nshells, niso = _response(response, lmax)
    p = _params(lmax, niso, b0_thresh, b_tol, lam, lam_iso, tau, niter)
    sh, *rest = _host.fit_outputs(dwi, mask, [ncoef(lmax)] + [1] * niso + [odf_dirs.nvert, 1, 3, 3, 3, 1, 1, 1])
    iso, (odf, nit), pf = rest[:niso], rest[niso:niso + 2], rest[niso + 2:]
    peak, f = pf[:3], pf[3:]
    o = _lib.MsmtOut(sh.vol.ctypes.data, (C.c_void_p * 2)(*[x.vol.ctypes.data for x in iso]), odf.vol.ctypes.data, nit.vol.ctypes.data,
                     _host.pointers(peak), _host.pointers(f))
    _lib.check(_lib.lib().fib_msmt_rec(device, vol.ctypes.data, nx, ny, nz, nvol, m.ctypes.data, mdt | _lib.FIB_MASK_OUTPUTS_ZEROED,
                                       bval.ctypes.data, bvec.ctypes.data, v.ctypes.data, v.shape[0], fc.ctypes.data, fc.shape[0],
                                       C.byref(p), wm.ctypes.data, iso_r.ctypes.data if niso else None, nshells, C.byref(o)))
    return MSMT(sh, iso, odf, peak, f, nit)


class MsmtPlan(Plan):
    """The deconvolution's tables (kernel matrix of every frame, constraint rows, basis) and the tessellation's neighbour table resident
    on one GPU"""
    _destroy = "fib_msmt_plan_destroy"

    def __init__(self, bval, bvec, response: MsmtResponse, odf_dirs: ODF = sphere_724, lmax: int = DEFAULTS["lmax"],
                 b0_thresh: float = DEFAULTS["b0_thresh"], b_tol: float = DEFAULTS["b_tol"], lam: float = DEFAULTS["lam"],
                 lam_iso: float = DEFAULTS["lam_iso"], tau: float = DEFAULTS["tau"], niter: int = DEFAULTS["niter"], device: int = 0):
        Plan.__init__(self, device)
        bval, bv = _host.table_args(bval, bvec)
        wm, iso, nshells, niso = _response(response, lmax)
        self.nvol, self.lmax, self.niso, self.nwm, self.nreg = int(bval.shape[0]), int(lmax), niso, ncoef(lmax), odf_dirs.nvert
        self.n, self.nshells = self.nwm + niso, nshells
        v, fc = _host.directions(odf_dirs, faces=True)
        p = _params(lmax, niso, b0_thresh, b_tol, lam, lam_iso, tau, niter)
        _lib.check(_lib.lib().fib_msmt_plan_create(device, bval.ctypes.data, bv.ctypes.data, self.nvol, v.ctypes.data, v.shape[0],
                                                   fc.ctypes.data, fc.shape[0], C.byref(p), wm.ctypes.data,
                                                   iso.ctypes.data if niso else None, nshells, C.byref(self._h)))

    def tables(self):
        """dict(shell [nvol], bbar [nshells], X [nvol, n], B [nreg + niso, n], Y [nreg, n]) as `msmt_design` returns them"""
        shell, bbar = np.zeros(self.nvol, np.int32), np.zeros(self.nshells, np.float64)
        X = np.zeros((self.nvol, self.n), np.float32, order="F")
        B = np.zeros((self.nreg + self.niso, self.n), np.float32, order="F")
        Y = np.zeros((self.nreg, self.n), np.float32, order="F")
        _lib.check(_lib.lib().fib_msmt_plan_tables(self._h, shell.ctypes.data, None, bbar.ctypes.data, X.ctypes.data, B.ctypes.data,
                                                   Y.ctypes.data))
        return dict(shell=shell, bbar=bbar, X=X, B=B, Y=Y)


def msmt_rec_device(plan: MsmtPlan, dwi, mask, out=None, stream=None):
    """dwi: float32 CUDA tensor [nvol, nvox] (planar), mask: uint8 CUDA tensor [nvox].  Returns a dict of tensors: sh [n_wm, nvox],
    iso [niso][nvox], odf [nreg, nvox], niter [nvox], peak [3][3, nvox], f [3][nvox] (`out`: such a dict to write into)."""
    import torch
    nvox = fit_args(plan, dwi, mask)
    with Launch(dwi, stream) as L:
        if out is None:
            out = dict(sh=L.empty((plan.nwm, nvox), torch.float32), iso=[L.empty(nvox, torch.float32) for _ in range(plan.niso)],
                       odf=L.empty((plan.nreg, nvox), torch.float32), niter=L.empty(nvox, torch.float32),
                       peak=[L.empty((3, nvox), torch.float32) for _ in range(3)], f=[L.empty(nvox, torch.float32) for _ in range(3)])
        else:
            for k, cnt in (("sh", plan.nwm * nvox), ("odf", plan.nreg * nvox), ("niter", nvox)):
                tensor(out[k], torch.float32, "out[%r]" % k, ref=plan, n=cnt)
            for k, cnt, want in (("iso", nvox, plan.niso), ("peak", 3 * nvox, 3), ("f", nvox, 3)):
                if len(out[k]) != want:
                    raise ArgError("out[%r] must be %d tensors" % (k, want))
                for t in out[k]:
                    tensor(t, torch.float32, "out[%r]" % k, ref=plan, n=cnt)
        o = _lib.MsmtOut(out["sh"].data_ptr(), (C.c_void_p * 2)(*[t.data_ptr() for t in out["iso"]]), out["odf"].data_ptr(),
                         out["niter"].data_ptr(), _lib.P3(*[t.data_ptr() for t in out["peak"]]), _lib.P3(*[t.data_ptr() for t in out["f"]]))
        _lib.check(_lib.lib().fibd_msmt_rec(plan._h, dwi.data_ptr(), mask.data_ptr(), nvox, C.byref(o), L.sp))
    return out
