"""dki_fit: diffusion kurtosis imaging (not in the reference; the definition is DESIGN.md §5).

`dki_fit(dwi, mask)` takes host `MRI`s and goes through the host-buffer C ABI (fib_dki_fit); `DkiPlan` + `dki_fit_device` are
the device-resident form on torch tensors (fibd_dki_fit).  `dki_design` builds the fit's tables on the host (no GPU needed)."""
import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _host, _lib
from ._dev import Launch, Plan, fit_args, tensor
from .dti import DTI_FIELDS
from .mri import MRI
from .odf import ODF, sphere_642

DKI_FIELDS = DTI_FIELDS + ("mk", "ak", "rk", "kt")
# the 15 independent elements of the kurtosis tensor, in the order of `kt`'s frames, and how often each occurs in the full tensor
KT_ORDER = ("xxxx", "yyyy", "zzzz", "xxxy", "xxxz", "xyyy", "yyyz", "xzzz", "yzzz", "xxyy", "xxzz", "yyzz", "xxyz", "xyyz", "xyzz")
KT_MULT = (1, 1, 1, 4, 4, 4, 4, 4, 4, 6, 6, 6, 12, 12, 12)
DEFAULTS = dict(min_signal=1e-4, min_diffusivity=1e-6, min_kurtosis=-3.0 / 7.0, max_kurtosis=10.0)


@dataclass
class DKI:
    """Container for outputs of a DKI fit: the ten `DTI` fields (of the kurtosis-corrected diffusion tensor), mean / axial / radial
    kurtosis and the kurtosis tensor W (15 frames in KT_ORDER)"""
    s0: MRI
    eigval1: MRI
    eigval2: MRI
    eigval3: MRI
    eigvec1: MRI
    eigvec2: MRI
    eigvec3: MRI
    rd: MRI
    md: MRI
    fa: MRI
    mk: MRI
    ak: MRI
    rk: MRI
    kt: MRI


def nframes(k):
    """frames of the output field `k` (of DKI_FIELDS)"""
    return 3 if "vec" in k else (15 if k == "kt" else 1)


_nframes = nframes      # the name tests/test_gpu_device_args.py, written before the rename, builds its rows with


def _params(min_signal, min_diffusivity, min_kurtosis, max_kurtosis):
    return _lib.DkiParams(min_signal, min_diffusivity, min_kurtosis, max_kurtosis)


def dki_design(bval, bvec):
    """The fit's tables, built on the host in float64 and rounded once: (A [nvol, 22] with b in ms/um^2, pA [22, nvol] scaled to
    mm^2/s and mm^4/s^2, rank).  A scheme whose design has a rank below 22 raises FibersError (code -1)."""
    bval, bv = _host.table_args(bval, bvec)
    nvol = int(bval.shape[0])
    A = np.zeros((nvol, 22), np.float32, order="F")
    pA = np.zeros((22, nvol), np.float32, order="F")
    rank = C.c_int(0)
    _lib.check(_lib.lib().fib_dki_design(bval.ctypes.data, bv.ctypes.data, nvol, A.ctypes.data, pA.ctypes.data, C.byref(rank)))
    return A, pA, int(rank.value)


def dki_fit(dwi: MRI, mask: MRI, odf_dirs: ODF = sphere_642, min_signal: float = DEFAULTS["min_signal"],
            min_diffusivity: float = DEFAULTS["min_diffusivity"], min_kurtosis: float = DEFAULTS["min_kurtosis"],
            max_kurtosis: float = DEFAULTS["max_kurtosis"], device: int = 0) -> DKI:
    """Fit the diffusion and kurtosis tensors to multi-shell DWIs and return a `DKI` structure.  mk is the mean of the apparent
    kurtosis over the half sphere of `odf_dirs`.  device: a GPU index, or _lib.DEVICE_ALL for the device set declared with
    fibers_jl_amd.init() (z-slab sharding, as dti_fit)."""
    bval, bvec = _host.check_tables(dwi)
    vol, m, mdt = _host.fit_inputs(dwi, mask)
    nx, ny, nz, nvol = vol.shape
    v = _host.directions(odf_dirs)
    outs = dict(zip(DKI_FIELDS, _host.fit_outputs(dwi, mask, [nframes(k) for k in DKI_FIELDS])))
    o = _lib.DkiOut(*[outs[k].vol.ctypes.data for k in DKI_FIELDS])
    p = _params(min_signal, min_diffusivity, min_kurtosis, max_kurtosis)
    _lib.check(_lib.lib().fib_dki_fit(device, vol.ctypes.data, nx, ny, nz, nvol, m.ctypes.data, mdt | _lib.FIB_MASK_OUTPUTS_ZEROED,
                                      bval.ctypes.data, bvec.ctypes.data, v.ctypes.data, v.shape[0], C.byref(p), C.byref(o)))
    return DKI(**outs)


class DkiPlan(Plan):
    """The DKI tables (pseudo-inverse columns, direction table of `odf_dirs`, limits) resident on one GPU"""
    _destroy = "fib_dki_plan_destroy"

    def __init__(self, bval, bvec, odf_dirs: ODF = sphere_642, min_signal: float = DEFAULTS["min_signal"],
                 min_diffusivity: float = DEFAULTS["min_diffusivity"], min_kurtosis: float = DEFAULTS["min_kurtosis"],
                 max_kurtosis: float = DEFAULTS["max_kurtosis"], device: int = 0):
        Plan.__init__(self, device)
        bval, bv = _host.table_args(bval, bvec)
        self.nvol = int(bval.shape[0])
        v = _host.directions(odf_dirs)
        self.ndir = odf_dirs.nvert
        p = _params(min_signal, min_diffusivity, min_kurtosis, max_kurtosis)
        _lib.check(_lib.lib().fib_dki_plan_create(device, bval.ctypes.data, bv.ctypes.data, self.nvol, v.ctypes.data, v.shape[0],
                                                  C.byref(p), C.byref(self._h)))

    def tables(self):
        """(A [nvol, 22], pA [22, nvol], dirs [ndir, 21])"""
        A = np.zeros((self.nvol, 22), np.float32, order="F")
        pA = np.zeros((22, self.nvol), np.float32, order="F")
        dirs = np.zeros((self.ndir, 21), np.float32)
        _lib.check(_lib.lib().fib_dki_plan_tables(self._h, A.ctypes.data, pA.ctypes.data, dirs.ctypes.data))
        return A, pA, dirs


def dki_fit_device(plan: DkiPlan, dwi, mask, out=None, stream=None, kt=True):
    """dwi: float32 CUDA tensor [nvol, nvox] (planar), mask: uint8 CUDA tensor [nvox].  Returns a dict of tensors: scalars [nvox],
    eigenvectors [3, nvox], kt [15, nvox].  `out` without a "kt" entry (or kt=False when the outputs are allocated here) skips
    the kurtosis tensor."""
    import torch
    nvox = fit_args(plan, dwi, mask)
    with Launch(dwi, stream) as L:
        if out is None:
            out = {k: L.empty((nframes(k), nvox) if nframes(k) > 1 else (nvox,), torch.float32) for k in DKI_FIELDS if kt or k != "kt"}
        else:
            for k in DKI_FIELDS:
                if k in out:
                    tensor(out[k], torch.float32, "out[%r]" % k, ref=plan, n=nframes(k) * nvox)
        o = _lib.DkiOut(*[out[k].data_ptr() if k in out else None for k in DKI_FIELDS])
        _lib.check(_lib.lib().fibd_dki_fit(plan._h, dwi.data_ptr(), mask.data_ptr(), nvox, C.byref(o), L.sp))
    return out
