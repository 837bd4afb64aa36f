"""dti_fit / adc_fit host mirror (reference: dti.jl:7 exports `DTI, adc_fit, dti_fit, dti_write`).

`dti_fit(dwi, mask)` and `adc_fit(dwi, mask)` take host `MRI`s and go through the host-buffer C ABI
(fib_dti_fit / fib_adc_fit).  `DtiPlan` + `dti_fit_device` / `adc_fit_device` are the device-resident
form on torch tensors (fibd_*), used for multi-GPU sharding and benchmarking."""
import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _host, _lib
from ._dev import Launch, Plan, fit_args, stream_ptr as _stream_ptr, tensor
from .mri import MRI

DTI_FIELDS = ("s0", "eigval1", "eigval2", "eigval3", "eigvec1", "eigvec2", "eigvec3", "rd", "md", "fa")


@dataclass
class DTI:
    """Container for outputs of a DTI fit (dti.jl:11-22)"""
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


def dti_fit(dwi: MRI, mask: MRI, device: int = 0) -> DTI:
    """Fit tensors to DWIs and return a `DTI` structure (dti.jl:221).  device: a GPU index, or _lib.DEVICE_ALL for the
    device set declared with fibers_jl_amd.init() (z-slab sharding, dti.jl:258)."""
    bval, bvec = _host.check_tables(dwi)
    vol, m, mdt = _host.fit_inputs(dwi, mask)
    nx, ny, nz, nvol = vol.shape
    outs = dict(zip(DTI_FIELDS, _host.fit_outputs(dwi, mask, [3 if "vec" in k else 1 for k in DTI_FIELDS])))
    o = _lib.DtiOut(*[outs[k].vol.ctypes.data for k in DTI_FIELDS])
    _lib.check(_lib.lib().fib_dti_fit(device, vol.ctypes.data, nx, ny, nz, nvol, m.ctypes.data, mdt | _lib.FIB_MASK_OUTPUTS_ZEROED,
                                      bval.ctypes.data, bvec.ctypes.data, C.byref(o)))
    return DTI(**outs)


def adc_fit(dwi: MRI, mask: MRI, device: int = 0):
    """Fit the apparent diffusion coefficient; returns (adc, s0) (dti.jl:164)."""
    bval, _ = _host.check_tables(dwi, need_bvec=False)
    vol, m, mdt = _host.fit_inputs(dwi, mask)
    nx, ny, nz, nvol = vol.shape
    adc, s0 = _host.fit_outputs(dwi, mask, [1, 1])
    _lib.check(_lib.lib().fib_adc_fit(device, vol.ctypes.data, nx, ny, nz, nvol, m.ctypes.data, mdt | _lib.FIB_MASK_OUTPUTS_ZEROED,
                                      bval.ctypes.data, adc.vol.ctypes.data, s0.vol.ctypes.data))
    return adc, s0


# ---------------------------------------------------------------------------------------------
# device-resident form (torch tensors are plumbing: device memory + streams)
# ---------------------------------------------------------------------------------------------
class DtiPlan(Plan):
    """DTIwork / ADCwork (dti.jl:39-155) resident on one GPU.  bvec=None builds the ADC plan."""
    _destroy = "fib_dti_plan_destroy"

    def __init__(self, bval, bvec=None, device: int = 0):
        Plan.__init__(self, device)
        bval, bv = _host.table_args(bval, bvec, need_bvec=bvec is not None)
        self.nvol = int(bval.shape[0])
        _lib.check(_lib.lib().fib_dti_plan_create(device, bval.ctypes.data, None if bv is None else bv.ctypes.data,
                                                  self.nvol, C.byref(self._h)))
        self.np = 7 if bv is not None else 2

    def tables(self):
        A = np.zeros((self.nvol, self.np), np.float32, order="F")
        pA = np.zeros((self.np, self.nvol), np.float32, order="F")
        n = C.c_int(0)
        _lib.check(_lib.lib().fib_dti_plan_tables(self._h, A.ctypes.data, pA.ctypes.data, C.byref(n)))
        return A, pA

    def last_partial_count(self, stream=None):
        c = C.c_int64(0)
        _lib.check(_lib.lib().fibd_dti_last_partial_count(self._h, _stream_ptr(stream), C.byref(c)))
        return int(c.value)


def dti_fit_device(plan: DtiPlan, dwi, mask, out=None, stream=None):
    """dwi: float32 CUDA tensor [nvol, nvox] (planar: frame slowest == MRI.vol memory order);
    mask: uint8 CUDA tensor [nvox].  Returns dict of tensors: scalars [nvox], eigvecs [3, nvox] (`out`: such a dict to write into)."""
    import torch
    nvox = fit_args(plan, dwi, mask)
    with Launch(dwi, stream) as L:
        if out is None:
            out = {k: L.empty((3, nvox) if "vec" in k else (nvox,), torch.float32) for k in DTI_FIELDS}
        else:
            for k in DTI_FIELDS:
                tensor(out[k], torch.float32, "out[%r]" % k, ref=plan, n=(3 if "vec" in k else 1) * nvox)
        o = _lib.DtiOut(*[out[k].data_ptr() for k in DTI_FIELDS])
        _lib.check(_lib.lib().fibd_dti_fit(plan._h, dwi.data_ptr(), mask.data_ptr(), nvox, C.byref(o), L.sp))
    return out


def adc_fit_device(plan: DtiPlan, dwi, mask, stream=None):
    import torch
    nvox = fit_args(plan, dwi, mask)
    with Launch(dwi, stream) as L:
        adc, s0 = L.empty(nvox, torch.float32), L.empty(nvox, torch.float32)
        _lib.check(_lib.lib().fibd_adc_fit(plan._h, dwi.data_ptr(), mask.data_ptr(), nvox, adc.data_ptr(), s0.data_ptr(), L.sp))
    return adc, s0
