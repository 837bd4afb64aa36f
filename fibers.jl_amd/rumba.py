"""rumba_rec host mirror (reference: rusd.jl:7 `RUMBASD, rumba_rec, rumba_write`) -- SURVEY.md row N4."""
import ctypes as C
from dataclasses import dataclass
from typing import List, Optional

import numpy as np

from . import _host, _lib
from ._dev import ArgError, Launch, Plan, tensor
from .mri import MRI
from .odf import ODF, sphere_724


@dataclass
class RUMBASD:
    """Container for outputs of a RUMBA-SD fit (rusd.jl:11-20)"""
    fodf: MRI
    fgm: MRI
    fcsf: MRI
    peak: List[MRI]
    gfa: MRI
    var: MRI
    snr_mean: float
    snr_std: float


def _coil_mode(coil_combine: str) -> int:
    if coil_combine == "SoS-GRAPPA":
        return 1
    if coil_combine != "SMF-SENSE":
        raise ValueError("Unknown coil combine mode " + coil_combine)          # rusd.jl:433
    return 0


def rumba_rec(dwi: MRI, mask: MRI, odf_dirs: ODF = sphere_724, niter: int = 600, lam_para: float = 1.7e-3,
              lam_perp: float = 0.2e-3, lam_csf: float = 3.0e-3, lam_gm: float = 0.8e-4, ncoils: int = 1,
              coil_combine: str = "SMF-SENSE", ipat_factor: int = 1, use_tv: bool = True, device: int = 0) -> RUMBASD:
    """Robust and unbiased model-based spherical deconvolution (rusd.jl:419)."""
    bval, bvec = _host.check_tables(dwi)
    sos = _coil_mode(coil_combine)
    if ipat_factor < 1:
        raise ValueError("iPAT factor must be a positive integer")             # rusd.jl:437
    vol, m, mdt = _host.fit_inputs(dwi, mask)
    nx, ny, nz, nvol = vol.shape
    v = _host.directions(odf_dirs)
    fodf, *rest = _host.fit_outputs(dwi, mask, [odf_dirs.nvert] + [1] * 4 + [3] * 5)
    sc, peak = rest[:4], rest[4:]
    out = _lib.RumbaOut(fodf.vol.ctypes.data, *[s.vol.ctypes.data for s in sc], _host.pointers(peak))
    sm, ss = C.c_float(0), C.c_float(0)
    _lib.check(_lib.lib().fib_rumba_rec(device, vol.ctypes.data, nx, ny, nz, nvol, m.ctypes.data, mdt,
                                        bval.ctypes.data, bvec.ctypes.data, v.ctypes.data, v.shape[0], int(niter),
                                        float(lam_para), float(lam_perp), float(lam_csf), float(lam_gm), int(ncoils), sos,
                                        int(ipat_factor), 1 if use_tv else 0, C.byref(out), C.byref(sm), C.byref(ss)))
    return RUMBASD(fodf, sc[0], sc[1], peak, sc[2], sc[3], float(sm.value), float(ss.value))


class RumbaPlan(Plan):
    """kernel + contraction plans of rumba_rec resident on one GPU"""
    _destroy = "fib_rumba_plan_destroy"

    def __init__(self, bval, bvec, odf_dirs: ODF = sphere_724, lam_para=1.7e-3, lam_perp=0.2e-3, lam_csf=3.0e-3,
                 lam_gm=0.8e-4, device: int = 0):
        Plan.__init__(self, device)
        bval, bvec = _host.table_args(bval, bvec)
        v = _host.directions(odf_dirs)
        self.nvert, self.nvol = odf_dirs.nvert, int(bval.shape[0])
        _lib.check(_lib.lib().fib_rumba_plan_create(device, bval.ctypes.data, bvec.ctypes.data, self.nvol, v.ctypes.data,
                                                    v.shape[0], float(lam_para), float(lam_perp), float(lam_csf),
                                                    float(lam_gm), C.byref(self._h)))

    def kernel(self):
        nd, nc = C.c_int(0), C.c_int(0)
        L = _lib.lib()
        _lib.check(L.fib_rumba_plan_kernel(self._h, None, C.byref(nd), C.byref(nc)))
        K = np.zeros((nd.value, nc.value), np.float32, order="F")
        _lib.check(L.fib_rumba_plan_kernel(self._h, K.ctypes.data, None, None))
        return K


def rumba_rec_device(plan: RumbaPlan, dwi, mask, shape, niter=600, ncoils=1, coil_combine="SMF-SENSE", ipat_factor=1,
                     use_tv=True, stream=None, out=None):
    """dwi: float32 CUDA [nvol, nvox]; mask uint8 [nvox]; shape = (nx, ny, nz).  Returns dict(fodf [nvert,nvox], fgm, fcsf,
    gfa, var [nvox], peak [5][3,nvox], snr_mean, snr_std).  out: such a dict of tensors to write into (every element is
    written: zeros outside the mask)."""
    import torch
    nx, ny, nz = (int(v) for v in shape)
    nvox = nx * ny * nz
    tensor(dwi, torch.float32, "dwi", ref=plan, shape=(plan.nvol, nvox))
    tensor(mask, torch.uint8, "mask", ref=plan, n=nvox)
    want = dict(fodf=(plan.nvert, nvox), fgm=(nvox,), fcsf=(nvox,), gfa=(nvox,), var=(nvox,))
    with Launch(dwi, stream) as L:
        if out is None:
            out = {k: L.empty(shp, torch.float32) for k, shp in want.items()}
            out["peak"] = [L.empty((3, nvox), torch.float32) for _ in range(5)]
        else:
            for k, shp in want.items():
                tensor(out[k], torch.float32, "out['%s']" % k, ref=plan, shape=shp)
            if len(out["peak"]) != 5:
                raise ArgError("out['peak'] must be five [3, %d] tensors" % nvox)
            for t in out["peak"]:
                tensor(t, torch.float32, "out['peak']", ref=plan, shape=(3, nvox))
        ro = _lib.RumbaOut(out["fodf"].data_ptr(), out["fgm"].data_ptr(), out["fcsf"].data_ptr(), out["gfa"].data_ptr(),
                           out["var"].data_ptr(), (C.c_void_p * 5)(*[t.data_ptr() for t in out["peak"]]))
        sm, ss = C.c_float(0), C.c_float(0)
        _lib.check(_lib.lib().fibd_rumba_rec(plan._h, dwi.data_ptr(), mask.data_ptr(), nx, ny, nz, int(niter), int(ncoils),
                                             _coil_mode(coil_combine), int(ipat_factor), 1 if use_tv else 0, C.byref(ro),
                                             C.byref(sm), C.byref(ss), L.sp))
    out["snr_mean"], out["snr_std"] = float(sm.value), float(ss.value)
    return out
