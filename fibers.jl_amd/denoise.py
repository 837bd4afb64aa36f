"""dwi_denoise: Marchenko-Pastur PCA denoising of a DWI series (not in the reference; the definition is include/fibers_hip.h
"Marchenko-Pastur PCA denoising" and DESIGN.md §5).

`dwi_denoise(dwi, mask)` takes host `MRI`s and goes through the host-buffer C ABI (fib_dwi_denoise, z-slabs); `dwi_denoise_device` is
the device-resident form on torch tensors (fibd_dwi_denoise), for the whole volume or a z-slab of it.  The result's `dwi` keeps the
gradient table and goes straight into `dti_fit`, `dki_fit`, `csd_rec`."""
import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _host, _lib
from ._dev import ArgError, Launch, tensor, work as _work
from .mri import MRI

ESTIMATORS = {"exp1": 1, "exp2": 2}     # FIB_DENOISE_EXP1 / FIB_DENOISE_EXP2


@dataclass
class Denoised:
    """Container for outputs of the denoising: the denoised series (with the input's bval / bvec), the noise level sigma and the number
    of signal components kept per voxel (rank; -1 with sigma = NaN where the eigen-solver did not converge)"""
    dwi: MRI
    sigma: MRI
    rank: MRI


def _estimator(estimator):
    if estimator not in ESTIMATORS:
        raise ValueError("estimator must be 'exp1' or 'exp2', not %r" % (estimator,))
    return ESTIMATORS[estimator]


def dwi_denoise_check(shape, nframes, patch=5, estimator="exp2"):
    """the library's refusals for a volume of `shape` with `nframes` frames (fib_dwi_denoise_check; no device needed): raises
    FibersError as `dwi_denoise` would"""
    nx, ny, nz = (int(n) for n in shape)
    _lib.check(_lib.lib().fib_dwi_denoise_check(nx, ny, nz, int(nframes), int(patch), _estimator(estimator)))


def dwi_denoise(dwi, mask=None, patch=5, estimator="exp2", device=0) -> Denoised:
    """Denoise `dwi` (an MRI [nx,ny,nz,N]) inside `mask` (an MRI or array [nx,ny,nz], None: everywhere) with P^3 patches, P = `patch`
    in (3, 5, 7), and return a `Denoised` structure.  estimator: "exp1" (Veraart 2016) or "exp2" (Cordero-Grande 2019)."""
    est = _estimator(estimator)
    src = dwi if isinstance(dwi, MRI) else MRI(np.asarray(dwi))
    vol = _host.volume(src, dtype=np.float32, series=True)
    nx, ny, nz, nvol = vol.shape
    if mask is None:
        m = np.ones((nx, ny, nz), np.uint8, order="F")
    else:
        m, _ = _host.mask(mask, (nx, ny, nz), "!= 0", frame0=False, refuse="mask of shape %s for a volume of %s")
    out = MRI(np.zeros(vol.shape, np.float32, order="F"), bval=src.bval, bvec=src.bvec, volres=src.volres, vox2ras=src.vox2ras.copy(), tr=src.tr)
    sigma, rank = MRI.like(src, 1), MRI.like(src, 1)
    _lib.check(_lib.lib().fib_dwi_denoise(int(device), vol.ctypes.data, nx, ny, nz, nvol, m.ctypes.data, int(patch), est,
                                          out.vol.ctypes.data, sigma.vol.ctypes.data, rank.vol.ctypes.data))
    return Denoised(out, sigma, rank)


def dwi_denoise_work_size(nx, ny, nz, nframes, patch=5):
    """bytes of device workspace dwi_denoise_device needs for nz output planes (fibd_dwi_denoise_work_size)"""
    b = C.c_uint64()
    _lib.check(_lib.lib().fibd_dwi_denoise_work_size(int(nx), int(ny), int(nz), int(nframes), int(patch), C.byref(b)))
    return int(b.value)


def dwi_denoise_device(dwi, mask, shape, patch=5, estimator="exp2", zin0=0, z0=0, z1=None, out=None, work=None, stream=None):
    """Device tier: dwi = a contiguous float32 CUDA tensor [N, nx*ny*nzin] holding planes [zin0, zin0 + nzin) of every frame of the
    nx*ny*nz volume `shape` (x fastest); mask = uint8 (or bool) [n] over the output planes [z0, z1) (default: all), n = nx*ny*(z1-z0).
    Returns dict(dwi [N, n], sigma [n], rank [n]) (`out`: such a dict to write into).  The patches are clamped against the whole
    volume, so dwi must hold the planes from the patch of plane z0 to the patch of plane z1 - 1 (at most patch - 1 beyond [z0, z1)).
    `work`: a caller's workspace of at least dwi_denoise_work_size(nx, ny, z1 - z0, N, patch) bytes (None: scratch of the launch);
    `stream`: _dev.Launch."""
    import torch
    est = _estimator(estimator)
    nx, ny, nz = (int(n) for n in shape)
    if nx <= 0 or ny <= 0 or nz <= 0:
        raise ArgError("shape %s: nx, ny and nz must be positive" % (tuple(shape),))
    plane = nx * ny
    tensor(dwi, torch.float32, "dwi", shape=(None, None))
    nvol = int(dwi.shape[0])
    tensor(dwi, torch.float32, "dwi (whole %d x %d planes of every frame)" % (nx, ny), unit=max(nvol, 1) * plane)
    nzin = dwi.shape[1] // plane
    z0, z1 = int(z0), nz if z1 is None else int(z1)
    if not 0 <= z0 < z1 <= nz:
        raise ArgError("output planes [%d, %d) outside [0, %d)" % (z0, z1, nz))
    n = plane * (z1 - z0)
    mask = tensor(mask, torch.uint8, "mask", ref=dwi, n=n, bool_ok=True)
    with Launch(dwi, stream) as L:
        if out is None:
            out = dict(dwi=L.empty((nvol, n), torch.float32), sigma=L.empty(n, torch.float32), rank=L.empty(n, torch.float32))
        else:
            for k, cnt in (("dwi", nvol * n), ("sigma", n), ("rank", n)):
                tensor(out[k], torch.float32, "out[%r]" % k, ref=dwi, n=cnt)
        w, wb = _work(L, work, dwi_denoise_work_size, "dwi_denoise_work_size", nx, ny, z1 - z0, nvol, patch)
        _lib.check(_lib.lib().fibd_dwi_denoise(dwi.data_ptr(), nx, ny, nz, int(zin0), nzin, z0, z1, nvol, int(patch), est, mask.data_ptr(),
                                               out["dwi"].data_ptr(), out["sigma"].data_ptr(), out["rank"].data_ptr(), w.data_ptr(), wb, L.sp))
    return out
