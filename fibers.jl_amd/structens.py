"""Structure tensor (structens.jl) behind the C ABI: `st_eigen` and `st_recon`.

`st_eigen` loops `eigen(Symmetric(S, :L))` over the voxels of six Float32 volumes; one HIP kernel does it with the 3x3 solver
of the tensor fit (csrc/sym3_eigen.inc).  `st_recon` builds those six volumes from a scalar volume -- Gaussian smoothing,
Scharr gradients, their products, Gaussian smoothing of the products, all imfilter(..., "reflect") -- and decomposes them, in
two HIP kernels (csrc/structens.hip)."""
import ctypes as C

import numpy as np

from . import _host, _lib
from ._dev import ArgError, Launch, tensor, work as _work


def st_eigen(Sxx, Sxy, Sxz, Syy, Syz, Szz, device=0):
    """st_eigen(Sxx, Sxy, Sxz, Syy, Syz, Szz) -> (eigvec [nx,ny,nz,3,3], eigval [nx,ny,nz,3]), ascending eigenvalues,
    eigvec[..., :, j] the j-th eigenvector (structens.jl:13-37).  Float32 3-D arrays of one shape."""
    vols = [np.asfortranarray(v, dtype=np.float32) for v in (Sxx, Sxy, Sxz, Syy, Syz, Szz)]
    shape = vols[0].shape
    if len(shape) != 3 or any(v.shape != shape for v in vols):
        raise ValueError("st_eigen takes six 3-D arrays of one shape")
    nvox = int(np.prod(shape))
    eigvec = np.empty(shape + (3, 3), np.float32, order="F")
    eigval = np.empty(shape + (3,), np.float32, order="F")
    ptrs = _host.pointers(vols)
    _lib.check(_lib.lib().fib_st_eigen(int(device), ptrs, nvox, eigvec.ctypes.data, eigval.ctypes.data))
    return eigvec, eigval


def st_eigen_device(S, stream=None):
    """Device tier: S = six float32 CUDA tensors [nvox] on one device; returns (eigvec [9, nvox], eigval [3, nvox]) with
    eigvec[i + 3 j] = component i of eigenvector j.  `stream`: _dev.Launch."""
    import torch
    if len(S) != 6:
        raise ArgError("six volumes expected")
    nvox = tensor(S[0], torch.float32, "S[0]").numel()
    for c in range(1, 6):
        tensor(S[c], torch.float32, "S[%d]" % c, ref=S[0], n=nvox)
    ptrs = (C.c_void_p * 6)(*[t.data_ptr() for t in S])
    with Launch(S[0], stream) as L:
        eigvec, eigval = L.empty((9, nvox), torch.float32), L.empty((3, nvox), torch.float32)
        _lib.check(_lib.lib().fibd_st_eigen(ptrs, nvox, eigvec.data_ptr(), eigval.data_ptr(), L.sp))
    return eigvec, eigval


def st_recon(vol, sigma, rho, device=0):
    """st_recon(vol, sigma, rho) -> (eigvec [nx,ny,nz,3,3], eigval [nx,ny,nz,3]) (structens.jl:40-88): the structure tensor
    of a 3-D volume (or a one-frame MRI), smoothed by Gaussians of sigma (the image) and rho (the tensor), each skipped when
    <= 0; ascending eigenvalues, eigvec[..., :, j] the j-th eigenvector.  sigma, rho <= 8."""
    from .mri import MRI
    if isinstance(vol, MRI):
        if vol.nframes != 1:
            raise ValueError("st_recon takes a one-frame MRI")
        vol = vol.vol[..., 0]
    v = np.asfortranarray(vol, dtype=np.float32)
    if v.ndim != 3:
        raise ValueError("st_recon takes a 3-D volume")
    nx, ny, nz = v.shape
    eigvec = np.empty(v.shape + (3, 3), np.float32, order="F")
    eigval = np.empty(v.shape + (3,), np.float32, order="F")
    _lib.check(_lib.lib().fib_st_recon(int(device), v.ctypes.data, nx, ny, nz, float(sigma), float(rho),
                                       eigvec.ctypes.data, eigval.ctypes.data))
    return eigvec, eigval


def st_recon_halo(sigma, rho):
    """planes of input a z-range of st_recon outputs needs on each side (fib_st_recon_halo)"""
    h = C.c_int()
    _lib.check(_lib.lib().fib_st_recon_halo(float(sigma), float(rho), C.byref(h)))
    return h.value


def st_recon_work_size(nx, ny, nz, sigma, rho):
    """bytes of device scratch st_recon_device needs for nz output planes (fibd_st_recon_work_size)"""
    b = C.c_uint64()
    _lib.check(_lib.lib().fibd_st_recon_work_size(int(nx), int(ny), int(nz), float(sigma), float(rho), C.byref(b)))
    return int(b.value)


def st_recon_device(vol, shape, sigma, rho, stream=None, S_out=False, zin0=0, z0=0, z1=None):
    """Device tier of st_recon: vol = a contiguous float32 CUDA tensor holding planes [zin0, zin0 + vol.numel() / (nx*ny)) of
    the nx*ny*nz volume `shape` (x fastest).  Returns (eigvec [9, n], eigval [3, n]) for output planes [z0, z1) (default: all),
    st_eigen_device's layout, plus S [6, n] (Sxx Sxy Sxz Syy Syz Szz, the smoothed tensor) when S_out.  vol must hold the
    planes st_recon_halo(sigma, rho) beyond [z0, z1) on each side (as far as the volume goes).
    `stream`: a torch stream, a raw hipStream_t handle, or None (the current stream).  The kernels are enqueued on it and vol must
    be ready there.  The outputs and the gradient workspace are allocated by _dev.Launch: on a torch stream the caching allocator
    hands the workspace out again only to work ordered after these kernels; with a raw handle the call waits for the stream before
    it lets the workspace go."""
    import torch
    nx, ny, nz = (int(n) for n in shape)
    if nx <= 0 or ny <= 0:
        raise ArgError("shape %s: nx and ny must be positive" % (tuple(shape),))
    tensor(vol, torch.float32, "vol (whole %d x %d planes)" % (nx, ny), unit=nx * ny)
    z1 = nz if z1 is None else int(z1)
    nzin, n = vol.numel() // (nx * ny), max(nx * ny * (z1 - int(z0)), 0)
    with Launch(vol, stream) as L:
        eigvec, eigval = L.empty((9, n), torch.float32), L.empty((3, n), torch.float32)
        S = L.empty((6, n), torch.float32) if S_out else None
        work, wb = _work(L, None, st_recon_work_size, "st_recon_work_size", nx, ny, max(z1 - int(z0), 1), sigma, rho)
        sp = (C.c_void_p * 6)(*[S[c].data_ptr() for c in range(6)]) if S_out else None
        _lib.check(_lib.lib().fibd_st_recon(vol.data_ptr(), nx, ny, nz, int(zin0), nzin, int(z0), z1, float(sigma), float(rho),
                                            eigvec.data_ptr(), eigval.data_ptr(), sp, work.data_ptr(), wb, L.sp))
    return (eigvec, eigval, S) if S_out else (eigvec, eigval)
