"""Structure tensor (structens.jl) behind the C ABI: `st_eigen` and `st_recon`.

`st_eigen` loops `eigen(Symmetric(S, :L))` over the voxels of six Float32 volumes; one HIP kernel does it with the 3x3 solver
of the tensor fit (csrc/sym3_eigen.inc).  `st_recon` builds those six volumes from a scalar volume -- Gaussian smoothing,
Scharr gradients, their products, Gaussian smoothing of the products, all imfilter(..., "reflect") -- and decomposes them, in
two HIP kernels (csrc/structens.hip)."""
import contextlib
import ctypes as C

import numpy as np

from . import _lib
from .dti import _stream_ptr, _sync


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
    ptrs = (C.c_void_p * 6)(*[v.ctypes.data for v in vols])
    _lib.check(_lib.lib().fib_st_eigen(int(device), ptrs, nvox, eigvec.ctypes.data, eigval.ctypes.data))
    return eigvec, eigval


def st_eigen_device(S, stream=None):
    """Device tier: S = six float32 CUDA tensors [nvox]; returns (eigvec [9, nvox], eigval [3, nvox]) with
    eigvec[i + 3 j] = component i of eigenvector j."""
    import torch
    if len(S) != 6:
        raise ValueError("six volumes expected")
    for t in S:
        if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
            raise ValueError("contiguous float32 CUDA tensors expected")
    nvox = S[0].numel()
    eigvec = torch.empty((9, nvox), dtype=torch.float32, device=S[0].device)
    eigval = torch.empty((3, nvox), dtype=torch.float32, device=S[0].device)
    ptrs = (C.c_void_p * 6)(*[t.data_ptr() for t in S])
    sp = None if stream is None else C.c_void_p(stream.cuda_stream)
    with torch.cuda.device(S[0].device):
        _lib.check(_lib.lib().fibd_st_eigen(ptrs, nvox, eigvec.data_ptr(), eigval.data_ptr(), sp))
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


def st_recon_device(vol, shape, sigma, rho, stream=None, S_out=False, zin0=0, z0=0, z1=None):
    """Device tier of st_recon: vol = a contiguous float32 CUDA tensor holding planes [zin0, zin0 + vol.numel() / (nx*ny)) of
    the nx*ny*nz volume `shape` (x fastest).  Returns (eigvec [9, n], eigval [3, n]) for output planes [z0, z1) (default: all),
    st_eigen_device's layout, plus S [6, n] (Sxx Sxy Sxz Syy Syz Szz, the smoothed tensor) when S_out.  vol must hold the
    planes st_recon_halo(sigma, rho) beyond [z0, z1) on each side (as far as the volume goes).
    `stream`: a torch stream, a raw hipStream_t handle, or None (the current stream).  The kernels are enqueued on it and vol must
    be ready there.  With a torch stream the outputs and the gradient workspace are allocated on that stream, so the caching
    allocator hands the workspace out again only to work ordered after these kernels; with a raw handle the call waits for the
    stream before it lets the workspace go."""
    import torch
    nx, ny, nz = (int(n) for n in shape)
    if not (vol.is_cuda and vol.dtype == torch.float32 and vol.is_contiguous()):
        raise ValueError("a contiguous float32 CUDA tensor expected")
    if nx <= 0 or ny <= 0 or vol.numel() % (nx * ny):
        raise ValueError("vol does not hold whole %d x %d planes" % (nx, ny))
    z1 = nz if z1 is None else int(z1)
    nzin, n = vol.numel() // (nx * ny), nx * ny * (z1 - int(z0))
    dev = vol.device
    L = _lib.lib()
    nbytes = C.c_uint64()
    _lib.check(L.fibd_st_recon_work_size(nx, ny, max(z1 - int(z0), 1), float(sigma), float(rho), C.byref(nbytes)))
    on_torch_stream = isinstance(stream, torch.cuda.Stream)
    with torch.cuda.device(dev), (torch.cuda.stream(stream) if on_torch_stream else contextlib.nullcontext()):
        eigvec = torch.empty((9, max(n, 0)), dtype=torch.float32, device=dev)
        eigval = torch.empty((3, max(n, 0)), dtype=torch.float32, device=dev)
        S = torch.empty((6, max(n, 0)), dtype=torch.float32, device=dev) if S_out else None
        work = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
        sp = (C.c_void_p * 6)(*[S[c].data_ptr() for c in range(6)]) if S_out else None
        _lib.check(L.fibd_st_recon(vol.data_ptr(), nx, ny, nz, int(zin0), nzin, int(z0), z1, float(sigma), float(rho),
                                   eigvec.data_ptr(), eigval.data_ptr(), sp, work.data_ptr(), nbytes.value, _stream_ptr(stream)))
    if stream is not None and not on_torch_stream:     # a raw handle: the allocator cannot order the workspace's reuse after it
        _sync(stream)
    return (eigvec, eigval, S) if S_out else (eigvec, eigval)
