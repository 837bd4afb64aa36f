"""mri_nlreg and warp_jacobian: a displacement field estimated on the GPU (single-contrast, multi-resolution, additive demons) and the
Jacobian map that checks it.  The estimator of what `mri_warp` / `str_warp` apply; not in the reference.  The definitions (geometry,
normalised values, moving sample, fixed gradient, force, cost, regularisation, the step between levels, the determinant) are the
"Non-linear registration" section of include/fibers_hip.h, restated in tests/nlreg_ref.py.  All compute is in csrc/nlreg.hip; there
is no NumPy path here: what this module computes itself are float64 matrices rounded once (`jacobian_matrix`, `mri_warp`'s three).

Host tier: `mri_nlreg(moving, fixed)` and `warp_jacobian(warp)` take `MRI`s / a `Warp` and go through fib_mri_nlreg /
fib_warp_jacobian on one device.  Device tier: `nlreg_step_device`, `warp_smooth_device`, `warp_upsample_device`, `warp_unpack_device`,
`warp_jacobian_device`, `mri_nlreg_device` on torch tensors."""
import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _host, _lib
from ._dev import ArgError, Launch, tensor, work as _work
from .mri import MRI
from .register import _as_mri, _i3, _shape, reg_levels
from .warp import Warp, _inv, _f64, _packed, volume_matrices
from .xform import Xform, round32, xfm_inv


@dataclass
class NonlinearRegistration:
    """Container for outputs of mri_nlreg: `warp` (a Warp on the fixed grid: phi takes fixed RAS to moving RAS), `post` (the Xform, or
    None, to hand to mri_warp / str_warp with it), `warped` (the moving volume on the fixed grid: bit-equal to mri_warp(warp, moving,
    outref=fixed, post=post)), `cost` (float64 [levels, max niter]: the mean squared difference of the normalised values BEFORE each
    iteration's update, row 0 the coarsest level, NaN where no iteration ran) and `count` (int64, the voxels behind each cost)"""
    warp: Warp
    post: Xform
    warped: MRI
    cost: np.ndarray
    count: np.ndarray


# ---- the library's host code ------------------------------------------------------------------------------------------------------
def _f9(m):
    return (C.c_float * 9)(*[float(v) for v in np.ascontiguousarray(m, np.float32).reshape(-1)])


def _post16(post):
    """None, an Xform (its ras2ras) or a [4, 4] matrix (fixed RAS -> moving RAS) -> the `const float *` of the ABI"""
    if post is None:
        return None
    return _host.m16(post.ras2ras if isinstance(post, Xform) else post)


def nlreg_level(fixed_vox2ras, moving_vox2ras, post=None, level=0, step=1.0):
    """what a level needs (fib_nlreg_level): (to_ras float32 [4, 4], from_ras float32 [4, 4], T float32 [3, 3], kappa float32)"""
    A, B, T, k = (C.c_float * 16)(), (C.c_float * 16)(), (C.c_float * 9)(), C.c_float()
    _lib.check(_lib.lib().fib_nlreg_level(_host.m16(fixed_vox2ras), _host.m16(moving_vox2ras), _post16(post), int(level), float(step), A, B, T,
                                          C.byref(k)))
    return (np.array(A, np.float32).reshape(4, 4), np.array(B, np.float32).reshape(4, 4), np.array(T, np.float32).reshape(3, 3),
            np.float32(k.value))


def jacobian_matrix(field_vox2ras):
    """linv of warp_jacobian: float32(inv(L)) with L the float64 3 x 3 linear part of the field's float32 vox2ras"""
    return round32(_inv(_f64(field_vox2ras)[:3, :3], "the field's vox2ras"))


def niter_list(niter, levels):
    """`niter` as one count per level, coarsest first: an int is repeated; a sequence must hold `levels` counts"""
    if isinstance(niter, (int, np.integer)):
        n = [int(niter)] * levels
    else:
        n = [int(v) for v in niter]
        if len(n) != levels:
            raise ValueError("niter holds %d counts for a pyramid of %d levels (one per level, coarsest first)" % (len(n), levels))
    if min(n) < 0:
        raise ValueError("niter must not be negative")
    return n


# ---- device tier ------------------------------------------------------------------------------------------------------------------
def _out_field(L, out, ref, nvox, what="out [nx*ny*nz, 4]"):
    import torch
    if out is None:
        return L.empty((nvox, 4), torch.float32)
    tensor(out, torch.float32, what, ref=ref, n=4 * nvox)
    if out.data_ptr() % 16:
        raise ArgError("out must be 16-byte aligned")
    return out


def nlreg_step_work_size(shape):
    """bytes of device workspace nlreg_step_device needs (fibd_nlreg_step_work_size)"""
    b = C.c_uint64()
    nx, ny, nz = _shape(shape)
    _lib.check(_lib.lib().fibd_nlreg_step_work_size(nx, ny, nz, C.byref(b)))
    return int(b.value)


def nlreg_step_device(fixed, fixed_shape, moving, moving_shape, norm, to_ras, from_ras, T, kappa, packed, out=None, cost=None, work=None,
                      stream=None):
    """fibd_nlreg_step: one demons iteration.  fixed float32 [nvox_f] and moving float32 [nvox_m] (the level volumes, x fastest), norm =
    (lo_fixed, s_fixed, lo_moving, s_moving), the level's matrices and kappa (nlreg_level), packed the current field [nvox_f, 4] ->
    (the updated packed field, cost: an int64 tensor [2] that holds { float64 ssd; uint64 count }, read with `cost_pair`).  `out`,
    `cost`, `work`: buffers to use (work: at least nlreg_step_work_size(fixed_shape) bytes).  The call does not wait for the kernels."""
    import torch
    nxf, nyf, nzf = _packed(packed, fixed_shape)
    nxm, nym, nzm = _shape(moving_shape)
    nvf = nxf * nyf * nzf
    tensor(fixed, torch.float32, "fixed", ref=packed, n=nvf)
    tensor(moving, torch.float32, "moving", ref=packed, n=nxm * nym * nzm)
    nrm = (C.c_float * 4)(*[float(v) for v in np.asarray(norm, np.float32).reshape(4)])
    with Launch(packed, stream) as L:
        out = _out_field(L, out, packed, nvf)
        if cost is None:
            cost = L.empty((2,), torch.int64)
        else:
            tensor(cost, torch.int64, "cost [2]", ref=packed, n=2)
        w, wb = _work(L, work, nlreg_step_work_size, "nlreg_step_work_size", (nxf, nyf, nzf))
        _lib.check(_lib.lib().fibd_nlreg_step(fixed.data_ptr(), nxf, nyf, nzf, moving.data_ptr(), nxm, nym, nzm, nrm, _host.m16(to_ras),
                                              _host.m16(from_ras), _f9(T), float(kappa), packed.data_ptr(), out.data_ptr(), cost.data_ptr(),
                                              w.data_ptr(), wb, L.sp))
    return out, cost


def cost_pair(cost):
    """a cost tensor on the host: (ssd float64, count int); waits for the tensor"""
    raw = cost.cpu().numpy().reshape(2)
    return float(raw[:1].view(np.float64)[0]), int(raw[1:].view(np.uint64)[0])


def warp_smooth_device(packed, shape, sigma=1.0, out=None, work=None, stream=None):
    """fibd_warp_smooth: the packed field [nvox, 4] smoothed by a separable Gaussian of `sigma` voxels (0: a copy; at most 4), x pass, then
    y, then z.  `out`: a packed field to write into; `work`: 16 * nvox bytes, 16-byte aligned.  The call does not wait for the kernels."""
    nx, ny, nz = _packed(packed, shape)
    nvox = nx * ny * nz
    with Launch(packed, stream) as L:
        out = _out_field(L, out, packed, nvox)
        w, wb = _work(L, work, lambda n: 16 * n, "16 * nvox", nvox)
        if w.data_ptr() % 16:
            raise ArgError("work must be 16-byte aligned")
        _lib.check(_lib.lib().fibd_warp_smooth(packed.data_ptr(), nx, ny, nz, float(sigma), out.data_ptr(), w.data_ptr(), wb, L.sp))
    return out


def warp_upsample_device(coarse, coarse_shape, shape, out=None, stream=None):
    """fibd_warp_upsample: the start of a finer level.  coarse: the packed field of `coarse_shape` -> the packed field of `shape`, fine
    voxel y taking S(0.5 y - 0.25) of the coarse one.  The call does not wait for the kernel."""
    cx, cy, cz = _packed(coarse, coarse_shape)
    nx, ny, nz = _shape(shape)
    with Launch(coarse, stream) as L:
        out = _out_field(L, out, coarse, nx * ny * nz)
        _lib.check(_lib.lib().fibd_warp_upsample(coarse.data_ptr(), cx, cy, cz, out.data_ptr(), nx, ny, nz, L.sp))
    return out


def warp_unpack_device(packed, shape, out=None, stream=None):
    """fibd_warp_unpack: the packed field [nvox, 4] -> the planar field float32 [3, nvox], the inverse of warp_pack_device.  The call
    does not wait for the kernel."""
    import torch
    nx, ny, nz = _packed(packed, shape)
    nvox = nx * ny * nz
    with Launch(packed, stream) as L:
        out = L.empty((3, nvox), torch.float32) if out is None else tensor(out, torch.float32, "out [3, nx*ny*nz]", ref=packed, n=3 * nvox)
        _lib.check(_lib.lib().fibd_warp_unpack(packed.data_ptr(), nx, ny, nz, out.data_ptr(), L.sp))
    return out


def warp_jacobian_device(packed, shape, linv, out=None, stream=None):
    """fibd_warp_jacobian: det(I + dd/dx) at every voxel of the packed field, float32 [nvox]; linv float32 [3, 3] (jacobian_matrix).
    The call does not wait for the kernel."""
    import torch
    nx, ny, nz = _packed(packed, shape)
    nvox = nx * ny * nz
    with Launch(packed, stream) as L:
        out = L.empty((nvox,), torch.float32) if out is None else tensor(out, torch.float32, "out [nx*ny*nz]", ref=packed, n=nvox)
        _lib.check(_lib.lib().fibd_warp_jacobian(packed.data_ptr(), nx, ny, nz, _f9(linv), out.data_ptr(), L.sp))
    return out


def nlreg_work_size(fixed_shape, moving_shape, niter):
    """bytes of device workspace mri_nlreg_device needs (fibd_nlreg_work_size); niter: one count per level, coarsest first"""
    n = np.ascontiguousarray(niter, np.int32).reshape(-1)
    b = C.c_uint64()
    _lib.check(_lib.lib().fibd_nlreg_work_size(_i3(fixed_shape), _i3(moving_shape), int(n.size), n.ctypes.data, C.byref(b)))
    return int(b.value)


def mri_nlreg_device(moving, moving_shape, moving_vox2ras, fixed, fixed_shape, fixed_vox2ras, post=None, levels=None, niter=30, sigma=1.0,
                     step=1.0, out=None, work=None, stream=None):
    """Device tier of mri_nlreg (fibd_nlreg_run): moving float32 [nvox_m] against fixed float32 [nvox_f] (x fastest) with their sizes and
    vox2ras; post: None, an Xform or a [4, 4] matrix, fixed RAS -> moving RAS; step in mm.  Returns (the packed level-0 field [nvox_f, 4],
    cost float64 [levels, max niter], count int64 [levels, max niter]).  Waits once for the ranges and once per level for its costs."""
    import torch
    fs, ms = _shape(fixed_shape), _shape(moving_shape)
    nvf = int(np.prod(fs))
    tensor(fixed, torch.float32, "fixed", n=nvf)
    tensor(moving, torch.float32, "moving", ref=fixed, n=int(np.prod(ms)))
    nl = reg_levels(fs, ms) if not levels else int(levels)
    try:
        n = np.array(niter_list(niter, nl), np.int32)
    except ValueError as e:
        raise ArgError(str(e)) from None
    width = max(1, int(n.max()))
    cost, count = np.empty((nl, width), np.float64), np.empty((nl, width), np.int64)
    with Launch(fixed, stream) as L:
        out = _out_field(L, out, fixed, nvf)
        w, wb = _work(L, work, nlreg_work_size, "nlreg_work_size", fs, ms, n)
        if w.data_ptr() % 16:
            raise ArgError("work must be 16-byte aligned")
        _lib.check(_lib.lib().fibd_nlreg_run(fixed.data_ptr(), _i3(fs), _host.m16(fixed_vox2ras), moving.data_ptr(), _i3(ms),
                                             _host.m16(moving_vox2ras), _post16(post), nl, n.ctypes.data, float(sigma), float(step), out.data_ptr(),
                                             cost.ctypes.data, count.ctypes.data, w.data_ptr(), wb, L.sp))
    return out, cost, count


# ---- host tier --------------------------------------------------------------------------------------------------------------------
def mri_nlreg(moving, fixed, init: Xform = None, levels=None, niter=30, sigma=1.0, step=None, frame=None, device=0) -> NonlinearRegistration:
    """Estimate the displacement field that takes `moving` onto `fixed` (MRIs of one contrast): multi-resolution additive demons with a
    fixed number of iterations per level.  `init`: the Xform of mri_register(moving, fixed) (in = moving, out = fixed), the affine the
    field refines; `levels`: pyramid levels (None: mri_register's rule); `niter`: an int, or one count per level from the coarsest to the
    finest; `sigma`: the Gaussian regularisation in level voxels (0: none; at most 4); `step`: the force's length scale in mm (None: the
    smallest fixed voxel size); `frame`: the frame of a moving series (None: the only frame; a series of several needs it named, one frame is registered).

    The result's `warp` lives on the fixed grid; mri_warp(r.warp, moving, outref=fixed, post=r.post) lands the moving volume on the fixed
    grid and str_warp(r.warp, lines_in_fixed_space, outref=moving, post=r.post) takes fixed-space lines into moving space.
    warp_jacobian(r.warp) is the check on the estimate: a value <= 0 marks a fold."""
    moving, fixed = _as_mri(moving), _as_mri(fixed)
    vol = _host.volume(moving, dtype=np.float32, series=True)
    if vol.shape[3] > 1 and frame is None:
        raise ValueError("moving holds %d frames: name the one to register with frame=" % vol.shape[3])
    f = 0 if frame is None else int(frame)
    if not 0 <= f < vol.shape[3]:
        raise ValueError("frame %d of a moving series of %d frames" % (f, vol.shape[3]))
    mov = np.asfortranarray(vol[..., f])
    fix = _host.volume(fixed, dtype=np.float32, frame0=True)
    fs, ms = fix.shape, mov.shape
    nl = reg_levels(fs, ms) if not levels else int(levels)
    n = np.array(niter_list(niter, nl), np.int32)
    step = float(np.float32(min(float(v) for v in fixed.volres))) if step is None else float(step)
    post = None if init is None else xfm_inv(init)
    one = MRI(mov, volres=moving.volres, vox2ras=np.array(moving.vox2ras, np.float32))
    mats = np.ascontiguousarray(np.stack(volume_matrices(fixed.vox2ras, fixed.vox2ras, moving.vox2ras, None, post)), np.float32)
    width = max(1, int(n.max()))
    cost, count = np.empty((nl, width), np.float64), np.empty((nl, width), np.int64)
    disp = np.empty(tuple(fs) + (3,), np.float32, order="F")
    warped = np.empty(tuple(fs) + (1,), np.float32, order="F")
    _lib.check(_lib.lib().fib_mri_nlreg(int(device), mov.ctypes.data, _i3(ms), _host.m16(moving.vox2ras), fix.ctypes.data, _i3(fs),
                                        _host.m16(fixed.vox2ras), _post16(post), nl, n.ctypes.data, float(sigma), step, disp.ctypes.data,
                                        cost.ctypes.data, count.ctypes.data, mats.ctypes.data, warped.ctypes.data))
    geo = dict(volres=tuple(float(v) for v in fixed.volres), vox2ras=np.array(fixed.vox2ras, np.float32))
    return NonlinearRegistration(Warp(MRI(disp, **geo)), post, _host.resampled(warped, one, fixed.volres, fixed.vox2ras), cost, count)


def warp_jacobian(warp: Warp, device: int = 0) -> MRI:
    """det(I + dd/dx) of a Warp at every voxel of its grid (an MRI of one float32 frame): the local volume change of phi.  A value
    <= 0 marks a fold; the estimate-side companion of warp_invert's err."""
    nx, ny, nz = _host.dims(warp.volsize)
    out = np.empty((nx, ny, nz, 1), np.float32, order="F")
    disp = warp._planar()
    _lib.check(_lib.lib().fib_warp_jacobian(int(device), disp.ctypes.data, nx, ny, nz, _f9(jacobian_matrix(warp.vox2ras)), out.ctypes.data))
    return MRI(out, volres=tuple(float(v) for v in warp.field.volres), vox2ras=np.array(warp.vox2ras, np.float32))
