"""Probabilistic tractography from the ODF (`prob_stream`): at every step the direction is drawn from the ODF of the voxel ahead,
restricted to a cone around the direction of travel.  Not in the reference; the definition (the quantised weight table, the cone, the
counter-based draws, the line) is the "Probabilistic tracking" section of include/fibers_hip.h.  All compute is in csrc/probtrack.hip;
there is no NumPy path here.

Host tier: `MRI` / `GQI` / `DSI` in, `Tract` out, through fib_prob_stream.  Device tier: torch tensors in and out, through
fibd_prob_table / fibd_prob_run on `stream`; the result is the dict of stream_device_run and every `str_*_device` entry takes it.  The two
device-tier functions are reached as `fibers_jl_amd.probtrack.prob_table_device` / `.prob_stream_device`: the package's top level lists the
`*_device` names that tests/test_gpu_device_args.py has a row for, and these two have their own checks in tests/test_gpu_probtrack.py."""
import ctypes as C
from typing import Optional

import numpy as np

from . import _host, _lib
from ._dev import ArgError, Launch, Plan, tensor, work as _work
from .mri import MRI
from .odf import ODF, sphere_642
from .stream import StreamBuffers, buffers_on, cosd32, make_sublist
from .tract import Tract


def prob_row_pitch(nvert: int) -> int:
    """elements per row of the weight table: 64 * ceil(nvert / 64)"""
    p = _lib.lib().fib_prob_row_pitch(int(nvert))
    if p <= 0:
        raise ValueError("1 to 512 directions are supported, not %d" % nvert)
    return p


def prob_work_size(nlines: int) -> int:
    """bytes of device scratch prob_stream_device needs for `nlines` = seeds x sub-voxel offsets"""
    n = C.c_uint64(0)
    _lib.check(_lib.lib().fibd_prob_work_size(int(nlines), C.byref(n)))
    return int(n.value)


class ProbPlan(Plan):
    """The directions U (the first half of `odf_dirs`' vertices, or a float32 [nvert, 3] array) and the cone's bit tables for
    `ang_thresh` degrees (below 90), resident on one GPU.  cosang_thresh, if given, is taken as it is instead of cosd(ang_thresh)."""
    _destroy = "fib_prob_plan_destroy"

    def __init__(self, odf_dirs=sphere_642, ang_thresh: float = 45, device: int = 0, cosang_thresh: Optional[float] = None):
        Plan.__init__(self, int(device))
        U = _host.directions(odf_dirs, half=True)
        self.nvert, self.pitch = U.shape[0], prob_row_pitch(U.shape[0])
        self.cosang_thresh = float(cosd32(ang_thresh) if cosang_thresh is None else np.float32(cosang_thresh))
        _lib.check(_lib.lib().fib_prob_plan_create(self.device, U.ctypes.data, self.nvert, self.cosang_thresh, C.byref(self._h)))


def prob_table_device(odf, mask=None, subtract_min: bool = True, pmf_thresh: float = 0.1, out=None, stream=None):
    """The weight table of an ODF volume.  odf: float32 CUDA [nvert, nvox] (what odf_rec_device returns); mask: uint8 / bool [nvox] or
    None; out: uint16 CUDA [nvox, pitch] to write into, or None.  Returns the table, uint16 [nvox, prob_row_pitch(nvert)]."""
    import torch
    tensor(odf, torch.float32, "odf [nvert, nvox]", shape=(None, None))
    nvert, nvox = int(odf.shape[0]), int(odf.shape[1])
    pitch = prob_row_pitch(nvert)
    if mask is not None:
        mask = tensor(mask, torch.uint8, "mask", ref=odf, n=nvox, bool_ok=True)
    if out is not None:
        tensor(out, torch.uint16, "out", ref=odf, shape=(nvox, pitch))
    with Launch(odf, stream) as L:
        table = L.empty((nvox, pitch), torch.uint16) if out is None else out
        _lib.check(_lib.lib().fibd_prob_table(odf.data_ptr(), None if mask is None else mask.data_ptr(), nvox, nvert, int(bool(subtract_min)),
                                              float(np.float32(pmf_thresh)), table.data_ptr(), L.sp))
    return table


def prob_stream_device(plan: ProbPlan, table, shape, seeds, sublist, len_min=3, len_max=None, step_size=0.5, rng_seed=0,
                       buffers: StreamBuffers = None, work=None, stream=None):
    """Trace on the GPU (fibd_prob_run).  table: uint16 CUDA [nvox, plan.pitch] from prob_table_device; seeds: int64 CUDA tensor of
    0-based column-major voxel indices; sublist: float32 CUDA [nsub, 3].  Results go into `buffers` (grown and the call repeated when
    they are too small).  Returns dict(npts, seed_index, xyz, buffers) as stream_device_run does -- views of the buffers, valid until
    the next call with them -- plus all_counts int32 [nseed * nsub, 2]: {nfwd, nbwd} of every line, a view of the scratch."""
    import torch
    nx, ny, nz = (int(v) for v in shape)
    tensor(table, torch.uint16, "table", ref=plan, shape=(nx * ny * nz, plan.pitch))
    tensor(seeds, torch.int64, "seeds", ref=plan)
    tensor(sublist, torch.float32, "sublist", ref=plan, shape=(None, 3))
    if sublist.shape[0] < 1:
        raise ArgError("sublist must hold at least one offset")
    nl_max = int(seeds.numel()) * int(sublist.shape[0])
    len_max = max(nx, ny, nz) if len_max is None else int(len_max)
    nl, npnt = C.c_int64(0), C.c_int64(0)
    with Launch(table, stream) as L:
        w, wb = _work(L, work, prob_work_size, "fibd_prob_work_size(nseed * nsub)", nl_max)
        if buffers is None:
            buffers = StreamBuffers(table.device)
        buffers_on(buffers, table)
        if buffers.npts is None or buffers.npts.numel() == 0:
            buffers.reserve(nl_max, 32 * nl_max)                    # a first guess; the call below says what is needed
        for attempt in range(2):
            rc = _lib.lib().fibd_prob_run(plan._h, nx, ny, nz, int(len_min), len_max, float(np.float32(step_size)), table.data_ptr(),
                                          seeds.data_ptr(), seeds.numel(), sublist.data_ptr(), sublist.shape[0], int(rng_seed) & (2 ** 64 - 1),
                                          buffers.npts.data_ptr(), buffers.seed_index.data_ptr(), buffers.npts.numel(), buffers.xyz.data_ptr(),
                                          buffers.xyz.shape[0], C.byref(nl), C.byref(npnt), w.data_ptr(), wb, L.sp)
            if rc == _lib.FIB_ERR_CAPACITY and attempt == 0:
                buffers.reserve(int(nl.value), int(npnt.value))
                continue
            _lib.check(rc)
            break
        counts = w.reshape(-1).view(torch.int32)[: 2 * nl_max].view(nl_max, 2)
    return dict(npts=buffers.npts[: nl.value], seed_index=buffers.seed_index[: nl.value], xyz=buffers.xyz[: npnt.value], buffers=buffers,
                all_counts=counts)


def prob_stream(odf, odf_dirs: ODF = sphere_642, *, mask: Optional[MRI] = None, seed: Optional[MRI] = None, nsub: int = 3, sublist=None,
                len_min: int = 3, len_max: Optional[int] = None, ang_thresh: float = 45, step_size: float = 0.5, pmf_thresh: float = 0.1,
                subtract_min: bool = True, rng_seed: int = 0, rng=None, device: int = 0) -> Tract:
    """Probabilistic streamline tractography from an ODF volume.  odf: an `MRI` with odf_dirs.nvert frames, or a `GQI` / `DSI` result
    (its `.odf`).  Seeds (the `seed` volume, else the mask, else every voxel; column-major order), `sublist` / `nsub` and the default
    of len_max follow `stream`; the line order and the points' 1-based voxel coordinates too.  ang_thresh (degrees, below 90) is the
    half-angle of the cone the next direction is drawn from; amplitudes below pmf_thresh of a voxel's maximum (after subtract_min)
    are never drawn.  The same arguments and rng_seed give the same bytes."""
    o = getattr(odf, "odf", odf)
    vol = _host.volume(o, dtype=np.float32, series=True)
    U = _host.directions(odf_dirs, half=True)
    if vol.ndim != 4 or vol.shape[3] != U.shape[0]:
        raise ValueError("odf must be [nx, ny, nz, %d] (one frame per direction), not %s" % (U.shape[0], vol.shape))
    shape = vol.shape[:3]

    def bytes_of(m, what):
        return None if m is None else _host.mask(m, shape, "> 0", refuse=what + " shape %s does not match the ODF volume %s")[0]

    m8, s8 = bytes_of(mask, "mask"), bytes_of(seed, "seed")
    sub = make_sublist(nsub, rng) if sublist is None else np.ascontiguousarray(sublist, np.float32).reshape(-1, 3)
    out = _lib.TractOut()
    L = _lib.lib()
    _lib.check(L.fib_prob_stream(int(device), shape[0], shape[1], shape[2], vol.ctypes.data, U.shape[0], U.ctypes.data,
                                 None if m8 is None else m8.ctypes.data, None if s8 is None else s8.ctypes.data, sub.ctypes.data, sub.shape[0],
                                 int(len_min), int(len_max if len_max is not None else max(shape)), float(cosd32(ang_thresh)),
                                 float(np.float32(step_size)), float(np.float32(pmf_thresh)), int(bool(subtract_min)),
                                 int(rng_seed) & (2 ** 64 - 1), C.byref(out)))
    npts, sidx, xyz, _ = _host.tract_arrays(out)
    ref = next((x for x in (mask, o) if isinstance(x, MRI)), None)
    return Tract(xyz=xyz, npts=npts, seed_index=sidx, volsize=shape,
                 volres=tuple(ref.volres) if ref is not None else (1.0, 1.0, 1.0),
                 vox2ras=ref.vox2ras.copy() if ref is not None else np.eye(4, dtype=np.float32), sublist=sub)
