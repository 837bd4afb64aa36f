"""NumPy Float32 restatement of the trilinear tracker's integrators (fib_stream_params.interp = 1, 2, 3; NOT in the reference), written
from the definition in include/fibers_hip.h.  D(p, r) is oracle_np.trilinear_direction; the line loop is oracle_np.stream_line's with
the rule for the tentative position `nxt` swapped in:

    euler: nxt = pos + vec * h
    rk2:   k2 = D(pos + vec * half, vec) ;  nxt = pos + k2 * h
    rk4:   k2 = D(pos + vec * half, vec) ;  k3 = D(pos + k2 * half, k2) ;  k4 = D(pos + k3 * h, k3) ;
           s = ((vec + 2 * k2) + 2 * k3) + k4 ;  nxt = pos + s * sixth

h = step, half = step * 0.5, sixth = step / 6 (one division), every operation a Float32 operation rounded on its own.  A stage without
a direction ends the pass and the current point is not emitted.  Test infrastructure only."""
import os
import sys

import numpy as np

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _ROOT not in sys.path:
    sys.path.insert(0, _ROOT)
from oracle.oracle_np import _pick_by_angle, norm32, trilinear_direction  # noqa: E402

f32 = np.float32
INTEGRATORS = ("euler", "rk2", "rk4")


def _D(p, r, ovecs):
    """D(p, r): None when p is not finite or the blend is zero / not finite"""
    p = np.asarray(p, f32)
    with np.errstate(invalid="ignore"):
        if not np.isfinite(p).all():
            return None
    return trilinear_direction(p, np.asarray(r, f32), ovecs)


def _axpy(pos, k, a):
    """pos + k * a, component-wise: the product rounded to Float32, then the sum"""
    return (pos + (k * a).astype(f32)).astype(f32)


def next_position(pos, vec, ovecs, step, integrator):
    """the tentative position of a step from the state (pos, vec); None when a stage finds no direction"""
    h = f32(step)
    if integrator == "euler":
        return _axpy(pos, vec, h)
    half = f32(h * f32(0.5))
    k2 = _D(_axpy(pos, vec, half), vec, ovecs)
    if k2 is None:
        return None
    if integrator == "rk2":
        return _axpy(pos, k2, h)
    if integrator != "rk4":
        raise ValueError("integrator must be one of %s" % (INTEGRATORS,))
    sixth = f32(h / f32(6))
    k3 = _D(_axpy(pos, k2, half), k2, ovecs)
    if k3 is None:
        return None
    k4 = _D(_axpy(pos, k3, h), k3, ovecs)
    if k4 is None:
        return None
    two = f32(2)
    s = (((vec + (two * k2).astype(f32)).astype(f32) + (two * k3).astype(f32)).astype(f32) + k4).astype(f32)
    return _axpy(pos, s, sixth)


def stream_line(seed, sub, ovecs, mask, step=0.5, cosang_thresh=None, smooth=0.2, len_max=None, integrator="euler"):
    """oracle_np.stream_line(..., interp="trilinear") with the integrator's rule for `nxt`.  ovecs [3, nvec, nx, ny, nz] Float32 (masked
    vectors zeroed), mask [nx, ny, nz], seed 1-based (ix, iy, iz); returns [npts, 3] in the reference's point order."""
    shape = ovecs.shape[2:]
    step, smooth = f32(step), f32(smooth)
    cosang_thresh = f32(np.cos(np.deg2rad(45.0))) if cosang_thresh is None else f32(cosang_thresh)
    len_max = max(shape) if len_max is None else len_max
    line = []
    npts = 0
    ivec = 0
    for fwd in (1, -1):
        pos = (np.asarray(seed, f32) + np.asarray(sub, f32)).astype(f32)
        vec = (ovecs[:, ivec, seed[0] - 1, seed[1] - 1, seed[2] - 1] * f32(fwd)).astype(f32)
        while True:
            nxt = next_position(pos, vec, ovecs, step, integrator)
            if nxt is None:                                                     # a stage without a direction: the pass ends, pos is not emitted
                break
            with np.errstate(invalid="ignore"):
                if not np.isfinite(nxt).all():
                    break
            vox = np.rint(nxt).astype(np.int64)
            if not all(1 <= vox[d] <= shape[d] for d in range(3)):
                break
            if not mask[vox[0] - 1, vox[1] - 1, vox[2] - 1]:
                break
            k, ck = _pick_by_angle(vec, ovecs[:, :, vox[0] - 1, vox[1] - 1, vox[2] - 1])   # the nearest voxel's pick must exist; it sets ivec
            with np.errstate(invalid="ignore"):
                if not np.isfinite(ck):
                    break
            ivec = k
            vnext = _D(nxt, vec, ovecs)
            if vnext is None:
                break
            if fwd == 1:
                line.insert(0, pos.copy())
            else:
                line.append(pos.copy())
            npts += 1
            d = (vec[0] * vnext[0] + vec[1] * vnext[1]) + vec[2] * vnext[2]
            if d < cosang_thresh:
                break
            if npts > len_max:
                break
            if smooth != 0:
                vnext = smooth * vec + (f32(1) - smooth) * vnext
                vnext = vnext / norm32(vnext)
            pos, vec = nxt, vnext.astype(f32)
    return np.array(line, f32).reshape(-1, 3)


def stream(ovecs, mask, seeds, sublist, len_min=3, **kw):
    """every (seed, offset) line in the reference's order: dict(npts, seed_index, xyz) of the lines with at least len_min points.
    seeds: 1-based voxels [nseed, 3] in findall order."""
    npts, sidx, xyz = [], [], []
    nsub = len(sublist)
    for si, seed in enumerate(seeds):
        for k in range(nsub):
            line = stream_line([int(v) for v in seed], sublist[k], ovecs, mask, **kw)
            if line.shape[0] >= len_min:
                npts.append(line.shape[0]); sidx.append(si * nsub + k); xyz.append(line)
    return dict(npts=np.array(npts, np.int32), seed_index=np.array(sidx, np.int64),
                xyz=np.concatenate(xyz, 0) if xyz else np.zeros((0, 3), f32))


# ---- the circular-field known answer (tests/test_stream_rk_ref.py, tests/test_gpu_stream_rk.py) -------------------------------------
CIRCLE_SHAPE = (48, 48, 3)
CIRCLE_C = 24.5
CIRCLE_SEEDS = [(40, 24, 2), (36, 25, 2), (33, 24, 2), (24, 38, 2)]           # 1-based voxels, radii 8.5 - 15.5 voxels
CIRCLE_SUB = np.array([[0.1, -0.2, 0.0]], f32)


def circle_field():
    """v = (-(y - c), (x - c), 0) / r on 48 x 48 x 3 in 1-based voxel coordinates, c = 24.5: [48, 48, 3, 3] Float32, Fortran order"""
    nx, ny, nz = CIRCLE_SHAPE
    x, y, _ = np.meshgrid(np.arange(1, nx + 1, dtype=np.float64), np.arange(1, ny + 1, dtype=np.float64), np.arange(nz), indexing="ij")
    r = np.hypot(x - CIRCLE_C, y - CIRCLE_C)
    v = np.stack([-(y - CIRCLE_C) / r, (x - CIRCLE_C) / r, np.zeros_like(r)], -1)
    return np.asfortranarray(v.astype(f32))


def circle_drift(line, seed, sub, c=CIRCLE_C):
    """max | ||p - c|| - ||p_seed - c|| | over a line's points, in the x-y plane (Float64)"""
    p = np.asarray(line, np.float64)[:, :2] - c
    p0 = np.asarray(seed, np.float64)[:2] + np.asarray(sub, np.float64)[:2] - c
    return float(np.abs(np.hypot(p[:, 0], p[:, 1]) - np.hypot(p0[0], p0[1])).max())
