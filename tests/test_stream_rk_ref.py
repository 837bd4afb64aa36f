"""The NumPy restatement of the trilinear tracker's integrators (tests/stream_rk_ref.py, the definition in include/fibers_hip.h under
fib_stream_params.interp) pinned by known answers -- it is what tests/test_gpu_stream_rk.py compares the HIP tracer with bit for bit.
No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stream_rk_ref as rk  # noqa: E402

from oracle import oracle_np as onp  # noqa: E402

f32 = np.float32


def _planar(vol):
    """[nx, ny, nz, 3] -> the oracle's [3, 1, nx, ny, nz]"""
    return np.ascontiguousarray(np.transpose(vol, (3, 0, 1, 2))[:, None]).astype(f32)


def test_euler_path_is_the_oracles_trilinear_tracker():
    """integrator="euler" adds nothing of its own: point for point oracle_np.stream_line(..., interp="trilinear") on a noisy field
    with mask holes, with and without smoothing"""
    rng = np.random.default_rng(7)
    n = 9
    x, y, z = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
    v = np.stack([np.cos(0.2 * x + 0.1 * z), np.sin(0.2 * x + 0.1 * z), 0.3 * np.sin(y / 3.0)], -1) + 0.25 * rng.normal(size=(n, n, n, 3))
    v /= np.linalg.norm(v, axis=-1, keepdims=True)
    mask = rng.random((n, n, n)) < 0.9
    ov = _planar(v) * mask[None, None]
    sub = np.array([[0.1, -0.2, 0.3], [-0.25, 0.15, 0.05]], f32)
    nlines = npoints = 0
    for seed in np.argwhere(mask)[::7] + 1:
        for s in sub:
            for smooth in (0.2, 0.0):
                want = onp.stream_line([int(q) for q in seed], s, ov, mask, smooth=smooth, len_max=14, interp="trilinear")
                got = rk.stream_line([int(q) for q in seed], s, ov, mask, smooth=smooth, len_max=14, integrator="euler")
                assert got.shape == want.shape and np.array_equal(got, want)
                nlines += 1
                npoints += got.shape[0]
    assert nlines > 150 and npoints > 4 * nlines


def _circle_lines(step, integrator):
    ov = _planar(rk.circle_field())
    mask = np.ones(rk.CIRCLE_SHAPE, bool)
    return [rk.stream_line(list(seed), rk.CIRCLE_SUB[0], ov, mask, step=step, smooth=0.0, len_max=100, integrator=integrator)
            for seed in rk.CIRCLE_SEEDS]


# drift = max | ||p - c|| - ||p_seed - c|| | over a line.  The bounds are 3-5 x what this restatement gives (Euler 0.775-1.336 at step
# 0.5; RK2 <= 0.0012 / 0.0105 and RK4 <= 0.0021 / 0.0042 at steps 0.5 / 1.0) and far below Euler's: a wrong stage weight or a missing
# `half` fails them.
@pytest.mark.parametrize("step,integrator,lo,hi", [(0.5, "euler", 0.5, None), (0.5, "rk2", None, 0.01), (0.5, "rk4", None, 0.01),
                                                   (1.0, "euler", None, None), (1.0, "rk2", None, 0.03), (1.0, "rk4", None, 0.03)])
def test_circular_field_drift(step, integrator, lo, hi):
    """every line has 102 points (len_max = 100) for all three integrators; Euler walks off its circle, RK2 and RK4 stay on it"""
    lines = _circle_lines(step, integrator)
    for seed, line in zip(rk.CIRCLE_SEEDS, lines):
        assert line.shape[0] == 102, (seed, line.shape)
        drift = rk.circle_drift(line, seed, rk.CIRCLE_SUB[0])
        print("step %.1f %-5s seed %s drift %.5f" % (step, integrator, seed, drift))
        if lo is not None:
            assert drift >= lo, (seed, drift)
        if hi is not None:
            assert drift <= hi, (seed, drift)


@pytest.mark.parametrize("direction", [(1.0, 0.0, 0.0), (1.0 / 3, 2.0 / 3, 2.0 / 3)])
def test_uniform_field_every_integrator_gives_the_same_line(direction):
    n = 12
    ov = _planar(np.broadcast_to(np.array(direction, f32), (n, n, n, 3)).copy())
    mask = np.ones((n, n, n), bool)
    for seed, sub in (((3, 4, 5), (0.1, -0.2, 0.3)), ((6, 6, 6), (0.0, 0.0, 0.0))):
        lines = [rk.stream_line(list(seed), np.array(sub, f32), ov, mask, smooth=0.0, integrator=i) for i in rk.INTEGRATORS]
        assert lines[0].shape[0] > 6
        assert all(ln.shape == lines[0].shape and np.array_equal(ln, lines[0]) for ln in lines[1:])


def test_a_stage_without_a_direction_ends_the_pass_without_emitting_the_point():
    """The only non-zero voxels are a rod one voxel wide along x -- voxels x = 1..8 of the row (y, z) = (6, 6), vectors +x -- and one
    island voxel at x = 10.  Seed (6, 6, 6), no offset, step 2, no smoothing.  Forward, Euler: emits 6 (nxt = 8), emits 8 (nxt = 10 is
    the island: a pick, and D(10) = the island's vector), ends at nxt = 12.  RK2 / RK4: emit 6 (stages at 7 and 8), and at pos = 8 the
    midpoint 9.0 lies in the gap: its cell's corner x = 9 has no vector and corner x = 10 has weight 0 -- the blend is empty, the stage
    is NONE, the pass ends and 8 is NOT emitted although Euler's own nxt = 10 would have been valid."""
    n = 14
    v = np.zeros((n, n, n, 3), f32)
    v[:8, 5, 5] = np.array([1, 0, 0], f32)
    v[9, 5, 5] = np.array([1, 0, 0], f32)
    ov = _planar(v)
    mask = np.ones((n, n, n), bool)                                  # the mask is open: only the vectors say where the rod is
    pos, ex, h = np.array([8.0, 6.0, 6.0], f32), np.array([1, 0, 0], f32), f32(2.0)
    assert np.array_equal(rk.next_position(pos, ex, ov, h, "euler"), [10.0, 6.0, 6.0])
    assert rk.next_position(pos, ex, ov, h, "rk2") is None and rk.next_position(pos, ex, ov, h, "rk4") is None
    le, l2, l4 = [rk.stream_line([6, 6, 6], np.zeros(3, f32), ov, mask, step=2.0, smooth=0.0, len_max=20, integrator=i) for i in rk.INTEGRATORS]
    assert np.array_equal(le[:, 0], [8.0, 6.0, 6.0, 4.0])            # [forward reversed, backward]: backward ends at nxt = 0, outside
    assert np.array_equal(l2[:, 0], [6.0, 6.0, 4.0]) and np.array_equal(l4, l2)
    assert np.all(le[:, 1:] == 6.0) and np.all(l2[:, 1:] == 6.0)
