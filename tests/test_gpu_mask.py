"""dwi_mask, vol_median and mask_components on the GPU against the NumPy restatement (tests/mask_ref.py), bit for bit: uint8 masks, int32
labels, the float32 bits of volumes, and the integers, float32 bits and float64 bits of `info`."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mask_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _dev(a):
    """host [nx,ny,nz] -> device [nvox], x fastest"""
    import torch
    return torch.from_numpy(np.array(a.reshape(-1, order="F"), order="C")).cuda()


def _planar(vol):
    import torch
    return torch.from_numpy(np.array(vol.reshape(-1, vol.shape[3], order="F").T, order="C")).cuda()


def _host(t, shape):
    return t.cpu().numpy().reshape(shape, order="F")


# ---- median ---------------------------------------------------------------------------------------------------------------------------
# smaller than the window and the tile; one past a tile edge (32 x 8 x 8) on each axis
MEDIAN_SHAPES = [(13, 9, 7), (3, 2, 1), (1, 1, 1), (33, 9, 9), (65, 17, 9)]
KINDS = ["ints", "const", "zeros", "nonfinite", "bits"]


@functools.lru_cache(maxsize=None)
def _median_data(shape, kind):
    rng = np.random.default_rng(len(kind) + 10 * shape[0])
    if kind == "ints":
        v = rng.integers(-2, 3, shape).astype(np.float32)
    elif kind == "const":
        v = np.full(shape, 3.25, np.float32)
    elif kind == "zeros":
        v = np.where(rng.random(shape) < 0.5, np.float32(0.0), np.float32(-0.0)).astype(np.float32)
    elif kind == "nonfinite":
        v = rng.normal(0, 1, shape).astype(np.float32)
        f = v.reshape(-1)
        idx = rng.permutation(f.size)[: max(3, f.size // 6)]
        f[idx] = rng.choice(np.array([np.nan, -np.nan, np.inf, -np.inf], np.float32), idx.size)
    else:
        v = rng.integers(0, 2 ** 32, shape, dtype=np.uint64).astype(np.uint32).view(np.float32)
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def _median_ref(shape, kind, radius):
    """passes 1 and 4 of the restatement"""
    v = _median_data(shape, kind)
    one = ref.median(v, radius, 1)
    return one, ref.median(one, radius, 3)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("radius", [1, 2, 3])
@pytest.mark.parametrize("shape", MEDIAN_SHAPES, ids=str)
def test_median_bit_for_bit(fj, shape, radius, kind):
    import torch
    v = _median_data(shape, kind)
    one, four = _median_ref(shape, kind, radius)
    d = _dev(v)
    for numpass, want in ((0, v), (1, one), (4, four)):
        got = _host(fj.mask.vol_median_device(d, shape, radius, numpass), shape)
        torch.cuda.synchronize()
        assert np.array_equal(_bits(got), _bits(want)), "numpass %d: %d voxels differ" % (numpass, np.count_nonzero(_bits(got) != _bits(want)))


@pytest.mark.parametrize("scheme", ["bisect", "columns"])
@pytest.mark.parametrize("radius", [1, 2, 3])
@pytest.mark.parametrize("shape", MEDIAN_SHAPES, ids=str)
def test_median_ab_partner_bit_for_bit(fj, monkeypatch, shape, radius, scheme):
    """both selection schemes at every radius (the diagnostic build's FIBERS_MEDIAN_SCHEME; the library runs bisection at radius 1 and
    2 and sorted columns at 3) give the same bits"""
    import ctypes as C
    import torch
    path = os.path.join(os.path.dirname(fj.LIB_PATH), "libfibers_hip_stamp.so")
    if not os.path.exists(path):
        pytest.skip("the diagnostic library is not built")
    L = C.CDLL(path)
    L.fibd_vol_median.restype = C.c_int
    L.fibd_vol_median.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
    monkeypatch.setenv("FIBERS_MEDIAN_SCHEME", scheme)
    n = int(np.prod(shape))
    for kind in ("ints", "nonfinite", "bits"):
        one, four = _median_ref(shape, kind, radius)
        d = _dev(_median_data(shape, kind))
        for numpass, want in ((1, one), (4, four)):
            out, work = torch.empty(n, dtype=torch.float32, device="cuda"), torch.empty(n + 16, dtype=torch.float32, device="cuda")
            assert L.fibd_vol_median(d.data_ptr(), *shape, radius, numpass, out.data_ptr(), work.data_ptr(), 4 * n + 64, None) == 0
            torch.cuda.synchronize()
            got = _host(out, shape)
            assert np.array_equal(_bits(got), _bits(want)), "%s numpass %d: %d voxels differ" % (kind, numpass, np.count_nonzero(_bits(got) != _bits(want)))


def test_median_host_form_frames_and_chunks(fj, monkeypatch):
    vol = np.stack([_median_data((13, 9, 7), k) for k in ("ints", "bits", "nonfinite")], axis=3)
    want = np.stack([ref.median(vol[..., f], 2, 2) for f in range(3)], axis=3)
    outs = []
    for nfc in (None, 1, 2):
        if nfc is None:
            monkeypatch.delenv("FIBERS_MEDIAN_FRAMES", raising=False)
        else:
            monkeypatch.setenv("FIBERS_MEDIAN_FRAMES", str(nfc))
        outs.append(fj.vol_median(fj.MRI(vol), radius=2, numpass=2).vol)
    for o in outs:
        assert np.array_equal(_bits(o), _bits(want))
    with pytest.raises(fj.FibersError) as e:
        fj.vol_median(vol, device=fj.DEVICE_ALL)
    assert e.value.code == -7 and "vol_median runs on one device" in e.value.message
    with pytest.raises(fj.FibersError) as e:
        fj.vol_median(vol, radius=4)
    assert e.value.code == -1


# ---- mean -----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _series():
    rng = np.random.default_rng(5)
    v = (rng.normal(0, 1, (9, 7, 5, 20)) * 10.0 ** rng.integers(-6, 6, (9, 7, 5, 20))).astype(np.float32)
    v = np.asfortranarray(v)
    v.setflags(write=False)
    return v


FRAME_LISTS = [[3], list(range(18)), [2, 2, 7], [11, 0, 19, 4, 1], list(range(20)) * 4]       # (80 frames: the frame-by-frame mode)


@pytest.mark.parametrize("frames", FRAME_LISTS, ids=lambda f: "%dframes" % len(f))
def test_mean_in_the_lists_order(fj, frames):
    import torch
    v = _series()
    want = ref.mean_frames(v, frames)
    o = fj.mask.dwi_mask_device(_planar(v), v.shape[:3], frames, numpass=0)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(_host(o["b0"], v.shape[:3])), _bits(want))
    r = fj.dwi_mask(fj.MRI(v), frames=frames, numpass=0)
    assert np.array_equal(_bits(r.b0.vol[..., 0]), _bits(want))


# ---- histogram / Otsu: the composed call with the stages after the threshold switched off ----------------------------------------------
def _threshold_only(fj, b0):
    """(mask, info) of mean -> histogram -> Otsu -> threshold on a one-frame series, device tier"""
    import torch
    shape = b0.shape
    o = fj.mask.dwi_mask_device(_dev(b0).reshape(1, -1), shape, [0], numpass=0, keep_largest=False, fill_holes=False)
    torch.cuda.synchronize()
    return _host(o["mask"], shape), fj.mask.info_dict(o["info"])


def _hold(got_mask, got_info, want_mask, want_info):
    bad = ref.info_equal(got_info, want_info)
    assert not bad, bad
    assert got_mask.dtype == np.uint8 and np.array_equal(got_mask, want_mask), "%d voxels differ" % np.count_nonzero(got_mask != want_mask)
    assert got_info["status"] != -1


def _otsu_cases():
    rng = np.random.default_rng(2)
    shape = (11, 6, 5)
    n = int(np.prod(shape))
    out = {}
    v = np.full(n, 7.0, np.float32)
    out["hi == lo"] = v.copy()
    v = np.full(n, 0.0, np.float32)
    v[::2] = -0.0
    out["+-0 only"] = v.copy()
    out["no finite value"] = np.where(rng.random(n) < 0.5, np.float32(np.nan), np.float32(np.inf)).astype(np.float32)
    v = np.full(n, 5.0, np.float32)
    v[-1] = 6.0                                              # all but one value in bin 0, the one at hi in bin 255
    out["one voxel at hi"] = v.copy()
    v = np.zeros(n, np.float32)
    v[: n // 2] = 10.0 / 256 * 100 + 0.1
    v[n // 2:] = 200.0 / 256 * 100 + 0.1
    v[0], v[-1] = 0.0, 100.0                                 # two peaks (bins 10 and 200) of equal size +- the two ends
    out["two peaks, empty bins between"] = v.copy()
    v = rng.normal(0, 1, n).astype(np.float32)
    v[rng.permutation(n)[:40]] = rng.choice(np.array([np.nan, np.inf, -np.inf], np.float32), 40)
    out["non-finite voxels excluded"] = v.copy()
    out["normal"] = (rng.normal(0, 1, n) + 5 * (rng.random(n) < 0.4)).astype(np.float32)
    out["wide range"] = (rng.normal(0, 1, n) * 10.0 ** rng.integers(-30, 30, n)).astype(np.float32)
    return {k: a.reshape(shape, order="F") for k, a in out.items()}


OTSU = _otsu_cases()


@pytest.mark.parametrize("name", sorted(OTSU))
def test_histogram_and_otsu(fj, name):
    b0 = OTSU[name]
    want_mask, _, want_info = ref.dwi_mask(b0[..., None], [0], numpass=0, flags=0)    # (the mean's sum starts from +0: -0 becomes +0)
    got_mask, got_info = _threshold_only(fj, b0)
    _hold(got_mask, got_info, want_mask, want_info)
    if name in ("hi == lo", "+-0 only", "no finite value"):
        assert got_info["status"] == 1 and not got_mask.any() and got_info["kstar"] == -1
    if name == "two peaks, empty bins between":
        assert got_info["kstar"] == 10                       # the first of the tied maxima
    if name == "one voxel at hi":
        assert got_info["n_above"] == 1 and got_mask.reshape(-1, order="F")[-1] == 1


VM_T, VM_MAX_BLOCKS = 256, 2048        # csrc/volmask.hip: the workgroup, and the min(vm_blocks(n), 2048) grid of vm_minmax_kernel / vm_hist_kernel
BIG_SHAPE = (81, 81, 81)


@functools.lru_cache(maxsize=None)
def _big_b0():
    """one frame of 81^3 = 531 441 voxels, 7153 more than one round of the capped grid: a positive skewed background, a brighter half
    (z >= 40) with an enclosed dark cavity across the voxel where the second round starts, and -- all past that voxel -- voxels brighter
    still (enough of them to move Otsu's k*), the finite extremes, a NaN, a +Inf and a -Inf"""
    rng = np.random.default_rng(12)
    n, per_round = int(np.prod(BIG_SHAPE)), VM_T * VM_MAX_BLOCKS
    flat = rng.gamma(2.0, 20.0, n) + 1.0
    flat[np.arange(n) // (81 * 81) >= 40] += 400.0
    flat[per_round:] += 500.0
    v = flat.astype(np.float32).reshape(BIG_SHAPE, order="F")
    x, y, z = per_round % 81, (per_round // 81) % 81, per_round // (81 * 81)
    assert (z, 1 <= x < 80, 1 <= y < 80) == (79, True, True)
    v[x - 1:x + 2, y - 1:y + 2, 78:80] = 0.5                  # the cavity: closed by z = 77 and the face plane z = 80
    f = v.reshape(-1, order="F")
    assert np.shares_memory(f, v)
    f[per_round + 100], f[per_round + 2000] = 0.25, 1500.0    # lo and hi
    f[per_round + 300], f[per_round + 301], f[per_round + 4000] = np.nan, np.inf, -np.inf
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def _big_ref(flags):
    return ref.mask_from_b0(_big_b0(), numpass=0, flags=flags, dilate_passes=0)


@pytest.mark.parametrize("flags", [0, 3], ids=["threshold", "largest+holes"])
def test_more_voxels_than_one_round_of_the_capped_grid(fj, flags):
    """vm_minmax_kernel and vm_hist_kernel (csrc/volmask.hip) run min(vm_blocks(n), 2048) workgroups of VM_T = 256 threads and stride on:
    524 288 voxels a round.  The extremes and the non-finite values lie in the second round, and its voxels move k*: lo, hi, kstar, the
    counts and the mask are the restatement's bit for bit only if both loops go round (the test asserts that the first round alone gives
    other extremes and another k*)."""
    import torch
    b0 = _big_b0()
    n, per_round = b0.size, VM_T * VM_MAX_BLOCKS
    print("%d voxels over min(vm_blocks, %d) x %d = %d a round: %.3f rounds" % (n, VM_MAX_BLOCKS, VM_T, per_round, n / per_round))
    assert n > per_round, "%d voxels stay inside one round of the 2048 x VM_T = %d of vm_minmax_kernel / vm_hist_kernel (csrc/volmask.hip)" % (n, per_round)
    want_mask, want_info = _big_ref(flags)
    first = b0.reshape(-1, order="F")[:per_round]
    r1 = ref.finite_range(first)
    assert (r1[0], r1[1]) != (want_info["lo"], want_info["hi"]) and want_info["lo"] == np.float32(0.25) and want_info["hi"] == np.float32(1500.0)
    b1 = ref.bins(first, want_info["lo"], want_info["hi"])
    k1 = ref.otsu(np.bincount(b1[b1 >= 0], minlength=256))
    print("lo, hi of the first round %s, of the volume %s; k* of the first round's histogram %d, of the volume's %d" % (
        r1, (want_info["lo"], want_info["hi"]), k1, want_info["kstar"]))
    assert k1 != want_info["kstar"], "the histogram of the first round alone gives the same k*: vm_hist_kernel's second round would not show"
    assert want_info["status"] == 0 and 0 < want_info["n_above"] < n
    if flags == 3:
        # the holes: the cavity's 18 voxels, the voxel at lo, and the NaN with the +Inf beside it (the -Inf and hi lie on the face z = 80)
        assert want_info["n_filled"] == 18 + 1 + 2 and want_info["n_components"] > 1 and want_info["n_kept"] < want_info["n_above"]
    o = fj.mask.dwi_mask_device(_dev(b0).reshape(1, -1), BIG_SHAPE, [0], numpass=0, keep_largest=bool(flags & 1), fill_holes=bool(flags & 2), dilate=0)
    torch.cuda.synchronize()
    _hold(_host(o["mask"], BIG_SHAPE), fj.mask.info_dict(o["info"]), want_mask, want_info)


# ---- components, holes, dilation ------------------------------------------------------------------------------------------------------
def _serpentine():
    m = np.zeros((16, 16, 4), bool)
    for z in (0, 2):
        for y in range(0, 16, 2):
            m[:, y, z] = True
            if y + 1 < 16:
                m[15 if (y // 2) % 2 == 0 else 0, y + 1, z] = True
    m[0, 15, 0:3] = True                                     # (row 15 is empty: the link between the two planes)
    m[0, 14, 0:3] = True
    return m


def _component_cases():
    rng = np.random.default_rng(9)
    out = {"serpentine": _serpentine()}
    m = np.zeros((6, 5, 4), bool)
    m[1, 1, 1] = m[2, 2, 1] = True                           # touch only diagonally: two
    m[4, 3, 2] = m[5, 4, 3] = True
    out["diagonal"] = m
    m = np.zeros((70, 20, 20), bool)                          # crosses every face of the median's tile and of the launch's blocks
    m[:, 9, 9] = True
    m[33, :, 9] = True
    m[33, 9, :] = True
    out["cross"] = m
    m = np.zeros((12, 6, 4), bool)
    m[1:4, 1:3, 1] = True
    m[7:10, 3:5, 2] = True                                   # two largest of six voxels each: the smaller label wins
    m[11, 0, 0] = True
    out["tie"] = m
    out["empty"] = np.zeros((7, 5, 3), bool)
    out["full"] = np.ones((7, 5, 3), bool)
    out["random 40^3"] = rng.random((40, 40, 40)) < 0.5
    out["one voxel"] = np.ones((1, 1, 1), bool)
    m = np.zeros((11, 11, 11), bool)
    m[1:10, 1:10, 1:10] = True
    m[3:8, 3:8, 3:8] = False                                  # a shell with a cavity ...
    m[5, 5, 5] = True                                         # ... an island in it ...
    out["hole, island in it"] = m.copy()
    m2 = np.zeros((13, 13, 13), bool)
    m2[1:12, 1:12, 1:12] = True
    m2[3:10, 3:10, 3:10] = False
    m2[5:8, 5:8, 5:8] = True
    m2[6, 6, 6] = False                                       # ... and a hole inside the hole's island
    out["hole inside a hole's island"] = m2
    m = np.zeros((9, 9, 9), bool)
    m[2:7, 2:7, 2:7] = True
    m[4, 4, 4] = False
    out["enclosed cavity"] = m.copy()
    m[4, 4, :4] = False
    out["cavity with a channel"] = m.copy()
    m = np.zeros((9, 9, 9), bool)
    m[0:6, 2:7, 2:7] = True
    m[0:3, 4, 4] = False
    out["cavity on a face"] = m
    return out


COMPONENTS = _component_cases()


@functools.lru_cache(maxsize=None)
def _components_ref(name, flags):
    return ref.mask_components(COMPONENTS[name], flags)


@pytest.mark.parametrize("flags", [0, 1, 2, 3])
@pytest.mark.parametrize("name", sorted(COMPONENTS))
def test_components_selection_and_holes(fj, name, flags):
    import torch
    m = COMPONENTS[name]
    lab, sel, info = _components_ref(name, flags)
    o = fj.mask.mask_components_device(_dev(m.astype(np.uint8) * 3), m.shape, bool(flags & 1), bool(flags & 2))
    torch.cuda.synchronize()
    got = fj.mask.info_dict(o["info"])
    assert got["status"] == 0
    _hold(_host(o["mask"], m.shape), got, sel, info)
    gl = _host(o["labels"], m.shape)
    assert gl.dtype == np.int32 and np.array_equal(gl, lab), "%d labels differ" % np.count_nonzero(gl != lab)


def test_component_cases_say_what_they_claim():
    n = lambda name, flags=0: ref.mask_components(COMPONENTS[name], flags)       # noqa: E731
    assert n("serpentine")[2]["n_components"] == 1 and COMPONENTS["serpentine"].sum() > 150
    assert n("diagonal")[2]["n_components"] == 4
    lab, sel, info = n("tie", 1)
    assert info["n_components"] == 3 and info["n_kept"] == 6 and sel[1, 1, 1] and not sel[7, 3, 2]
    assert n("random 40^3")[2]["n_components"] > 200
    assert n("enclosed cavity", 2)[2]["n_filled"] == 1 and n("cavity with a channel", 2)[2]["n_filled"] == 0
    assert n("cavity on a face", 2)[2]["n_filled"] == 0
    assert n("hole, island in it", 2)[2]["n_filled"] == 124 and n("hole, island in it", 3)[2]["n_filled"] == 125
    assert n("hole inside a hole's island", 2)[2]["n_filled"] == 7 ** 3 - 27 + 1


def test_mask_components_host_form(fj):
    m = COMPONENTS["random 40^3"][:17, :13, :9]
    lab, sel, info = ref.mask_components(m, 0)
    got, ginfo = fj.mask_components(np.where(m, -2, 0).astype(np.int16), compact=False, with_info=True)
    assert np.array_equal(got.vol[..., 0], lab) and not ref.info_equal(ginfo, info)
    c = fj.mask_components(fj.MRI(m.astype(np.uint8))).vol[..., 0]
    u = np.unique(lab[lab != 0])
    assert np.array_equal(c, np.searchsorted(u, lab) + (lab != 0)) and c.max() == u.size
    lab, sel, info = ref.mask_components(m, 3)
    got = fj.mask_components(m, keep_largest=True, fill_holes=True, compact=False)
    assert np.array_equal(got.vol[..., 0], lab)
    with pytest.raises(fj.FibersError) as e:
        fj.mask_components(m, device=fj.DEVICE_ALL)
    assert e.value.code == -7 and "mask_components runs on one device" in e.value.message


@pytest.mark.parametrize("passes", [0, 1, 3])
def test_dilation_at_the_faces(fj, passes):
    import torch
    b0 = np.zeros((9, 6, 5), np.float32)
    b0[0, 0, 0] = b0[8, 5, 4] = b0[4, 0, 2] = b0[4, 3, 4] = b0[8, 2, 2] = 100.0
    want_mask, want_info = ref.mask_from_b0(b0, numpass=0, flags=0, dilate_passes=passes)
    o = fj.mask.dwi_mask_device(_dev(b0).reshape(1, -1), b0.shape, [0], numpass=0, keep_largest=False, fill_holes=False, dilate=passes)
    torch.cuda.synchronize()
    _hold(_host(o["mask"], b0.shape), fj.mask.info_dict(o["info"]), want_mask, want_info)
    assert want_info["n_mask"] > want_info["n_above"] or passes == 0


# ---- the composed call ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _phantom(shape, seed):
    dwi, ball = ref.ball_phantom(shape, seed)
    dwi.setflags(write=False)
    return dwi, ball


@functools.lru_cache(maxsize=None)
def _phantom_ref(shape, seed, flags, dilate):
    return ref.dwi_mask(_phantom(shape, seed)[0], [0, 1, 2], 1, 2, flags, dilate)


@pytest.mark.parametrize("flags", [0, 1, 2, 3])
@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("shape", [(24, 24, 24), (29, 17, 11)], ids=str)
def test_ball_phantom_device_and_host(fj, shape, seed, flags):
    import torch
    dwi, ball = _phantom(shape, seed)
    dil = seed % 2
    want_mask, want_b0, want_info = _phantom_ref(shape, seed, flags, dil)
    kw = dict(radius=1, numpass=2, keep_largest=bool(flags & 1), fill_holes=bool(flags & 2), dilate=dil)
    o = fj.mask.dwi_mask_device(_planar(dwi), shape, [0, 1, 2], **kw)
    torch.cuda.synchronize()
    _hold(_host(o["mask"], shape), fj.mask.info_dict(o["info"]), want_mask, want_info)
    assert np.array_equal(_bits(_host(o["b0"], shape)), _bits(want_b0))
    r = fj.dwi_mask(fj.MRI(dwi), frames=[0, 1, 2], **kw)
    _hold(r.mask.vol[..., 0], r.info, want_mask, want_info)
    assert np.array_equal(_bits(r.b0.vol[..., 0]), _bits(want_b0))
    if shape == (24, 24, 24) and flags == 3 and dil == 0:
        assert ref.dice(r.mask.vol[..., 0], ball) >= 0.99


def test_default_radius_and_passes(fj):
    dwi, _ = _phantom((24, 24, 24), 0)
    want_mask, want_b0, want_info = ref.dwi_mask(dwi, [0], 2, 4)
    r = fj.dwi_mask(dwi)                                      # no b-table: frame 0; radius 2, four passes
    _hold(r.mask.vol[..., 0], r.info, want_mask, want_info)


def test_frame_chunks_give_identical_bytes(fj, monkeypatch):
    v = _series()
    frames = [11, 0, 19, 4, 1, 4]
    outs = []
    for nfc in (None, 1, 4, 6):
        if nfc is None:
            monkeypatch.delenv("FIBERS_MASK_FRAMES", raising=False)
        else:
            monkeypatch.setenv("FIBERS_MASK_FRAMES", str(nfc))
        r = fj.dwi_mask(fj.MRI(v), frames=frames, radius=1, numpass=1)
        outs.append((r.mask.vol.tobytes(), r.b0.vol.tobytes(), tuple(sorted((k, repr(x)) for k, x in r.info.items()))))
        b0 = r.b0.vol[..., 0]
    assert all(o == outs[0] for o in outs[1:])
    assert np.array_equal(_bits(b0), _bits(ref.mean_frames(v, frames)))


def test_refusals_and_the_device_set(fj):
    import torch
    dwi, _ = _phantom((24, 24, 24), 0)
    with pytest.raises(fj.FibersError) as e:
        fj.dwi_mask(dwi, device=fj.DEVICE_ALL)
    assert e.value.code == -7 and "dwi_mask runs on one device" in e.value.message
    with pytest.raises(fj.FibersError) as e:
        fj.dwi_mask(dwi, frames=[3])
    assert e.value.code == -1 and "outside [0, 3)" in e.value.message
    d = torch.zeros((2, 60), dtype=torch.float32, device="cuda")
    for kw in (dict(radius=0), dict(numpass=-1), dict(dilate=-1), dict(frames=[]), dict(frames=[2])):
        with pytest.raises(fj.FibersError) as e:
            fj.mask.dwi_mask_device(d, (5, 4, 3), **kw)
        assert e.value.code == -1
    v = torch.zeros(60, dtype=torch.float32, device="cuda")
    with pytest.raises(fj.FibersError) as e:
        fj.mask.vol_median_device(v, (5, 4, 3), radius=4)
    assert e.value.code == -1


def test_the_mask_goes_into_the_fit(fj):
    from fibers_jl_amd import phantom
    shape = (24, 24, 24)
    bval, bvec = phantom.scheme_dti(6, 2)
    vol, _, _ = phantom.make_volume(shape, bval, bvec, seed=4)
    _, ball = ref.ball_phantom(shape, 0)
    vol = np.asfortranarray(np.where(ball[..., None], vol, vol * 0.01).astype(np.float32))
    dwi = fj.MRI(vol, bval, bvec)
    bm = fj.dwi_mask(dwi, radius=1, numpass=2)
    m = bm.mask.vol[..., 0] != 0
    assert 0.9 * ball.sum() < m.sum() < 1.1 * ball.sum() and bm.info["status"] == 0
    assert np.array_equal(_bits(bm.b0.vol[..., 0]), _bits(ref.mean_frames(vol, np.flatnonzero(bval == bval.min()))))
    fit = fj.dti_fit(dwi, bm.mask)
    assert not fit.fa.vol[..., 0][~m].any() and not fit.md.vol[..., 0][~m].any() and fit.md.vol[..., 0][m].all()


# ---- device arguments -----------------------------------------------------------------------------------------------------------------
def _bad_forms(t):
    """a tensor like t, wrong in one way each: on the host, of another dtype, one element short, not contiguous"""
    import torch
    other = torch.float64 if t.dtype != torch.float64 else torch.float32
    wide = torch.zeros((t.numel(), 2), dtype=t.dtype, device=t.device)
    return {"host": t.cpu(), "dtype": t.to(other), "length": t.reshape(-1)[:-1].clone(), "strided": wide[:, 0]}


def test_device_arguments_are_checked_before_any_launch(fj, monkeypatch):
    import torch
    from fibers_jl_amd import _lib
    mk = fj.mask
    shape, n = (5, 4, 3), 60
    f32 = lambda k=n: torch.zeros(k, dtype=torch.float32, device="cuda")      # noqa: E731
    u8 = lambda: torch.zeros(n, dtype=torch.uint8, device="cuda")            # noqa: E731
    i32 = lambda: torch.zeros(n, dtype=torch.int32, device="cuda")           # noqa: E731
    info = lambda: torch.zeros(8, dtype=torch.int64, device="cuda")          # noqa: E731
    calls = {
        "median": (lambda a: mk.vol_median_device(a["vol"], shape, out=a["out"]), dict(vol=f32(), out=f32())),
        "components": (lambda a: mk.mask_components_device(a["mask"], shape, out=dict(labels=a["labels"], mask=a["omask"], info=a["info"])),
                       dict(mask=u8(), labels=i32(), omask=u8(), info=info())),
        "dwi_mask": (lambda a: mk.dwi_mask_device(a["dwi"], shape, [0], out=dict(mask=a["omask"], b0=a["b0"], info=a["info"])),
                     dict(dwi=f32(2 * n).reshape(2, n), omask=u8(), b0=f32(), info=info())),
    }
    for name, (fn, good) in calls.items():                                   # the good forms pass, so each refusal below is its own
        fn(good)
    torch.cuda.synchronize()
    launched = []
    real = _lib.lib()

    class Watch:
        def __getattr__(self, k):
            if k.startswith("fibd_") and not k.endswith("_work_size"):
                launched.append(k)
            return getattr(real, k)
    monkeypatch.setattr(_lib, "lib", lambda: Watch())
    for name, (fn, good) in calls.items():
        for arg, t in good.items():
            for how, bad in _bad_forms(t).items():
                if arg == "dwi" and how in ("length", "strided"):
                    bad = torch.zeros((2, n + 1), dtype=torch.float32, device="cuda")[:, :n] if how == "strided" else \
                        torch.zeros((2, n - 1), dtype=torch.float32, device="cuda")
                with pytest.raises(fj.mask.ArgError):
                    fn(dict(good, **{arg: bad}))
        with pytest.raises(fj.mask.ArgError):                                # a workspace that is too small
            {"median": lambda: mk.vol_median_device(good["vol"], shape, numpass=2, work=torch.zeros(8, dtype=torch.uint8, device="cuda")),
             "components": lambda: mk.mask_components_device(good["mask"], shape, work=torch.zeros(8, dtype=torch.uint8, device="cuda")),
             "dwi_mask": lambda: mk.dwi_mask_device(good["dwi"], shape, [0], work=torch.zeros(8, dtype=torch.uint8, device="cuda"))}[name]()
    with pytest.raises(fj.mask.ArgError):
        v = f32()
        mk.vol_median_device(v, shape, out=v)
    assert not launched, launched
    if torch.cuda.device_count() > 1:
        with pytest.raises(fj.mask.ArgError):
            mk.vol_median_device(f32(), shape, out=torch.zeros(n, dtype=torch.float32, device="cuda:1"))
