"""CPU tests of the brain mask: the NumPy restatement (tests/mask_ref.py) against independent routes (scipy.ndimage, the textbook Otsu),
the known answer of the ball phantom, the library's refusals (fib_dwi_mask_check needs no device) and what the three host wrappers
pass to the library."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mask_ref as ref  # noqa: E402

SHAPES = [(13, 9, 7), (3, 2, 1), (1, 1, 1), (16, 16, 4), (5, 5, 5)]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_the_key_orders_every_pattern_and_inverts():
    v = np.array([-np.inf, -3.5, -1e-45, -0.0, 0.0, 1e-45, 2.0, np.inf], np.float32)
    k = ref.key(v)
    assert np.all(np.diff(k.astype(np.int64)) > 0)
    assert np.array_equal(_bits(ref.unkey(k)), _bits(v))
    nan_neg, nan_pos = np.array([0xFFC00000], np.uint32).view(np.float32), np.array([0x7FC00000], np.uint32).view(np.float32)
    assert ref.key(nan_neg)[0] < k[0] and ref.key(nan_pos)[0] > k[-1]
    raw = np.random.default_rng(0).integers(0, 2 ** 32, 1000, dtype=np.uint64).astype(np.uint32)
    assert np.array_equal(ref.unkey(ref.key(raw.view(np.float32))).view(np.uint32), raw)


@pytest.mark.parametrize("shape", SHAPES, ids=str)
@pytest.mark.parametrize("radius", [1, 2, 3])
def test_median_is_scipys(shape, radius):
    nd = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(radius)
    for vol in (rng.integers(0, 4, shape).astype(np.float32), rng.normal(0, 1, shape).astype(np.float32)):
        want = nd.median_filter(vol, size=2 * radius + 1, mode="nearest")
        assert np.array_equal(_bits(ref.median(vol, radius)), _bits(want))
    vol = rng.normal(0, 1, shape).astype(np.float32)
    assert np.array_equal(_bits(ref.median(vol, radius, 2)), _bits(ref.median(ref.median(vol, radius), radius)))
    assert np.array_equal(_bits(ref.median(vol, radius, 0)), _bits(vol))


def _canonical(lab):
    """labels of any numbering -> 1 + smallest linear index (x fastest) of each"""
    flat = lab.reshape(-1, order="F")
    out = np.zeros(flat.size, np.int32)
    for u in np.unique(flat[flat != 0]):
        idx = np.flatnonzero(flat == u)
        out[idx] = idx[0] + 1
    return out.reshape(lab.shape, order="F")


@pytest.mark.parametrize("shape, density", [((13, 9, 7), 0.5), ((16, 16, 4), 0.3), ((5, 5, 5), 0.7), ((3, 2, 1), 0.5), ((1, 1, 1), 1.0)], ids=str)
def test_components_holes_and_dilation_are_scipys(shape, density):
    nd = pytest.importorskip("scipy.ndimage")
    m = np.random.default_rng(7).random(shape) < density
    lab, n = nd.label(m)
    got = ref.components(m)
    assert np.array_equal(got, _canonical(lab)) and np.unique(got[got != 0]).size == n
    assert np.array_equal(m | ref.holes(m), nd.binary_fill_holes(m))
    for k in (0, 1, 3):
        assert np.array_equal(ref.dilate(m, k), nd.binary_dilation(m, iterations=k) if k else m)


def test_holes_known_cases():
    m = np.zeros((9, 9, 9), bool)
    m[2:7, 2:7, 2:7] = True
    m[4, 4, 4] = False                                       # enclosed
    assert ref.holes(m).sum() == 1
    m[4, 4, :4] = False                                      # a one-voxel channel to the face z = 0
    assert ref.holes(m).sum() == 0


def _textbook_otsu(h):
    """between-class variance on bin centres in float64, first maximum"""
    h = np.asarray(h, np.float64)
    centres = np.arange(256) + 0.5
    best, bestk = -1.0, -1
    for k in range(255):
        w0, w1 = h[: k + 1].sum(), h[k + 1:].sum()
        if w0 == 0 or w1 == 0:
            continue
        m0, m1 = (h[: k + 1] * centres[: k + 1]).sum() / w0, (h[k + 1:] * centres[k + 1:]).sum() / w1
        var = w0 * w1 * (m0 - m1) ** 2
        if var > best:
            best, bestk = var, k
    return bestk


def test_integer_otsu_picks_the_textbook_bin():
    rng = np.random.default_rng(11)
    for t in range(200):
        a = rng.normal(rng.uniform(20, 90), rng.uniform(3, 15), rng.integers(200, 4000))
        b = rng.normal(rng.uniform(140, 230), rng.uniform(3, 15), rng.integers(200, 4000))
        h = np.bincount(np.clip(np.concatenate([a, b]), 0, 255).astype(np.int64), minlength=256)
        assert ref.otsu(h) == _textbook_otsu(h), t            # (empty valley bins tie exactly in both forms: the first maximum)
    h = np.zeros(256, np.int64)
    h[10], h[200] = 50, 50                                   # two equal peaks, empty bins between: the first maximum
    assert ref.otsu(h) == 10
    h = np.zeros(256, np.int64)
    h[7] = 9
    assert ref.otsu(h) == -1


def test_bins_edges():
    v = np.array([1.0, 2.0, 3.0, np.nan, np.inf, -np.inf], np.float32)
    lo, hi = ref.finite_range(v)
    assert (lo, hi) == (1.0, 3.0)
    assert ref.bins(v, lo, hi).tolist() == [0, 128, 255, -1, -1, -1]
    assert ref.finite_range(np.array([np.nan, np.inf], np.float32)) is None
    lo, hi = ref.finite_range(np.array([0.0, -0.0], np.float32))
    assert np.signbit(lo) and not np.signbit(hi) and lo == hi


@pytest.mark.parametrize("seed", range(5))
def test_ball_phantom_known_answer(seed):
    dwi, ball = ref.ball_phantom((24, 24, 24), seed)
    b0 = ref.mean_frames(dwi, [0, 1, 2])
    # more than one component exists before the selection: the islands survive the median
    v = ref.median(b0, 1, 2)
    lo, hi = ref.finite_range(v)
    b = ref.bins(v, lo, hi)
    above = b > ref.otsu(np.bincount(b.reshape(-1), minlength=256))
    assert np.unique(ref.components(above)).size - 1 > 1
    m, _, info = ref.dwi_mask(dwi, [0, 1, 2], radius=1, numpass=2)
    assert info["status"] == 0 and info["n_components"] > 1
    d = ref.dice(m, ball)
    print("seed %d: Dice %.4f" % (seed, d))
    assert d >= 0.99
    c = (np.array(ball.shape) - 1) / 2.0
    x, y, z = np.meshgrid(*[np.arange(n) for n in ball.shape], indexing="ij")
    cav = (x - (c[0] + 8.5 / 3)) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2 <= 4.0
    assert cav.sum() > 20 and m[cav].all(), "the cavity is filled"
    assert not m[:5, :5, :5].any(), "the islands are gone"


def test_mean_is_in_the_lists_order():
    rng = np.random.default_rng(3)
    v = (rng.normal(0, 1, (4, 3, 2, 6)) * 10.0 ** rng.integers(-6, 6, (4, 3, 2, 6))).astype(np.float32)
    a, b = ref.mean_frames(v, [0, 1, 2, 3, 4, 5]), ref.mean_frames(v, [5, 4, 3, 2, 1, 0])
    assert np.allclose(a, b, rtol=1e-6) and np.array_equal(_bits(ref.mean_frames(v, [2])), _bits(v[..., 2]))
    assert np.array_equal(_bits(ref.mean_frames(v, [1, 1])), _bits(v[..., 1]))


# ---- the library's refusals (no device) -----------------------------------------------------------------------------------------------
def _check(fj, shape=(8, 8, 8), nframes=4, frames=(0,), **kw):
    fj.mask.dwi_mask_check(shape, nframes, list(frames), **kw)


@pytest.mark.parametrize("kw, code, words", [
    (dict(radius=0), -1, "radius must be 1, 2 or 3, not 0"),
    (dict(radius=4), -1, "radius must be 1, 2 or 3, not 4"),
    (dict(numpass=-1), -1, "numpass must not be negative"),
    (dict(dilate=-2), -1, "dilate must not be negative"),
    (dict(frames=()), -1, "the frame list is empty"),
    (dict(frames=(0, 4)), -1, "frame 4 (entry 1 of the list) is outside [0, 4)"),
    (dict(frames=(-1,)), -1, "frame -1 (entry 0 of the list) is outside [0, 4)"),
    (dict(shape=(1024, 1024, 129)), -7, "the limit is 2^27"),
    (dict(shape=(0, 4, 4)), -1, "must be positive"),
])
def test_refusals(fj, kw, code, words):
    with pytest.raises(fj.FibersError) as e:
        _check(fj, **kw)
    assert e.value.code == code and words in e.value.message, e.value.message


def test_accepted(fj):
    _check(fj)
    _check(fj, shape=(512, 512, 512), frames=(3, 3, 0), radius=3, numpass=0, dilate=5, keep_largest=False, fill_holes=False)
    _check(fj, shape=(1, 1, 1), nframes=1)


def test_struct_layouts(fj):
    from fibers_jl_amd import _lib
    assert C.sizeof(_lib.MaskParams) == 16 and C.sizeof(_lib.MaskInfo) == 64
    assert [(_lib.MaskInfo.threshold.offset), _lib.MaskInfo.n_above.offset, _lib.MaskInfo.n_mask.offset] == [16, 24, 56]


# ---- what the wrappers pass ------------------------------------------------------------------------------------------------------------
class Recorder:
    """stands in for the library: records the scalars and the bytes behind the input pointers"""

    def __init__(self):
        self.calls = []

    def fib_dwi_mask(self, dev, dwi, nx, ny, nz, nvol, frames, nframes, p, mask, b0, info):
        n = nx * ny * nz
        self.calls.append(("fib_dwi_mask", dev, (nx, ny, nz, nvol), C.string_at(dwi, 4 * n * nvol), C.string_at(frames, 4 * nframes), nframes,
                           tuple(getattr(p._obj, f) for f, _ in p._obj._fields_)))
        C.memset(mask, 1, n)
        C.memset(b0, 0, 4 * n)
        info._obj.n_mask = n
        return 0

    def fib_vol_median(self, dev, vol, nx, ny, nz, nf, radius, numpass, out):
        self.calls.append(("fib_vol_median", dev, (nx, ny, nz, nf), C.string_at(vol, 4 * nx * ny * nz * nf), radius, numpass))
        C.memmove(out, vol, 4 * nx * ny * nz * nf)
        return 0

    def fib_mask_components(self, dev, mask, nx, ny, nz, flags, labels, out_mask, info):
        n = nx * ny * nz
        self.calls.append(("fib_mask_components", dev, (nx, ny, nz), C.string_at(mask, n), flags, out_mask))
        lab = (np.frombuffer(C.string_at(mask, n), np.uint8) != 0).astype(np.int32) * 41
        C.memmove(labels, lab.ctypes.data, 4 * n)
        return 0


@pytest.fixture
def rec(fj, monkeypatch):
    from fibers_jl_amd import _lib
    r = Recorder()
    monkeypatch.setattr(_lib, "lib", lambda: r)
    return r


def _xfast(a, dtype):
    return np.asarray(a, dtype).tobytes(order="F")


def test_dwi_mask_arguments(fj, rec):
    vol = np.arange(3 * 4 * 5 * 6, dtype=np.float32).reshape(3, 4, 5, 6)
    bval = np.array([5, 1000, 5, 2000, 5, 1000], np.float32)
    forms = [fj.MRI(np.asfortranarray(vol), bval), fj.MRI(np.ascontiguousarray(vol), bval)]
    for d in forms:
        r = fj.dwi_mask(d, radius=1, numpass=3, fill_holes=False, dilate=2, device=1)
        assert isinstance(r, fj.BrainMask) and r.mask.vol.dtype == np.uint8 and r.mask.vol.shape == (3, 4, 5, 1) and r.b0.vol.dtype == np.float32
        assert r.info["n_mask"] == 60 and set(r.info) == set(fj.mask.INFO_FIELDS)
    assert rec.calls[0] == rec.calls[1]
    name, dev, dims, raw, frames, nframes, params = rec.calls[0]
    assert (name, dev, dims, nframes) == ("fib_dwi_mask", 1, (3, 4, 5, 6), 3)
    assert raw == _xfast(vol, np.float32) and frames == np.array([0, 2, 4], np.int32).tobytes()       # bval == minimum(bval)
    assert params == (1, 3, 1, 2)                                                                     # KEEP_LARGEST only
    fj.dwi_mask(vol)                                                                                  # no b-table: frame 0, the defaults
    assert rec.calls[2][4:] == (np.zeros(1, np.int32).tobytes(), 1, (2, 4, 3, 0))
    fj.dwi_mask(vol.astype(np.float64), frames=[5, 1, 1])                                             # converted; the list as given
    assert rec.calls[3][3] == _xfast(vol, np.float32) and rec.calls[3][4] == np.array([5, 1, 1], np.int32).tobytes()


def test_vol_median_arguments(fj, rec):
    vol = np.arange(2 * 3 * 4 * 2, dtype=np.float32).reshape(2, 3, 4, 2)
    a = fj.vol_median(fj.MRI(np.ascontiguousarray(vol)), radius=2, numpass=3)
    b = fj.vol_median(vol[..., 0])
    assert rec.calls[0] == ("fib_vol_median", 0, (2, 3, 4, 2), _xfast(vol, np.float32), 2, 3)
    assert rec.calls[1] == ("fib_vol_median", 0, (2, 3, 4, 1), _xfast(vol[..., 0], np.float32), 1, 1)
    assert a.vol.shape == (2, 3, 4, 2) and b.vol.shape == (2, 3, 4, 1) and np.array_equal(a.vol, vol)


def test_mask_components_arguments(fj, rec):
    m = np.zeros((3, 4, 2), np.int16)
    m[0, 1, 0], m[2, 3, 1], m[1, 1, 1] = -3, 7, 1                                                    # a signed mask: != 0
    want = _xfast(m != 0, np.uint8)
    for form in (m, fj.MRI(m), np.ascontiguousarray(m), m[..., None], m.astype(np.float64), m != 0):
        lab = fj.mask_components(form, keep_largest=True, fill_holes=True)
        assert lab.vol.dtype == np.int32 and lab.vol.shape == (3, 4, 2, 1)
        assert np.array_equal(lab.vol[..., 0], (m != 0).astype(np.int32))                            # compact: 41 -> 1
    assert all(c == ("fib_mask_components", 0, (3, 4, 2), want, 3, None) for c in rec.calls) and len(rec.calls) == 6
    lab = fj.mask_components(m, compact=False)
    assert rec.calls[-1][4] == 0 and np.array_equal(lab.vol[..., 0], (m != 0).astype(np.int32) * 41)
    with pytest.raises(ValueError):
        fj.mask_components(np.zeros((2, 2, 2, 3)))


def test_compact_labels(fj):
    lab = np.array([0, 17, 0, 5, 17, 900, 5], np.int32)
    assert fj.mask.compact_labels(lab).tolist() == [0, 2, 0, 1, 2, 3, 1]
    assert fj.mask.compact_labels(np.zeros(4, np.int32)).tolist() == [0, 0, 0, 0]
