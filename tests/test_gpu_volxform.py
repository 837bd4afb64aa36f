"""Volume resampling on the GPU (fibd_vol_xform, fib_vol_xform, mri_xform), bit for bit against the NumPy restatement
(tests/volxform_ref.py, pinned on the CPU by tests/test_volxform_ref.py) over every output voxel: both interpolations, affine and
projective matrices, rows longer than a workgroup, all-outside and all-NaN coordinates, 4-byte-aligned views on a side stream, the
host form under every frame chunking, narrow integer types, the refused arguments, and the road from an .mgz label file to a
connectome.  Shapes are a few hundred voxels: the file runs in seconds.  In-process only."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import volxform_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

F = np.float32
FIB_ERR_INVALID, FIB_ERR_UNSUPPORTED = -1, -7
SMALL, LARGE = (7, 5, 3), (9, 6, 4)


def _projective():
    """an output -> input matrix whose last row is not 0 0 0 1"""
    M = R.out2in(R.oblique()).copy()
    M[3] = (0.002, -0.001, 0.0015, 1.0)
    return M


def _floats(nf, shape, seed):
    nx, ny, nz = shape
    return (np.random.default_rng(seed).standard_normal((nf, nz, ny, nx)) * 100).astype(F)


def _labels(nf, shape, seed):
    nx, ny, nz = shape
    return np.random.default_rng(seed).integers(-5, 2000, (nf, nz, ny, nx)).astype(np.int32)


def _same_bits(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))


def _device(fj, M, vol, inshape, outshape, interp, outside, **kw):
    """vol [nf, nz, ny, nx] through vol_xform_device -> [nf, nzo, nyo, nxo]"""
    import torch
    d = torch.from_numpy(np.ascontiguousarray(vol).reshape(vol.shape[0], -1)).cuda()
    out = fj.vol_xform_device(M, d, inshape, outshape, interp=interp, outside=outside, **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy().reshape((vol.shape[0],) + tuple(outshape)[::-1])


@pytest.fixture(scope="module")
def matrices():
    return {"oblique": R.out2in(R.oblique()), "oblique_back": R.oblique(), "projective": _projective()}


@pytest.mark.parametrize("outside", [np.nan, -1.0])
@pytest.mark.parametrize("nframes", [1, 3])
@pytest.mark.parametrize("direction", ["up", "down"])
def test_device_form_on_the_main_grids(fj, matrices, direction, nframes, outside):
    """7 x 5 x 3 -> 9 x 6 x 4 through the oblique transform and the projective matrix, and the reverse through the oblique one's
    inverse: float32 under both interpolations, int32 labels under nearest"""
    inshape, outshape = (SMALL, LARGE) if direction == "up" else (LARGE, SMALL)
    names = ("oblique", "projective") if direction == "up" else ("oblique_back",)
    v, lab = _floats(nframes, inshape, 2), _labels(nframes, inshape, 3)
    for name in names:
        M = matrices[name]
        ok = R.inside_mask(R.pull_back(M, outshape), inshape)
        assert 0 < ok.sum() < ok.size, name                                      # both branches of the inside test are taken
        for interp in ("nearest", "trilinear"):
            want = R.vol_xform_ref(M, v, inshape, outshape, interp, F(outside))
            got = _device(fj, M, v, inshape, outshape, interp, outside)
            assert _same_bits(got, want), (name, interp, int((got.view(np.uint32) != want.view(np.uint32)).sum()))
        fill = np.int32(-1) if outside == -1.0 else np.int32(0x7FC00000)
        want = R.vol_xform_ref(M, lab, inshape, outshape, "nearest", fill)
        got = _device(fj, M, lab, inshape, outshape, "nearest", int(fill))
        assert got.dtype == np.int32 and np.array_equal(got, want), name


@pytest.mark.parametrize("nframes", [4, 5, 9])
def test_series_of_four_frames_and_more(fj, matrices, nframes):
    """from 4 frames on the launch takes the kernel whose frame loop goes four at a time: the threshold, one past it (a remainder of
    one) and two rounds plus one"""
    M = matrices["oblique"]
    v, lab = _floats(nframes, SMALL, 20), _labels(nframes, SMALL, 21)
    for interp in ("nearest", "trilinear"):
        want = R.vol_xform_ref(M, v, SMALL, LARGE, interp, F(np.nan))
        assert _same_bits(_device(fj, M, v, SMALL, LARGE, interp, np.nan), want), interp
    assert np.array_equal(_device(fj, M, lab, SMALL, LARGE, "nearest", -1), R.vol_xform_ref(M, lab, SMALL, LARGE, "nearest", np.int32(-1)))


def test_one_frame_given_as_a_vector(fj, matrices):
    import torch
    v = _floats(1, SMALL, 4)
    out = fj.vol_xform_device(matrices["oblique"], torch.from_numpy(v.reshape(-1)).cuda(), SMALL, LARGE, interp="trilinear", outside=np.nan)
    assert tuple(out.shape) == (9 * 6 * 4,)
    assert _same_bits(out.cpu().numpy().reshape(LARGE[::-1]), R.vol_xform_ref(matrices["oblique"], v, SMALL, LARGE, "trilinear", F(np.nan))[0])


@pytest.mark.parametrize("interp", ["nearest", "trilinear"])
def test_rows_longer_than_a_workgroup(fj, interp):
    """300 x 3 x 2 <- 11 x 4 x 3: an output row is more than one 256-lane segment and no multiple of it (nor of a 64-lane tile), and
    3 x 2 rows are no multiple of a 4-row tile"""
    inshape, outshape = (11, 4, 3), (300, 3, 2)
    A = np.eye(4)
    az = np.deg2rad(12.0)
    A[:3, :3] = np.array([[np.cos(az), -np.sin(az), 0], [np.sin(az), np.cos(az), 0], [0, 0, 1]]) * np.array([10.5 / 299, 1.1, 1.2])
    A[:3, 3] = (0.1, 0.4, 0.3)
    M = A.astype(F)                                                               # output -> input: 300 voxels span the 11
    ok = R.inside_mask(R.pull_back(M, outshape), inshape)
    assert ok[:, :, 256:].any() and (~ok).any()                                   # the second segment of a row holds inside voxels
    v = _floats(2, inshape, 6)
    want = R.vol_xform_ref(M, v, inshape, outshape, interp, F(-1))
    assert _same_bits(_device(fj, M, v, inshape, outshape, interp, -1.0), want)


@pytest.mark.parametrize("interp", ["nearest", "trilinear"])
def test_all_outside_and_all_nan_coordinates_give_the_fill(fj, interp):
    inshape, outshape = (11, 4, 3), (300, 3, 2)
    v = _floats(2, inshape, 8)
    far = np.eye(4, dtype=F)
    far[:3, 3] = (1e6, -1e30, 400.0)
    nan = np.eye(4, dtype=F)
    nan[:3, 3] = np.nan                                                           # every coordinate NaN: the inside test comes
    huge = np.eye(4, dtype=F)                                                     # before any conversion to an integer
    huge[:3, :3] *= F(3e38)
    for M in (far, nan):
        ok = R.inside_mask(R.pull_back(M, outshape), inshape)
        assert not ok.any()
        got = _device(fj, M, v, inshape, outshape, interp, 7.5)
        assert got.shape == (2, 2, 3, 300) and np.all(got == F(7.5))
        assert _same_bits(got, R.vol_xform_ref(M, v, inshape, outshape, interp, F(7.5)))
    got = _device(fj, huge, v, inshape, outshape, interp, 7.5)                    # Inf coordinates everywhere but at o = 0
    assert _same_bits(got, R.vol_xform_ref(huge, v, inshape, outshape, interp, F(7.5)))


def test_views_one_element_into_a_buffer_on_a_side_stream(fj, matrices):
    import torch
    M = matrices["oblique"]
    nvi, nvo = 7 * 5 * 3, 9 * 6 * 4
    v = _floats(3, SMALL, 9)
    src = torch.zeros(3 * nvi + 1, dtype=torch.float32, device="cuda")
    dst = torch.full((3 * nvo + 2,), 123.0, dtype=torch.float32, device="cuda")
    src[1:] = torch.from_numpy(v.reshape(-1)).cuda()
    vin, vout = src[1:].view(3, nvi), dst[1:1 + 3 * nvo].view(3, nvo)
    assert vin.data_ptr() % 16 == 4 and vout.data_ptr() % 16 == 4
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = fj.vol_xform_device(M, vin, SMALL, LARGE, interp="trilinear", outside=-1.0, out=vout, stream=side)
    side.synchronize()
    assert got.data_ptr() == vout.data_ptr()
    want = R.vol_xform_ref(M, v, SMALL, LARGE, "trilinear", F(-1))
    assert _same_bits(got.cpu().numpy().reshape(want.shape), want)
    assert dst[0].item() == 123.0 and dst[-1].item() == 123.0                     # nothing written outside the view


def _as_mri(fj, vol):
    """[nf, nz, ny, nx] -> MRI ([nx, ny, nz, nf], Fortran-ordered)"""
    return fj.MRI(np.asfortranarray(vol.transpose(3, 2, 1, 0)))


def _from_mri(mri):
    return np.ascontiguousarray(mri.vol.transpose(3, 2, 1, 0))


def test_host_form_does_not_depend_on_the_frame_chunks(fj, monkeypatch):
    x = fj.Xform(insize=SMALL, outsize=LARGE, outres=(2.0, 1.5, 1.0), vox2vox=R.oblique(),
                 outvox2ras=np.array([[0, 0, -1.5, 20], [1.25, 0, 0, -30], [0, 2.0, 0, 5], [0, 0, 0, 1]], F))
    M = R.out2in(R.oblique())
    assert np.array_equal(fj.vol_xform_matrix(x), M)
    v = _floats(5, SMALL, 10)
    mri = _as_mri(fj, v)
    mri.bval, mri.bvec = np.ones(5, F), np.ones((5, 3), F)
    for interp in ("trilinear", "nearest"):
        want = R.vol_xform_ref(M, v, SMALL, LARGE, interp, F(np.nan))
        results = []
        for frames in (None, "1", "2"):
            if frames is None:
                monkeypatch.delenv("FIBERS_VOL_XFORM_FRAMES", raising=False)
            else:
                monkeypatch.setenv("FIBERS_VOL_XFORM_FRAMES", frames)
            res = fj.mri_xform(x, mri, interp=interp, outside=np.nan)
            assert res.volsize == LARGE and res.nframes == 5 and res.vol.dtype == F and res.vol.flags.f_contiguous
            assert res.volres == (2.0, 1.5, 1.0) and np.array_equal(res.vox2ras, x.outvox2ras)
            assert res.bval is None and res.bvec is None                        # gradients are not carried unrotated
            results.append(_from_mri(res))
        for r in results:
            assert _same_bits(r, want), interp
    monkeypatch.delenv("FIBERS_VOL_XFORM_FRAMES", raising=False)


@pytest.mark.parametrize("dtype", [np.uint8, np.int16, np.int8, np.uint16, np.uint32, np.int32])
def test_integer_volumes_under_nearest_keep_their_type(fj, dtype):
    x = fj.Xform(insize=SMALL, outsize=LARGE, vox2vox=R.oblique())
    info = np.iinfo(dtype)
    v = np.random.default_rng(12).integers(info.min, info.max, (2, 3, 5, 7), endpoint=True).astype(dtype)
    res = fj.mri_xform(x, _as_mri(fj, v), interp="nearest", outside=-1)
    assert res.vol.dtype == dtype
    wide = v.astype(np.int32 if info.min < 0 else np.uint32)
    fill = np.array([-1]).astype(dtype).astype(wide.dtype)[0]                     # `outside` cast to the volume's type first
    want = R.vol_xform_ref(R.out2in(R.oblique()), wide, SMALL, LARGE, "nearest", fill)
    assert np.array_equal(want.astype(dtype).astype(wide.dtype), want)           # narrowing back is exact
    assert np.array_equal(_from_mri(res), want.astype(dtype))


def test_identity_header_transform_returns_the_volume(fj):
    v = _floats(2, SMALL, 13)
    mri = _as_mri(fj, v)
    mri.vox2ras = np.array([[-2, 0, 0, 90], [0, 0, 2, -126], [0, -2, 0, 72], [0, 0, 0, 1]], F)
    mri.volres = (2.0, 2.0, 2.0)
    x = fj.xfm_header(mri, mri)
    assert np.array_equal(x.vox2vox, np.eye(4, dtype=F))
    for interp in ("nearest", "trilinear"):
        assert _same_bits(_from_mri(fj.mri_xform(x, mri, interp=interp)), v)


def test_from_an_mgz_label_file_to_a_connectome(fj, tmp_path):
    """labels on a 1 mm anatomical grid, written as .mgz, read back, moved onto a 2 mm diffusion grid of the same field of view by the
    header-only transform, and handed to str_connectome with a hand-made Tract"""
    az = np.deg2rad(12.0)
    Rm = np.array([[np.cos(az), -np.sin(az), 0], [np.sin(az), np.cos(az), 0], [0, 0, 1]])

    def header(res):
        M = np.eye(4)
        M[:3, :3] = Rm * res
        M[:3, 3] = np.array([-20.0, 13.0, 5.5]) + M[:3, :3] @ np.full(3, 0.5)
        return M.astype(F)
    anat, diff = (12, 10, 8), (6, 5, 4)
    i, j, k = np.meshgrid(np.arange(12), np.arange(10), np.arange(8), indexing="ij")
    lab = (1 + (i >= 6) + 2 * (j >= 5) + 4 * (k >= 4)).astype(np.int32)             # 8 blocks, labels 1..8
    path = str(tmp_path / "aparc+aseg.mgz")
    assert fj.mri_write(fj.MRI(np.asfortranarray(lab), volres=(1.0, 1.0, 1.0), vox2ras=header(1.0)), path) is False
    labmri = fj.mri_read(path)
    assert labmri.vol.dtype == np.int32 and np.array_equal(labmri.vol[..., 0], lab)
    dwi_ref = fj.MRI(np.zeros(diff, F), volres=(2.0, 2.0, 2.0), vox2ras=header(2.0))
    x = fj.xfm_header(labmri, dwi_ref)
    moved = fj.mri_xform(x, labmri, "nearest")
    assert moved.volsize == diff and moved.vol.dtype == np.int32
    want = R.vol_xform_ref(R.out2in(x.vox2vox), np.ascontiguousarray(labmri.vol.transpose(3, 2, 1, 0)), anat, diff, "nearest", np.int32(0))
    assert np.array_equal(_from_mri(moved), want)
    assert set(np.unique(want)) >= set(range(1, 9))                               # every block survived the move
    # lines in 1-based coordinates of the diffusion grid, from one block to another
    lines = [[(1.2, 1.1, 1.0), (3.0, 2.5, 2.0), (5.8, 4.9, 3.8)],                 # block 1 -> block 8
             [(5.6, 1.3, 1.4), (1.4, 4.6, 1.2)],                                  # block 2 -> block 3
             [(1.5, 1.5, 3.5), (5.5, 1.5, 3.5), (5.5, 4.5, 3.5)],                 # block 5 -> block 8
             [(2.0, 2.0, 2.0), (9.0, 2.0, 2.0)]]                                  # block 1 -> outside
    tr = fj.Tract(np.array([p for ln in lines for p in ln], F), np.array([len(ln) for ln in lines], np.int32), volsize=diff,
                  volres=(2.0, 2.0, 2.0), vox2ras=header(2.0))
    ids = list(range(1, 9))
    con = fj.str_connectome(tr, moved, ids=ids)
    ref = fj.str_connectome(tr, fj.MRI(np.asfortranarray(want[0].transpose(2, 1, 0))), ids=ids)
    assert np.array_equal(con.counts, ref.counts) and np.array_equal(con.assign, ref.assign)
    assert con.counts[1, 8] == 1 and con.counts[2, 3] == 1 and con.counts[5, 8] == 1 and con.counts.sum() >= 4


def test_refused_arguments(fj):
    import torch
    L = fj.lib()
    M = (C.c_float * 16)(*np.eye(4, dtype=F).reshape(-1).tolist())
    buf = torch.zeros(4096, dtype=torch.float32, device="cuda")
    p = buf.data_ptr()
    q = p + 4 * 2048
    assert L.fibd_vol_xform(M, p, 4, 4, 4, 1, 2, 0, q, 4, 4, 4, None) == FIB_ERR_INVALID                # unknown interp
    assert b"interpolation" in L.fib_last_error()
    assert L.fibd_vol_xform(M, p, 4, 4, 4, 1, -1, 0, q, 4, 4, 4, None) == FIB_ERR_INVALID
    for bad in ((0, 4, 4, 1, 4, 4, 4), (4, -1, 4, 1, 4, 4, 4), (4, 4, 4, 0, 4, 4, 4), (4, 4, 4, 1, 4, 0, 4), (4, 4, 4, 1, 4, 4, -3)):
        nxi, nyi, nzi, nf, nxo, nyo, nzo = bad
        assert L.fibd_vol_xform(M, p, nxi, nyi, nzi, nf, 0, 0, q, nxo, nyo, nzo, None) == FIB_ERR_INVALID, bad
    assert L.fibd_vol_xform(M, None, 4, 4, 4, 1, 0, 0, q, 4, 4, 4, None) == FIB_ERR_INVALID
    assert L.fibd_vol_xform(M, p, 4, 4, 4, 1, 0, 0, None, 4, 4, 4, None) == FIB_ERR_INVALID
    assert L.fibd_vol_xform(None, p, 4, 4, 4, 1, 0, 0, q, 4, 4, 4, None) == FIB_ERR_INVALID
    # any overlap: the same array, out one word inside vol's end, vol inside out
    assert L.fibd_vol_xform(M, p, 4, 4, 4, 1, 0, 0, p, 4, 4, 4, None) == FIB_ERR_INVALID
    assert b"overlap" in L.fib_last_error()
    assert L.fibd_vol_xform(M, p, 4, 4, 4, 1, 0, 0, p + 4 * 63, 4, 4, 4, None) == FIB_ERR_INVALID
    assert L.fibd_vol_xform(M, p + 4 * 8, 2, 2, 2, 1, 0, 0, p, 4, 4, 4, None) == FIB_ERR_INVALID
    assert L.fibd_vol_xform(M, p, 4, 4, 4, 1, 0, 0, p + 4 * 64, 4, 4, 4, None) == 0                     # adjacent is fine
    torch.cuda.synchronize()
    assert torch.all(buf == 0).item()
    # the host form
    hin, hout = np.zeros(64, F), np.zeros(64, F)
    assert L.fib_vol_xform(-1, M, hin.ctypes.data, 4, 4, 4, 1, 0, 0, hout.ctypes.data, 4, 4, 4) == FIB_ERR_UNSUPPORTED
    assert L.fib_vol_xform(0, M, hin.ctypes.data, 4, 4, 4, 1, 5, 0, hout.ctypes.data, 4, 4, 4) == FIB_ERR_INVALID
    assert L.fib_vol_xform(0, M, hin.ctypes.data, 4, 4, 0, 1, 0, 0, hout.ctypes.data, 4, 4, 4) == FIB_ERR_INVALID
    assert L.fib_vol_xform(0, M, hin.ctypes.data, 4, 4, 4, 1, 0, 0, hin.ctypes.data, 4, 4, 4) == FIB_ERR_INVALID
    # the Python layer
    x = fj.Xform(insize=SMALL, outsize=LARGE, vox2vox=R.oblique())
    with pytest.raises(ValueError, match="input space"):
        fj.mri_xform(x, fj.MRI(np.zeros(LARGE, F)))
    with pytest.raises(ValueError, match="int32"):
        fj.mri_xform(x, fj.MRI(np.zeros(SMALL, np.int32)), interp="trilinear")
    with pytest.raises(ValueError, match="float64"):
        fj.mri_xform(x, fj.MRI(np.zeros(SMALL, np.float64)))
    with pytest.raises(ValueError, match="float64"):
        fj.mri_xform(x, fj.MRI(np.zeros(SMALL, np.float64)), interp="nearest")
    with pytest.raises(ValueError, match="interp"):
        fj.mri_xform(x, fj.MRI(np.zeros(SMALL, F)), interp="cubic")
    with pytest.raises(ValueError, match="trilinear"):
        fj.vol_xform_device(np.eye(4, dtype=F), torch.zeros(105, dtype=torch.int32, device="cuda"), SMALL, LARGE)
    with pytest.raises(ValueError):
        fj.vol_xform_device(np.eye(4, dtype=F), torch.zeros(105, dtype=torch.float64, device="cuda"), SMALL, LARGE)
