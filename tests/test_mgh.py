"""CPU tests (no GPU): MGH / MGZ files.  The reader is held to files written byte by byte with `struct` here (nothing of the package's
writer is involved), the writer to the reader and to the expected byte count."""
import gzip
import os
import struct

import numpy as np
import pytest

F = np.float32
MGH_TYPES = {"FLOAT": (3, ">f4", np.float32), "INT": (1, ">i4", np.int32), "SHORT": (4, ">i2", np.int16), "UCHAR": (0, ">u1", np.uint8),
             "USHRT": (10, ">u2", np.uint16)}
DIMS = (3, 2, 2, 2)
DELTA = np.array([1.25, 0.75, 2.0], F)
MR_PARMS = np.array([2500.0, 0.1309, 3.5, 900.0], F)
C_RAS = np.array([-3.5, 12.25, 40.125], F)


def _cosines():
    """oblique direction cosines: columns x_ras, y_ras, z_ras, as float32"""
    az, ax = np.deg2rad(25.0), np.deg2rad(-15.0)
    Rz = np.array([[np.cos(az), -np.sin(az), 0], [np.sin(az), np.cos(az), 0], [0, 0, 1]])
    Rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
    return (Rz @ Rx).astype(F)


def _expected_M(dims=DIMS):
    """float64 from the float32 header fields, Pcrs_c = dims / 2, rounded once"""
    MdcD = _cosines().astype(np.float64) * DELTA.astype(np.float64)
    M = np.eye(4)
    M[:3, :3] = MdcD
    M[:3, 3] = C_RAS.astype(np.float64) - MdcD @ (np.array(dims[:3], np.float64) / 2)
    return M.astype(F)


def _values(kind):
    _, _, dt = MGH_TYPES[kind]
    n = int(np.prod(DIMS))
    if dt == np.float32:
        return (np.arange(n) * 1.5 - 7.25).astype(dt)
    info = np.iinfo(dt)
    return np.linspace(info.min, info.max, n).astype(np.int64).astype(dt)


def _write_by_hand(path, kind, good=1, type_code=None, mr_parms=True):
    code, fmt, _ = MGH_TYPES[kind]
    vals = _values(kind)
    Mdc = _cosines()
    buf = struct.pack(">7i", 1, *DIMS, code if type_code is None else type_code, 1)
    buf += struct.pack(">h", good)
    buf += struct.pack(">3f", *DELTA)
    for col in range(3):                                       # x_ras, y_ras, z_ras: column by column
        buf += struct.pack(">3f", *Mdc[:, col])
    buf += struct.pack(">3f", *C_RAS)
    buf += b"\0" * (284 - len(buf))
    assert len(buf) == 284
    ch = {">f4": "f", ">i4": "i", ">i2": "h", ">u1": "B", ">u2": "H"}[fmt]
    buf += struct.pack(">%d%s" % (vals.size, ch), *vals.tolist())
    if mr_parms:
        buf += struct.pack(">4f", *MR_PARMS)
    with open(path, "wb") as fh:
        fh.write(buf)
    return vals.reshape(DIMS, order="F")


@pytest.mark.parametrize("kind", sorted(MGH_TYPES))
def test_load_mgh_reads_a_file_written_by_hand(fj, tmp_path, kind):
    path = str(tmp_path / ("hand_%s.mgh" % kind))
    want = _write_by_hand(path, kind)
    vol, M, mr_parms, volsz = fj.load_mgh(path)
    assert tuple(volsz) == DIMS and vol.shape == DIMS and vol.dtype == MGH_TYPES[kind][2] and vol.flags.f_contiguous
    assert np.array_equal(vol, want)
    assert vol[1, 0, 0, 0] == want.reshape(-1, order="F")[1] and vol[0, 1, 0, 0] == want.reshape(-1, order="F")[3]      # x fastest
    assert M.dtype == F and np.array_equal(M, _expected_M())
    assert mr_parms.dtype == F and np.array_equal(mr_parms, MR_PARMS)
    hv, hM, hp, hsz = fj.load_mgh(path, headeronly=True)
    assert hv.size == 0 and np.array_equal(hM, M) and np.array_equal(hp, MR_PARMS) and tuple(hsz) == DIMS
    mri = fj.mri_read(path)
    assert mri.vol.dtype == vol.dtype and np.array_equal(mri.vol, want) and mri.tr == float(MR_PARMS[0])
    assert np.array_equal(mri.vox2ras, M) and np.allclose(mri.volres, DELTA, rtol=1e-6) and mri.bval is None and mri.bvec is None


def test_load_mgh_without_mr_parms_and_gzipped(fj, tmp_path):
    path = str(tmp_path / "short.mgh")
    want = _write_by_hand(path, "SHORT", mr_parms=False)
    vol, _M, mr_parms, _sz = fj.load_mgh(path)
    assert np.array_equal(vol, want) and mr_parms.size == 0
    gz = str(tmp_path / "short.mgz")
    with open(path, "rb") as src, gzip.open(gz, "wb") as dst:
        dst.write(src.read())
    vol2, M2, _p, _s = fj.load_mgh(gz)
    assert np.array_equal(vol2, want) and np.array_equal(M2, _expected_M())


def test_ras_good_flag_zero_is_the_references_error(fj, tmp_path):
    path = str(tmp_path / "nogeom.mgh")
    _write_by_hand(path, "FLOAT", good=0)
    with pytest.raises(ValueError, match="Loading .* as MGH"):
        fj.load_mgh(path)
    with pytest.raises(ValueError, match="Loading .* as MGH"):
        fj.mri_read(path)


def test_an_unknown_element_type_raises(fj, tmp_path):
    path = str(tmp_path / "long.mgh")
    _write_by_hand(path, "INT", type_code=2)                    # MRI_LONG
    with pytest.raises(ValueError, match="type"):
        fj.load_mgh(path)
    with pytest.raises(ValueError, match="not supported"):
        fj.save_mgh(np.zeros((2, 2, 2, 1), np.float64), str(tmp_path / "f64.mgh"))


def test_other_extensions_fail_as_before(fj, tmp_path):
    with pytest.raises(ValueError, match=r"File extension not supported by this back end \(NIfTI only\): x.img"):
        fj.mri_read("x.img")
    with pytest.raises(ValueError, match=r"File extension not supported by this back end \(NIfTI only\): x.img"):
        fj.mri_write(fj.MRI(np.zeros((2, 2, 2), F)), "x.img")


def _ulp_close(got, want):
    """every entry within one float32 ulp of the input's entry"""
    return np.all(np.abs(got.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want)).astype(np.float64))


@pytest.mark.parametrize("ext", [".mgh", ".mgz", ".mgh.gz"])
@pytest.mark.parametrize("kind", sorted(MGH_TYPES))
def test_save_mgh_load_mgh_round_trip(fj, tmp_path, kind, ext):
    """The volume comes back identical.  M is re-derived from delta / Mdc / c_ras, each rounded to float32 when written (three
    roundings between the input M and the one read back), so it is held to one float32 ulp per entry, not to bit identity."""
    vol = np.asfortranarray(_values(kind).reshape(DIMS, order="F"))
    M = _expected_M()
    path = str(tmp_path / ("rt_" + kind + ext))
    assert fj.save_mgh(vol, path, M, MR_PARMS) is False
    raw = (gzip.open(path, "rb") if ext != ".mgh" else open(path, "rb")).read()
    assert len(raw) == 284 + vol.size * vol.dtype.itemsize + 16
    if ext != ".mgh":
        assert open(path, "rb").read(2) == b"\x1f\x8b"
    got, M2, p2, sz = fj.load_mgh(path)
    assert got.dtype == vol.dtype and np.array_equal(got, vol) and tuple(sz) == DIMS
    assert np.array_equal(p2, MR_PARMS)
    err = np.abs(M2.astype(np.float64) - M.astype(np.float64)) / np.spacing(np.abs(M)).astype(np.float64)
    print("round-tripped M: worst entry %.2f ulp" % err.max())
    assert _ulp_close(M2, M)


def test_round_trip_of_a_matrix_no_file_delivered(fj, tmp_path):
    """A vox2ras that was not made from float32 header fields (voxel sizes and cosines that are not float32 products, any offset)
    is not held to one ulp: the offset is re-derived as c_ras - MdcD n / 2, a difference that cancels.  What the three roundings
    allow: delta, Mdc and c_ras are each rounded once (relative 2^-24), the product Mdc * delta and the offset once more, so
      |M'_ij - M_ij| <= 4 * 2^-24 |M_ij|   ((1 + 2^-24)^3 - 1, with 3 rounded up to 4 for the second-order terms) and
      |t'_i - t_i|   <= 2^-24 (|c_i| + |t_i|) + sum_j 4 * 2^-24 |M_ij| n_j / 2."""
    rng = np.random.default_rng(11)
    n = np.array(DIMS[:3], np.float64)
    u = 2.0 ** -24
    worst = 0.0
    for t in range(25):
        Q, _r = np.linalg.qr(rng.standard_normal((3, 3)))
        M = np.eye(4)
        M[:3, :3] = Q * rng.uniform(0.5, 3.0, 3)
        M[:3, 3] = rng.uniform(-100, 100, 3)
        M = M.astype(F)
        path = str(tmp_path / ("generic%d.mgh" % t))
        fj.save_mgh(np.zeros(DIMS, F), path, M, MR_PARMS)
        M2 = fj.load_mgh(path, headeronly=True)[1].astype(np.float64)
        M64 = M.astype(np.float64)
        assert np.all(np.abs(M2[:3, :3] - M64[:3, :3]) <= 4 * u * np.abs(M64[:3, :3]))
        c = M64[:3, :3] @ (n / 2) + M64[:3, 3]
        bound = u * (np.abs(c) + np.abs(M64[:3, 3])) * (1 + 2.0 ** -20) + 4 * u * (np.abs(M64[:3, :3]) @ (n / 2))
        err = np.abs(M2[:3, 3] - M64[:3, 3])
        worst = max(worst, (err / bound).max())
        assert np.all(err <= bound), (err, bound)
        assert np.array_equal(M2[3], [0, 0, 0, 1])
    print("generic M: worst offset error %.2f of its bound" % worst)


@pytest.mark.parametrize("ext", [".mgh", ".mgz"])
def test_mri_write_mri_read_round_trip(fj, tmp_path, ext):
    for kind in ("FLOAT", "UCHAR"):
        vol = np.asfortranarray(_values(kind).reshape(DIMS, order="F"))
        mri = fj.MRI(vol, volres=tuple(float(v) for v in DELTA), vox2ras=_expected_M())
        mri.tr = 2500.0
        path = str(tmp_path / ("mri_" + kind + ext))
        assert fj.mri_write(mri, path) is False
        raw = (gzip.open(path, "rb") if ext == ".mgz" else open(path, "rb")).read()
        assert len(raw) == 284 + vol.size * vol.dtype.itemsize + 16
        back = fj.mri_read(path)
        assert back.vol.dtype == vol.dtype and np.array_equal(back.vol, vol) and back.nframes == DIMS[3]
        assert back.tr == 2500.0 and _ulp_close(back.vox2ras, mri.vox2ras)
        assert np.allclose(back.volres, DELTA, rtol=1e-6)
        assert back.bval is None


def test_mgh_b_tables_use_the_nifti_lookup(fj, tmp_path):
    vol = np.zeros(DIMS, F, order="F")
    path = str(tmp_path / "dwi.mgz")
    fj.save_mgh(vol, path, _expected_M(), MR_PARMS)
    np.savetxt(str(tmp_path / "dwi.bval"), np.array([0.0, 1000.0]))
    np.savetxt(str(tmp_path / "dwi.bvec"), np.array([[0.0, 0.0, 0.0], [0.0, 3.0, 4.0]]))
    mri = fj.mri_read(path)
    assert np.array_equal(mri.bval, np.array([0, 1000], F)) and np.allclose(mri.bvec[1], [0, 0.6, 0.8])
    assert os.path.exists(path)
