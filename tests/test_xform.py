"""The host layer of the transform port (fibers.jl_amd/xform.py) against the restatement (tests/xform_ref.py) and the reference's
text: xfm_read of FreeSurfer .lta files (types 0 and 1, every missing-field error) and FSL .mat files (both determinant signs),
xfm_inv / xfm_compose / voxrot, str_xform's header, str_merge and the integer form of xfm_apply!.  No GPU needed."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import xform_ref as ref  # noqa: E402

SRC = dict(size=(96, 90, 60), res=(2.0, 2.0, 2.5), xras=(-0.9986, 0.0523, 0.0), yras=(0.0349, 0.6663, -0.7449),
           zras=(-0.039, -0.7438, -0.6669), cras=(1.5, -20.25, 10.0))
DST = dict(size=(256, 256, 256), res=(1.0, 1.0, 1.0), xras=(-1.0, 0.0, 0.0), yras=(0.0, 0.0, -1.0), zras=(0.0, 1.0, 0.0),
           cras=(0.5, -17.0, 19.0))
REG = np.array([[0.9994, -0.0312, 0.0151, 2.125], [0.0309, 0.9993, 0.0207, -4.5], [-0.0158, -0.0202, 0.9997, 7.75],
                [0.0, 0.0, 0.0, 1.0]])


def _f(v):
    return " ".join("%.6f" % x for x in v)


def _lta(path, regtype, reg=REG, drop=None, src=SRC, dst=DST):
    lines = ["# transform file %s" % path, "# created by test", "type      = %d # LINEAR_%s" % (regtype, "RAS_TO_RAS" if regtype else "VOX_TO_VOX"),
             "nxforms   = 1", "mean      = 0.0000 0.0000 0.0000", "sigma     = 1.0000", "1 4 4"]
    lines += [_f(r) for r in reg]
    for side, v in (("src", src), ("dst", dst)):
        lines += ["%s volume info" % side, "valid = 1  # volume info valid", "filename = /data/%s.nii.gz" % side,
                  "volume = %d %d %d" % tuple(v["size"]), "voxelsize = %s" % _f(v["res"]), "xras   = %s" % _f(v["xras"]),
                  "yras   = %s" % _f(v["yras"]), "zras   = %s" % _f(v["zras"]), "cras   = %s" % _f(v["cras"])]
    lines += ["subject test", "fscale 0.100000"]
    if drop is not None:
        side, key = drop
        if side is None:
            lines = [ln for ln in lines if not ln.startswith(key)]
        else:
            start = lines.index("%s volume info" % side)
            k = next(i for i in range(start, len(lines)) if lines[i].startswith(key))
            del lines[k]
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    return str(path)


def _fields32(v):
    return {k: (np.asarray(x, np.float32).astype(np.float64) if k != "size" else np.asarray(x, np.float64)) for k, x in v.items()}


@pytest.mark.parametrize("regtype", [0, 1])
def test_lta_geometry_and_matrices_match_a_float64_derivation(fj, tmp_path, regtype):
    x = fj.xfm_read(_lta(tmp_path / "reg.lta", regtype))
    reg32 = np.asarray(REG, np.float32)
    A, B, v2v, r2r = ref.derive_lta(regtype, reg32, _fields32(SRC), _fields32(DST))
    assert x.insize.tolist() == list(SRC["size"]) and x.outsize.tolist() == list(DST["size"])
    assert np.array_equal(x.inres, np.float32(SRC["res"])) and np.array_equal(x.outres, np.float32(DST["res"]))
    for got, want in ((x.invox2ras, A), (x.outvox2ras, B), (x.vox2vox, v2v), (x.ras2ras, r2r)):
        assert got.dtype == np.float32
        assert np.allclose(got, want, rtol=1e-6, atol=1e-6 * np.abs(want).max())
    # the given matrix is stored as read; ras2ras = outvox2ras vox2vox invox2ras^-1 either way round
    assert np.array_equal(x.vox2vox if regtype == 0 else x.ras2ras, reg32)
    lhs = x.outvox2ras.astype(np.float64) @ x.vox2vox @ np.linalg.inv(x.invox2ras.astype(np.float64))
    assert np.allclose(lhs, x.ras2ras, rtol=1e-5, atol=1e-4)
    u, _, vt = np.linalg.svd(x.vox2vox[:3, :3].astype(np.float64))
    assert np.allclose(x.voxrot, u @ vt, atol=1e-6)


MISSING = [((None, "type"), "Missing transform type in "), ((None, "1 4 4"), "Missing transform matrix in "),
           (("src", "volume"), "Missing source dimensions in "), (("dst", "volume"), "Missing destination dimensions in "),
           (("src", "voxelsize"), "Missing source resolution in "), (("dst", "voxelsize"), "Missing destination resolution in "),
           (("src", "xras"), "Missing source x_ras in "), (("dst", "xras"), "Missing destination x_ras in "),
           (("src", "yras"), "Missing source y_ras in "), (("dst", "yras"), "Missing destination y_ras in "),
           (("src", "zras"), "Missing source z_ras in "), (("dst", "zras"), "Missing destination z_ras in "),
           (("src", "cras"), "Missing source c_ras in "), (("dst", "cras"), "Missing destination c_ras in ")]


@pytest.mark.parametrize("drop,msg", MISSING)
def test_lta_missing_fields_raise_the_reference_errors(fj, tmp_path, drop, msg):
    path = tmp_path / "bad.lta"
    if drop == (None, "1 4 4"):                                   # the matrix header and its four rows
        _lta(path, 1)
        lines = open(path).read().splitlines()
        k = lines.index("1 4 4")
        open(path, "w").write("\n".join(lines[:k] + lines[k + 5:]) + "\n")
    else:
        _lta(path, 1, drop=drop)
    with pytest.raises(ValueError) as e:
        fj.xfm_read(str(path))
    assert str(e.value) == msg + str(path)


def test_lta_invalid_type(fj, tmp_path):
    path = _lta(tmp_path / "t2.lta", 2)
    with pytest.raises(ValueError) as e:
        fj.xfm_read(path)
    assert str(e.value) == "Invalid transform type 2 in " + path


def _vol(fj, shape, res, flip):
    M = np.diag([res[0], res[1], res[2], 1.0]).astype(np.float32)
    if flip:                                                      # det < 0: the usual radiological x axis
        M[0, 0] = -M[0, 0]
    M[:3, 3] = (-40.0, 30.0, -12.5)
    return fj.MRI(np.zeros(shape, np.uint8), volres=res, vox2ras=M)


@pytest.mark.parametrize("flip", [False, True])
def test_fsl_mat_identity_and_translation(fj, tmp_path, flip):
    vol = _vol(fj, (40, 36, 30), (1.5, 1.25, 2.0), flip)
    det = np.linalg.det(vol.vox2ras.astype(np.float64))
    assert (det > 0) == (not flip)
    f = tmp_path / "id.mat"
    np.savetxt(f, np.eye(4), fmt="%.6f")
    x = fj.xfm_read(str(f), vol, vol)
    assert np.allclose(x.vox2vox, np.eye(4), atol=1e-6)
    assert np.allclose(x.ras2ras, np.eye(4), atol=1e-5)
    assert x.insize.tolist() == [40, 36, 30] and np.array_equal(x.outvox2ras, vol.vox2ras)
    t = np.eye(4)
    t[:3, 3] = (3.0, -2.5, 4.0)                                  # FSL millimetres
    np.savetxt(f, t, fmt="%.6f")
    x = fj.xfm_read(str(f), vol, vol)
    sx = -1.0 if det > 0 else 1.0                                 # FSL's x runs the other way when det(vox2ras) > 0
    assert np.allclose(x.vox2vox[:3, :3], np.eye(3), atol=1e-6)
    assert np.allclose(x.vox2vox[:3, 3], (sx * 3.0 / 1.5, -2.5 / 1.25, 4.0 / 2.0), atol=1e-5)


def _some_xform(fj, tmp_path, regtype=1, name="a.lta", reg=REG):
    return fj.xfm_read(_lta(tmp_path / name, regtype, reg=reg))


def test_inv_compose_and_voxrot(fj, tmp_path):
    a = _some_xform(fj, tmp_path)
    rot = np.array([[0.0, -1.0, 0.0, 10.0], [1.0, 0.0, 0.0, -3.0], [0.0, 0.0, 1.0, 1.5], [0.0, 0.0, 0.0, 1.0]])
    b = fj.xfm_read(_lta(tmp_path / "b.lta", 1, reg=rot, src=DST, dst=SRC))        # DST space -> SRC space
    ia = fj.xfm_inv(a)
    assert ia.insize.tolist() == a.outsize.tolist() and np.array_equal(ia.invox2ras, a.outvox2ras)
    assert np.array_equal(ia.voxrot, a.voxrot.T)
    c = fj.xfm_compose(ia, a)
    assert np.allclose(c.vox2vox, np.eye(4), atol=1e-5) and np.allclose(c.ras2ras, np.eye(4), atol=1e-5)
    # the last argument is applied first: compose(b, a) maps SRC -> DST -> SRC
    ba = fj.xfm_compose(b, a)
    assert ba.insize.tolist() == a.insize.tolist() and ba.outsize.tolist() == b.outsize.tolist()
    assert np.array_equal(ba.invox2ras, a.invox2ras) and np.array_equal(ba.outvox2ras, b.outvox2ras)
    assert np.allclose(ba.vox2vox, b.vox2vox.astype(np.float64) @ a.vox2vox, rtol=1e-6, atol=1e-5)
    assert not np.allclose(ba.vox2vox, a.vox2vox.astype(np.float64) @ b.vox2vox, atol=1e-2)
    abc = fj.xfm_compose(a, b, a)
    assert np.allclose(abc.ras2ras, a.ras2ras.astype(np.float64) @ b.ras2ras @ a.ras2ras, rtol=1e-5, atol=1e-4)
    for x in (a, b, ba, abc):
        assert np.allclose(x.voxrot.astype(np.float64) @ x.voxrot.T, np.eye(3), atol=1e-6)
    v = np.array([0.3, -0.5, 0.8], np.float32)
    r = fj.xfm_rotate(a, v)
    assert r.dtype == np.float32 and np.allclose(r, a.voxrot.astype(np.float64) @ v, atol=1e-7)


def test_str_xform_header_is_that_of_the_output_geometry(fj, tmp_path):
    from fibers_jl_amd.trk import tract_header
    x = fj.Xform(insize=(20, 20, 20), outsize=(30, 25, 20), outres=(1.5, 1.25, 2.0),
                 outvox2ras=np.array([[0, 0, -2.0, 20], [1.5, 0, 0, -30], [0, 1.25, 0, 5], [0, 0, 0, 1]], np.float32))
    tr = fj.Tract(xyz=np.zeros((0, 3), np.float32), npts=np.zeros(0, np.int32), volsize=(20, 20, 20), seed_index=np.zeros(0, np.int64))
    t2 = fj.str_xform(x, tr)
    assert t2.volsize == (30, 25, 20) and t2.volres == (1.5, 1.25, 2.0) and np.array_equal(t2.vox2ras, x.outvox2ras)
    f = str(tmp_path / "x.trk")
    assert fj.trk_write(t2, f) is False
    hdr = open(f, "rb").read()[:1000]
    mri = fj.MRI(np.zeros((30, 25, 20), np.uint8), volres=(1.5, 1.25, 2.0), vox2ras=x.outvox2ras)
    assert hdr == tract_header(mri, n_count=0)
    assert hdr[948:952] == b"ASL\0" and hdr[952:956] == b"ASL\0"              # voxel_order(_original): columns +y, +z, -x
    assert np.frombuffer(hdr[6:12], np.int16).tolist() == [30, 25, 20]
    assert np.array_equal(np.frombuffer(hdr[440:504], np.float32).reshape(4, 4), x.outvox2ras)


def _tract(fj, nlines, seed, scalars=True, props=True):
    rng = np.random.default_rng(seed)
    npts = rng.integers(1, 7, nlines).astype(np.int32)
    n = int(npts.sum())
    return fj.Tract(xyz=rng.random((n, 3)).astype(np.float32), npts=npts, volsize=(10, 12, 14), volres=(1.0, 1.0, 1.5),
                    scalars=rng.random(n).astype(np.float32) if scalars else None,
                    properties=rng.random((nlines, 2)).astype(np.float32) if props else None)


def test_str_merge(fj):
    a, b, c = _tract(fj, 5, 1), _tract(fj, 3, 2), _tract(fj, 4, 3)
    m = fj.str_merge(a, b, c)
    xyz, npts, sc, pr = ref.str_merge(a, b, c)
    assert m.nstr == 12 and np.array_equal(m.npts, npts) and np.array_equal(m.xyz, xyz)
    assert np.array_equal(m.scalars, sc) and np.array_equal(m.properties, pr)
    assert np.array_equal(m.offsets, np.concatenate([[0], np.cumsum(npts)]))
    assert np.array_equal(m.line(6), b.line(1))
    assert m.volsize == a.volsize and m.n_scalars == 1 and m.n_properties == 2
    assert a.nstr == 5                                            # the inputs are left alone
    d = _tract(fj, 2, 4)
    d.volsize = (10, 12, 15)
    with pytest.raises(ValueError, match=r"Mismatch in header field dim between input tracts \(\(10, 12, 14\), \(10, 12, 15\)\)"):
        fj.str_merge(a, d)
    with pytest.raises(ValueError, match="Mismatch in header field n_properties"):
        fj.str_merge(a, _tract(fj, 2, 5, props=False))
    e = _tract(fj, 2, 6)
    e.vox2ras = np.diag([1.0, 1.0, 1.5, 1.0]).astype(np.float32)
    e.vox2ras[0, 3] = 1.0
    with pytest.raises(ValueError, match="Mismatch in header field vox_to_ras"):
        fj.str_merge(a, e)


def test_integer_apply_rounds_ties_to_even(fj):
    m = np.eye(4, dtype=np.float32)
    m[:3, 3] = 0.5
    x = fj.Xform(vox2vox=m)
    pts = np.array([[0.0, 1.0, 2.0], [-1.0, -2.0, 3.0], [4.0, 5.0, -0.25]], np.float32)   # +0.5: 0.5 1.5 2.5 -0.5 -1.5 3.5 4.5 5.5 0.25
    out = np.zeros((3, 3), np.int64)
    assert fj.xfm_apply(x, pts, out=out) is out
    assert out.tolist() == [[0, 2, 2], [0, -2, 4], [4, 6, 0]]
    assert np.array_equal(out, np.rint(ref.apply_f32(m, pts)).astype(np.int64))
    with pytest.raises(OverflowError):
        fj.xfm_apply(x, np.array([np.nan, 0, 0], np.float32), out=np.zeros(3, np.int32))
