"""What the Python host tier hands to the fib_* entries: every public function that passes host pointers is run against a recorder that
stands in for the library, and the record -- entry name, scalar arguments, the bytes behind every input pointer -- (a) does not depend on
how the caller held the data and (b) is what the ABI's layout says, written out element by element (x fastest, frame slowest).

No GPU and no built library: `_lib.lib` is replaced (the technique of tests/test_table_args.py).  The recorder answers FIB_OK, clears the
output buffers the wrappers allocate uninitialised and fills the few results a wrapper reads back.  Only public names are used."""
import ctypes as C
import struct

import numpy as np
import pytest

SHAPE, NF = (3, 2, 4), 7                     # three distinct extents; 7 frames
NVOX = 24
ZEROED = 0x100                               # FIB_MASK_OUTPUTS_ZEROED

# ---------------------------------------------------------------------------------------------------------------------------------------
# the recorder
# ---------------------------------------------------------------------------------------------------------------------------------------
# One row per entry, one word per argument, in the order of include/fibers_hip.h:
#   name            a scalar (also a variable of the byte counts)
#   name:bytes      an input pointer to `bytes` bytes (None allowed)
#   name>bytes      an output pointer; cleared when `bytes` is given
#   name=           a ctypes array passed as such (float[16], float[3])
#   name*n:bytes    an array of n input pointers, `bytes` each
#   name@code       a mask pointer whose element type is the scalar `code` (DTYPES, flags above bit 7)
#   name&           an input struct by reference (its integer fields become variables)
_FIT = "dev vol:4*nx*ny*nz*nvol nx ny nz nvol mask@mdt mdt bval:4*nvol "
_STREAM = ("dev prm& ov*nvec:12*nx*ny*nz f*nvec:4*nx*ny*nz f_thresh fa:4*nx*ny*nz fa_thresh mask@mdt mdt seed@sdt sdt sub:12*nsub nsub ")
_LINES = "dev xyz:12*npnt npts:4*nl nl npnt "
_PEAKS = "dev odf:4*(nv//2)*nvox nvox v:12*nv nv f:12*nf nf "
_FIELD = "dev disp:12*nx*ny*nz nx ny nz "
_RESAMPLE = "vol:4*nxi*nyi*nzi*nf nxi nyi nzi nf code bits out>4*nxo*nyo*nzo*nf nxo nyo nzo"
TABLE = {
    "fib_dti_fit": _FIT + "bvec:12*nvol out>",
    "fib_adc_fit": _FIT + "adc> s0>",
    "fib_dki_fit": _FIT + "bvec:12*nvol v:12*nv nv prm& out>",
    "fib_csd_rec": _FIT + "bvec:12*nvol v:12*nv nv f:12*nf nf prm& out>",
    "fib_gqi_rec": _FIT + "bvec:12*nvol v:12*nv nv f:12*nf nf sigma odf> peak> qa>",
    "fib_dsi_rec": _FIT + "bvec:12*nvol v:12*nv nv f:12*nf nf hann pdf> odf> peak> qa>",
    "fib_rumba_rec": _FIT + "bvec:12*nvol v:12*nv nv niter lpar lperp lcsf lgm ncoils sos ipat tv out> sm> ss>",
    "fib_find_peaks": _PEAKS + "top>12*nvox nvalid>4*nvox",
    "fib_find_peaks_work": _PEAKS + "pk>4*(nv//2)*nvox isort>4*(nv//2)*nvox nvalid>4*nvox",
    "fib_dwi_denoise": "dev vol:4*nx*ny*nz*nvol nx ny nz nvol mask:nx*ny*nz patch est out> sigma> rank>",
    "fib_st_eigen": "dev S*6:4*nvox nvox eigvec>36*nvox eigval>12*nvox",
    "fib_st_recon": "dev vol:4*nx*ny*nz nx ny nz sigma rho eigvec>36*nx*ny*nz eigval>12*nx*ny*nz",
    "fib_stream": _STREAM + "out>",
    "fib_stream_lcm": _STREAM + "lcm:40*nx*ny*nz lcm_thresh rng out>",
    "fib_prob_stream": ("dev nx ny nz odf:4*nx*ny*nz*nvert nvert U:12*nvert mask:nx*ny*nz seed:nx*ny*nz sub:12*nsub nsub len_min len_max cos "
                        "step pmf submin rng out>"),
    "fib_tract_free": "out>",
    "fib_xfm_apply": "dev M= p:12*n out>12*n n",
    "fib_vol_xform": "dev M= " + _RESAMPLE,
    "fib_warp_points": _FIELD + "A= Q= B= xyz:12*n out>12*n n",
    "fib_warp_volume": _FIELD + "A= Q= B= " + _RESAMPLE,
    "fib_warp_invert": _FIELD + "Y= Q= niter inv>12*nxo*nyo*nzo err>4*nxo*nyo*nzo nxo nyo nzo",
    "fib_str_density": _LINES + "nx ny nz mode d:4*nx*ny*nz nout>",
    "fib_str_sample": "dev xyz:12*n n vol:4*nx*ny*nz*nf nx ny nz nf outside s>4*n*nf",
    "fib_str_stats": _LINES + "res= sc:4*npnt*ns ns p>4*nl*(1+ns)",
    "fib_str_select": _LINES + "nx ny nz rois*nroi:nx*ny*nz nroi m0 m1 m2 m3 min_npts max_npts keep> hits>12*nl counts>",
    "fib_str_connectome": _LINES + "nx ny nz res= lab:4*nx*ny*nz remap:4*nremap nremap L flags cmat:4*(L+1)**2 wmat:8*(L+1)**2 assign>8*nl n>",
    "fib_str_resample": _LINES + "res= K flip:nl out>12*nl*K",
    "fib_str_assign": "dev a:12*nl*K nl K m:12*nm*K nm res= thresh label>4*nl dist>4*nl flip>nl dist_all>",
    "fib_str_centroids": "dev a:12*nl*K nl K label:4*nl flip:nl nm flags sums:24*nm*K counts:4*nm",
}
_CODE_DTYPE = {}                             # DTYPES code -> numpy dtype, filled from the package's table by `rec`


class Mask:
    """a mask argument: its DTYPES code (flags stripped) and the bytes behind the pointer"""

    def __init__(self, code, raw):
        self.code, self.raw = code, raw

    def values(self):
        return None if self.raw is None else np.frombuffer(self.raw, _CODE_DTYPE[self.code]).astype(np.float64).tobytes()


def _scalar(v):
    return struct.pack("<d", v) if isinstance(v, float) else v              # (NaN compares equal as bytes)


def _fields(obj):
    return tuple((n, _scalar(getattr(obj, n))) for n, _ in obj._fields_)


class Recorder:
    def __init__(self):
        self.calls = []                      # (entry, {argument: what was recorded})
        self._own = (C.c_int32 * 1)(), (C.c_int64 * 1)(), (C.c_float * 3)(), (C.c_uint8 * 1)()

    def __getattr__(self, name):
        if name not in TABLE:
            raise AttributeError(name)
        return lambda *args: self._call(name, args)

    def _call(self, name, args):
        words = TABLE[name].split()
        assert len(words) == len(args), "%s takes %d arguments, got %d" % (name, len(words), len(args))
        var, seen = {}, {}
        for w, a in zip(words, args):                                            # first the scalars: they size the pointers
            if w.isidentifier():
                var[w] = seen[w] = _scalar(a)
            elif w.endswith("&"):
                seen[w[:-1]] = _fields(a._obj)
                var.update({n: v for n, v in seen[w[:-1]] if isinstance(v, int)})
        size = lambda expr: int(eval(expr, {}, dict(var)))                       # noqa: E731
        grab = lambda p, n: None if p is None else C.string_at(p, n)             # noqa: E731
        for w, a in zip(words, args):
            if ":" in w:
                key, expr = w.split(":")
                if "*" in key:
                    key, count = key.split("*")
                    seen[key] = None if a is None else tuple(grab(a[k], size(expr)) for k in range(size(count)))
                else:
                    seen[key] = grab(a, size(expr))
            elif "@" in w:
                key, code = w.split("@")
                seen[key] = Mask(var[code] & 0xFF, grab(a, size("nx*ny*nz") * _CODE_DTYPE[var[code] & 0xFF].itemsize))
                seen[code] = var[code] & ~0xFF                                   # the flags; the element type travels with the mask
            elif w.endswith("="):
                seen[w[:-1]] = None if a is None else bytes(a)
            elif ">" in w and not w.endswith(">") and a is not None:
                C.memset(a, 0, size(w.split(">")[1]))
        if name == "fib_str_select":                                             # every line kept
            C.memset(args[words.index("keep>")], 1, var["nl"])
            args[-1][0], args[-1][1] = var["nl"], var["npnt"]
        elif name == "fib_str_connectome":
            args[-1]._obj.value = var["nl"]
        elif name in ("fib_stream", "fib_stream_lcm", "fib_prob_stream"):        # a tractogram of no lines, in arrays of the recorder
            t = args[-1]._obj
            t.nlines = t.npoints = 0
            for field, own in zip(("npts", "seed_index", "xyz", "flags"), self._own):
                setattr(t, field, C.cast(own, type(getattr(t, field))))
        self.calls.append((name, seen))
        return 0

    def canon(self):
        """the calls with every mask as the values it holds, whatever element type carried them"""
        return [(name, {k: v.values() if isinstance(v, Mask) else v for k, v in seen.items()}) for name, seen in self.calls]

    def only(self, name):
        got = [seen for n, seen in self.calls if n == name]
        assert len(got) == 1, "%d calls of %s" % (len(got), name)
        return got[0]


@pytest.fixture
def rec(fj, monkeypatch):
    from fibers_jl_amd import _lib
    _CODE_DTYPE.update({code: np.dtype(name) for name, code in _lib.DTYPES.items()})
    r = Recorder()
    monkeypatch.setattr(_lib, "lib", lambda: r)
    return r


# ---------------------------------------------------------------------------------------------------------------------------------------
# the data, and the forms a caller may hold it in
# ---------------------------------------------------------------------------------------------------------------------------------------
def xfast(a, dtype):
    """the elements of `a` one by one, first index fastest and last index slowest, as bytes of `dtype`"""
    a = np.asarray(a)
    return np.array([a[idx[::-1]] for idx in np.ndindex(*a.shape[::-1])], dtype).tobytes()


def rowwise(a, dtype):
    """the elements of `a` one by one, last index fastest"""
    a = np.asarray(a)
    return np.array([a[idx] for idx in np.ndindex(*a.shape)], dtype).tobytes()


def values(shape, start=1.0, step=0.25):
    """distinct values, exact in float32"""
    n = int(np.prod(shape))
    return (start + step * np.arange(n, dtype=np.float64)).reshape(shape)


DWI = values(SHAPE + (NF,)).astype(np.float32)
INSIDE = (np.arange(NVOX).reshape(SHAPE) % 3 != 0).astype(np.int64)              # 0 / 1, no symmetry between the axes
SEEDS = (np.arange(NVOX).reshape(SHAPE) % 5 == 1).astype(np.int64)
BVAL = np.array([0.0] + [1000.0] * 3 + [2000.0] * 3)
BVEC = np.random.default_rng(5).standard_normal((NF, 3))
BVEC /= np.linalg.norm(BVEC, axis=1, keepdims=True)
PTS = values((7, 3), 0.5, 0.125)                                                 # three lines of 1, 4 and 2 points
NPTS = np.array([1, 4, 2])
SUB = np.array([[0.125, -0.25, 0.375], [0.0, 0.0, 0.0]])
RESPONSE = (1.7e-3, 0.2e-3, 1.0)

BASE = dict(order="F", f64=False, mask_mri=True, mask_dtype=np.uint8, mask_4d=False, flat=False, late=False)
FORMS = [BASE] + [dict(BASE, **d) for d in (
    dict(order="C"), dict(f64=True), dict(order="C", f64=True), dict(mask_mri=False), dict(mask_mri=False, mask_4d=True),
    dict(mask_dtype=np.bool_), dict(mask_dtype=np.int16, mask_mri=False, order="C"), dict(mask_dtype=np.float64), dict(flat=True),
    dict(flat=True, f64=True), dict(late=True))]


def held(a, F, widen=True):
    """`a` in the memory order of the form and, where the form says so and the function converts, in float64"""
    a = np.asarray(a)
    dt = np.float64 if widen and F["f64"] and a.dtype.kind == "f" else a.dtype
    return np.array(a, dtype=dt, order=F["order"])


def table(a, F):
    """a b-table: float64 lists, or float32 arrays in the form's order"""
    return np.asarray(a, np.float64).tolist() if F["f64"] else np.array(a, np.float32, order=F["order"])


def mask_of(fj, inside, F, mri=None):
    m = np.array(np.asarray(inside).astype(F["mask_dtype"]), order=F["order"])
    if F["mask_mri"] if mri is None else mri:
        return fj.MRI(m)
    return m[..., None] if F["mask_4d"] else m


def dwi_of(fj, F):
    if F["late"]:                                                                # fields assigned after the MRI was built
        d = fj.MRI(np.zeros(SHAPE + (NF,), np.float32))
        d.vol, d.bval, d.bvec = np.ascontiguousarray(DWI), BVAL.tolist(), np.ascontiguousarray(BVEC)
        return d
    return fj.MRI(held(DWI, F, widen=False), bval=table(BVAL, F), bvec=table(BVEC, F))


def tract_of(fj, F, pts=PTS, npts=NPTS, **kw):
    xyz = np.array(pts, np.float64 if F["f64"] else np.float32, order=F["order"])
    return fj.Tract(xyz.reshape(-1) if F["flat"] else xyz, np.asarray(npts, np.int64 if F["f64"] else np.int32), volsize=SHAPE,
                    volres=(1.0, 2.0, 3.0), **kw)


def vol_of(fj, a, F, mri=None):
    """a scalar volume as an MRI or an array ([nx, ny, nz] or [nx, ny, nz, 1])"""
    return mask_of(fj, a, dict(F, mask_dtype=np.float64 if F["f64"] else np.float32), mri)


def _warp(fj, F):
    field = fj.MRI(held(0.125 * values(SHAPE + (3,)), F, widen=False).astype(np.float32))
    if F["late"]:
        field.vol = np.ascontiguousarray(field.vol)
    field.vox2ras = np.array([[2, 0, 0, -3], [0, 2, 0, -2], [0, 0, 2, -4], [0, 0, 0, 1]], np.float32)
    return fj.warp.Warp(field)


def _xform(fj):
    M = np.array([[1, 0.25, 0, 0.5], [0, 2, 0, -1], [0.5, 0, 1, 2], [0, 0, 0, 1]], np.float32)
    return fj.Xform(insize=SHAPE, outsize=(2, 3, 2), outres=(2, 1, 3), vox2vox=M)


def _models(fj, F):
    return tract_of(fj, F, values((6, 3), 1.0, 0.375), [3, 3])


def _stream(fj, F, **kw):
    ov = [values(SHAPE + (3,), -1.0, 0.03125), values(SHAPE + (3,), 2.0, 0.0625)]
    f = [values(SHAPE, 0.25, 0.03125), values(SHAPE, 0.5, 0.015625)]
    as_mri = F["mask_mri"]
    ovec = [fj.MRI(held(o, F)) if as_mri else held(o, F) for o in ov]
    fs = [vol_of(fj, x, F) for x in f]
    return fj.stream(ovec, f=fs, f_thresh=0.5, fa=vol_of(fj, values(SHAPE, 0.125, 0.03125), F), fa_thresh=0.25,
                     mask=mask_of(fj, INSIDE, F), seed=mask_of(fj, SEEDS, F), sublist=held(SUB, F), len_min=2, len_max=9, **kw)


def _bundles(fj, F):
    tr = tract_of(fj, F)
    b = fj.str_bundles(tr, _models(fj, F), 10.0, npoints=5)
    return tr, b


ODFS = values(SHAPE + (181,), 0.0, 0.0078125)                                    # one frame per half-sphere vertex of sphere_362

CASES = {
    "dti_fit": lambda fj, F: fj.dti_fit(dwi_of(fj, F), mask_of(fj, INSIDE, F)),
    "adc_fit": lambda fj, F: fj.adc_fit(dwi_of(fj, F), mask_of(fj, INSIDE, F)),
    "dki_fit": lambda fj, F: fj.dki_fit(dwi_of(fj, F), mask_of(fj, INSIDE, F), fj.sphere_362),
    "csd_rec": lambda fj, F: fj.csd_rec(dwi_of(fj, F), mask_of(fj, INSIDE, F), RESPONSE, fj.sphere_362, lmax=4),
    "gqi_rec": lambda fj, F: fj.gqi_rec(dwi_of(fj, F), mask_of(fj, INSIDE, F), fj.sphere_362),
    "dsi_rec": lambda fj, F: fj.dsi_rec(dwi_of(fj, F), mask_of(fj, INSIDE, F), fj.sphere_362, hann_width=16),
    "rumba_rec": lambda fj, F: fj.rumba_rec(dwi_of(fj, F), mask_of(fj, INSIDE, F), fj.sphere_362, niter=3),
    "find_peaks": lambda fj, F: fj.find_peaks(held(ODFS, F), fj.sphere_362),
    "find_peaks_work": lambda fj, F: fj.find_peaks_work(held(ODFS, F), fj.sphere_362),
    "dwi_denoise": lambda fj, F: fj.dwi_denoise(fj.MRI(held(DWI, F)) if F["mask_mri"] else held(DWI, F), mask_of(fj, INSIDE, F), patch=3),
    "dwi_denoise-no-mask": lambda fj, F: fj.dwi_denoise(fj.MRI(held(DWI, F)), None, patch=3),
    "st_eigen": lambda fj, F: fj.st_eigen(*[held(values(SHAPE, float(c)), F) for c in range(6)]),
    "st_recon": lambda fj, F: fj.st_recon(vol_of(fj, values(SHAPE), dict(F, mask_4d=False)), 1.0, 2.0),        # (an array is 3-D)
    "stream": lambda fj, F: _stream(fj, F),
    "stream-lcms": lambda fj, F: _stream(fj, F, lcms=fj.MRI(held(values(SHAPE + (10,), 0.0, 0.001953125), F)) if F["mask_mri"]
                                         else held(values(SHAPE + (10,), 0.0, 0.001953125), F), lcm_thresh=0.25, rng_seed=11),
    "prob_stream": lambda fj, F: fj.prob_stream(fj.MRI(held(ODFS, F)) if F["mask_mri"] else held(ODFS, F), fj.sphere_362,
                                                mask=mask_of(fj, INSIDE, F), seed=mask_of(fj, SEEDS, F), sublist=held(SUB, F),
                                                len_min=2, len_max=9, rng_seed=3),
    "xfm_apply": lambda fj, F: fj.xfm_apply(_xform(fj), held(PTS, F).reshape(-1) if F["flat"] else held(PTS, F)),
    "str_xform": lambda fj, F: fj.str_xform(_xform(fj), tract_of(fj, F)),
    "mri_xform": lambda fj, F: fj.mri_xform(_xform(fj), fj.MRI(held(DWI, F, widen=False))),
    "mri_xform-uint8": lambda fj, F: fj.mri_xform(_xform(fj), fj.MRI(held(np.arange(NVOX * 2).reshape(SHAPE + (2,)).astype(np.uint8), F)),
                                                  interp="nearest", outside=-1),
    "str_warp": lambda fj, F: fj.warp.str_warp(_warp(fj, F), tract_of(fj, F), outref=fj.MRI(np.zeros((2, 3, 2), np.float32))),
    "mri_warp": lambda fj, F: fj.warp.mri_warp(_warp(fj, F), fj.MRI(held(DWI, F, widen=False)), outref=fj.MRI(np.zeros((2, 3, 2), np.float32))),
    "mri_warp-int16": lambda fj, F: fj.warp.mri_warp(_warp(fj, F), fj.MRI(held((np.arange(NVOX) - 7).reshape(SHAPE).astype(np.int16), F)),
                                                     interp="nearest", outside=-2),
    "warp_invert": lambda fj, F: fj.warp.warp_invert(_warp(fj, F), fj.MRI(np.zeros((2, 3, 2), np.float32)), niter=4),
    "str_density": lambda fj, F: fj.str_density(tract_of(fj, F), "points"),
    "str_density-accumulate": lambda fj, F: fj.str_density(tract_of(fj, F), "lines", out=fj.str_density(tract_of(fj, F), "lines")),
    "str_sample": lambda fj, F: fj.str_sample(tract_of(fj, F), fj.MRI(held(DWI, F)), outside=float("nan")),
    "str_sample-two-volumes": lambda fj, F: fj.str_sample(tract_of(fj, F), [fj.MRI(held(DWI, F)), fj.MRI(held(values(SHAPE), F))]),
    "str_stats": lambda fj, F: fj.str_stats(tract_of(fj, F, scalars=held(values((7,)), F) if F["flat"] else held(values((7, 1)), F))),
    "str_select": lambda fj, F: fj.str_select(tract_of(fj, F), include=[mask_of(fj, INSIDE, F)], exclude=mask_of(fj, SEEDS, F, mri=False),
                                              end_in=[mask_of(fj, 1 - INSIDE, F), mask_of(fj, INSIDE, F)], min_npts=2),
    "str_connectome": lambda fj, F: fj.str_connectome(tract_of(fj, F), mask_of(fj, 3 * INSIDE + 2 * SEEDS, dict(
        F, mask_dtype=np.int32 if F["mask_dtype"] in (np.uint8, np.bool_) else F["mask_dtype"]))),
    "str_resample": lambda fj, F: fj.str_resample(tract_of(fj, F), 5, flip=[0, 1, 0] if F["f64"] else np.array([False, True, False])),
    "str_bundles": lambda fj, F: _bundles(fj, F),
    "str_centroids": lambda fj, F: fj.str_centroids(*_bundles(fj, F)),
    "str_profile": lambda fj, F: fj.str_profile(tract_of(fj, F), fj.MRI(held(DWI, F)), _models(fj, F), 10.0, npoints=5),
}


# ---------------------------------------------------------------------------------------------------------------------------------------
# (a) the record does not depend on how the caller held the data
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_the_record_does_not_depend_on_the_form_of_the_inputs(fj, rec, name):
    want = None
    for F in FORMS:
        del rec.calls[:]
        CASES[name](fj, F)
        got = rec.canon()
        assert got and all(n in TABLE for n, _ in got)
        if want is None:
            want = got
        assert [n for n, _ in got] == [n for n, _ in want], F
        for (n, g), (_, w) in zip(got, want):
            for key in w:
                assert g[key] == w[key], "%s: argument %r of %s differs for the form %s" % (name, key, n, F)


# ---------------------------------------------------------------------------------------------------------------------------------------
# (b) the bytes are the ones the ABI's layout says
# ---------------------------------------------------------------------------------------------------------------------------------------
def _sphere_bytes(odf):
    return xfast(odf.vertices, np.float32), xfast(odf.faces, np.int32)           # planar: every x, then every y, then every z


@pytest.mark.parametrize("name", ["dti_fit", "adc_fit", "dki_fit", "csd_rec", "gqi_rec", "dsi_rec", "rumba_rec"])
def test_a_fit_passes_the_volume_the_mask_and_the_tables_as_the_abi_reads_them(fj, rec, name):
    CASES[name](fj, BASE)
    a = rec.only("fib_" + name)
    assert (a["dev"], a["nx"], a["ny"], a["nz"], a["nvol"]) == (0,) + SHAPE + (NF,)
    assert a["vol"] == xfast(DWI, np.float32)                                    # x fastest, frame slowest
    assert a["mask"].code == 0 and a["mask"].raw == xfast(INSIDE, np.uint8)
    assert a["mdt"] == (0 if name == "rumba_rec" else ZEROED)                    # who declares its outputs freshly zeroed
    assert a["bval"] == BVAL.astype(np.float32).tobytes()
    if name != "adc_fit":
        assert a["bvec"] == xfast(BVEC.astype(np.float32), np.float32)           # planar [3][nvol]
    if name not in ("dti_fit", "adc_fit"):
        v, f = _sphere_bytes(fj.sphere_362)
        assert a["nv"] == 362 and a["v"] == v
        if name in ("csd_rec", "gqi_rec", "dsi_rec"):
            assert a["nf"] == 720 and a["f"] == f


@pytest.mark.parametrize("dtype, code, carried", [(np.int16, 2, np.int16), (np.float64, 7, np.float64), (np.bool_, 9, np.bool_),
                                                  (np.float16, 7, np.float64)])
def test_a_fit_and_the_tracer_pass_the_mask_in_its_own_element_type(fj, rec, dtype, code, carried):
    """the test of the mask is the library's; an element type the table lacks travels as float64"""
    F = dict(BASE, mask_dtype=dtype, mask_mri=False)
    CASES["dti_fit"](fj, F)
    CASES["stream"](fj, F)
    for a, flags in ((rec.only("fib_dti_fit"), ZEROED), (rec.only("fib_stream"), 0)):
        assert (a["mask"].code, a["mdt"]) == (code, flags)
        assert a["mask"].raw == xfast(INSIDE, carried)
    a = rec.only("fib_stream")
    assert (a["seed"].code, a["sdt"]) == (code, 0) and a["seed"].raw == xfast(SEEDS, carried)


def test_the_two_byte_mask_rules(fj, rec):
    """prob_stream keeps the voxels > 0, dwi_denoise and the regions of str_select those != 0; labels keep their values"""
    signed = np.where(INSIDE == 1, 2, -1).astype(np.int16)
    fj.prob_stream(fj.MRI(ODFS.astype(np.float32)), fj.sphere_362, mask=signed, seed=fj.MRI(signed), sublist=SUB)
    a = rec.only("fib_prob_stream")
    assert a["mask"] == a["seed"] == xfast(signed > 0, np.uint8)
    fj.dwi_denoise(fj.MRI(DWI), signed, patch=3)
    assert rec.only("fib_dwi_denoise")["mask"] == xfast(signed != 0, np.uint8)
    fj.dwi_denoise(fj.MRI(DWI), None, patch=3)
    assert rec.calls[-1][1]["mask"] == b"\1" * NVOX
    fj.str_select(tract_of(fj, BASE), include=[signed])
    assert rec.only("fib_str_select")["rois"] == (xfast(signed != 0, np.uint8),)
    fj.str_connectome(tract_of(fj, BASE), np.abs(signed).astype(np.float64), lengths=False)
    a = rec.only("fib_str_connectome")
    assert a["lab"] == xfast(np.abs(signed), np.int32) and a["remap"] == np.array([0, 1, 2], np.int32).tobytes()
    assert a["wmat"] is None and (a["L"], a["flags"]) == (2, 0)


def test_the_peak_finders_pass_planar_amplitudes_and_the_tessellation(fj, rec):
    v, f = _sphere_bytes(fj.sphere_362)
    for name in ("find_peaks", "find_peaks_work"):
        CASES[name](fj, BASE)
        a = rec.only("fib_" + name)
        assert (a["nvox"], a["nv"], a["nf"]) == (NVOX, 362, 720) and (a["v"], a["f"]) == (v, f)
        assert a["odf"] == rowwise(np.moveaxis(ODFS, -1, 0), np.float32)         # [nvert][nvox], the voxels in the order of odf.reshape(nvox, nvert)


def test_the_tracers_arguments(fj, rec):
    CASES["stream-lcms"](fj, BASE)
    a = rec.only("fib_stream_lcm")
    prm = dict(a["prm"])
    assert (prm["nx"], prm["ny"], prm["nz"], prm["nvec"], prm["len_min"], prm["len_max"]) == SHAPE + (2, 2, 9)
    assert (prm["search_dist"], prm["ws"], prm["interp"], prm["search_flat_axis"]) == (0, None, 0, 0)
    assert prm["cosang_thresh"] == struct.pack("<d", float(np.float32(np.cos(np.pi / 4))))
    ov = [values(SHAPE + (3,), -1.0, 0.03125), values(SHAPE + (3,), 2.0, 0.0625)]
    assert a["ov"] == tuple(xfast(o, np.float32) for o in ov)                    # [3][nvox] each
    assert a["f"] == (xfast(values(SHAPE, 0.25, 0.03125), np.float32), xfast(values(SHAPE, 0.5, 0.015625), np.float32))
    assert a["fa"] == xfast(values(SHAPE, 0.125, 0.03125), np.float32)
    assert a["mask"].raw == xfast(INSIDE, np.uint8) and a["seed"].raw == xfast(SEEDS, np.uint8)
    assert a["sub"] == rowwise(SUB, np.float32) and a["nsub"] == 2
    assert a["lcm"] == xfast(values(SHAPE + (10,), 0.0, 0.001953125), np.float32) and a["rng"] == 11
    assert (a["f_thresh"], a["fa_thresh"], a["lcm_thresh"]) == tuple(struct.pack("<d", v) for v in (0.5, 0.25, 0.25))
    fj.stream(fj.MRI(ov[0].astype(np.float32)), mask=INSIDE.astype(np.uint8), sublist=SUB)       # no f, fa or seed: null pointers
    a = rec.only("fib_stream")
    assert (a["f"], a["fa"], a["seed"].raw, a["sdt"]) == (None, None, None, 0) and dict(a["prm"])["len_max"] == 4


def test_prob_stream_passes_the_half_sphere_point_by_point(fj, rec):
    CASES["prob_stream"](fj, BASE)
    a = rec.only("fib_prob_stream")
    assert (a["nx"], a["ny"], a["nz"], a["nvert"], a["nsub"], a["len_min"], a["len_max"], a["rng"]) == SHAPE + (181, 2, 2, 9, 3)
    assert a["U"] == rowwise(fj.sphere_362.vertices[:181], np.float32)           # [nvert][3]: the first half of the vertices
    assert a["odf"] == xfast(ODFS, np.float32)
    assert a["mask"] == xfast(INSIDE, np.uint8) and a["seed"] == xfast(SEEDS, np.uint8) and a["sub"] == rowwise(SUB, np.float32)
    del rec.calls[:]
    U = fj.sphere_362.vertices[:5].astype(np.float64)                            # directions given as an array
    fj.prob_stream(ODFS[..., :5].astype(np.float32), np.asfortranarray(U), sublist=SUB)
    a = rec.only("fib_prob_stream")
    assert a["U"] == rowwise(U, np.float32) and (a["mask"], a["seed"]) == (None, None)


def test_the_line_tools_pass_packed_lines(fj, rec):
    xyz, npts = rowwise(PTS, np.float32), NPTS.astype(np.int32).tobytes()        # [npoints][3], int32 counts
    for name, entry in (("str_density", "fib_str_density"), ("str_stats", "fib_str_stats"), ("str_select", "fib_str_select"),
                        ("str_connectome", "fib_str_connectome"), ("str_resample", "fib_str_resample")):
        del rec.calls[:]
        CASES[name](fj, BASE)
        a = rec.only(entry)
        assert (a["xyz"], a["npts"], a["nl"], a["npnt"]) == (xyz, npts, 3, 7), name
        if "res" in a:
            assert a["res"] == np.array([1, 2, 3], np.float32).tobytes()
    del rec.calls[:]
    CASES["str_sample-two-volumes"](fj, BASE)
    a = rec.only("fib_str_sample")
    assert (a["xyz"], a["n"], a["nf"]) == (xyz, 7, NF + 1)
    assert a["vol"] == xfast(DWI, np.float32) + xfast(values(SHAPE), np.float32)                 # the frames of every volume, in order
    del rec.calls[:]
    CASES["str_warp"](fj, BASE)
    a = rec.only("fib_warp_points")
    assert (a["xyz"], a["n"]) == (xyz, 7) and a["disp"] == xfast(0.125 * values(SHAPE + (3,)), np.float32)
    del rec.calls[:]
    CASES["str_select"](fj, BASE)
    a = rec.only("fib_str_select")
    assert a["rois"] == tuple(xfast(r, np.uint8) for r in (INSIDE, SEEDS, 1 - INSIDE, INSIDE))
    assert (a["nroi"], a["m0"], a["m1"], a["m2"], a["m3"], a["min_npts"], a["max_npts"]) == (4, 1, 2, 12, 0, 2, 0)


def test_matrices_are_sixteen_floats_row_by_row(fj, rec):
    x = _xform(fj)
    CASES["xfm_apply"](fj, BASE)
    a = rec.only("fib_xfm_apply")
    assert a["M"] == rowwise(x.vox2vox, np.float32) and a["p"] == rowwise(PTS, np.float32) and a["n"] == 7
    CASES["mri_xform-uint8"](fj, BASE)
    a = rec.only("fib_vol_xform")
    assert a["M"] == rowwise(np.linalg.inv(x.vox2vox.astype(np.float64)), np.float32)            # output -> input
    assert a["vol"] == xfast(np.arange(NVOX * 2).reshape(SHAPE + (2,)), np.uint32)               # 8-bit elements widened to words
    assert (a["nxi"], a["nyi"], a["nzi"], a["nf"], a["code"], a["nxo"], a["nyo"], a["nzo"]) == SHAPE + (2, 0, 2, 3, 2)
    assert a["bits"] == 255                                                      # -1 as uint8, then as the 32-bit word
    CASES["mri_warp-int16"](fj, BASE)
    a = rec.only("fib_warp_volume")
    assert a["vol"] == xfast((np.arange(NVOX) - 7).reshape(SHAPE), np.int32) and a["bits"] == -2
    w = _warp(fj, BASE)
    assert a["A"] == rowwise(w.vox2ras, np.float32)                              # the field's own grid is filled: to_field = I
    assert a["Q"] == a["B"] == rowwise(np.eye(4), np.float32)
    CASES["mri_warp"](fj, BASE)                                                  # onto a grid whose vox2ras is I
    assert rec.calls[-1][1]["Q"] == rowwise(np.linalg.inv(w.vox2ras.astype(np.float64)), np.float32)


def test_results_carry_the_element_type_and_geometry_of_their_inputs(fj, rec):
    out = CASES["mri_xform-uint8"](fj, BASE)
    assert out.vol.dtype == np.uint8 and out.vol.shape == (2, 3, 2, 2) and out.vol.flags.f_contiguous and out.volres == (2.0, 1.0, 3.0)
    src = fj.MRI((np.arange(NVOX) - 7).reshape(SHAPE).astype(np.int16), tr=2.5)
    out = fj.warp.mri_warp(_warp(fj, BASE), src, interp="nearest")
    assert out.vol.dtype == np.int16 and out.vol.shape == SHAPE + (1,) and out.tr == 2.5
    # a voxel fit's outputs: the geometry of the mask when it is an MRI, else the DWI's
    dwi, m = dwi_of(fj, BASE), fj.MRI(INSIDE.astype(np.uint8), volres=(2.0, 3.0, 4.0))
    dwi.volres = (0.5, 0.5, 0.5)
    for fit in (lambda mask: fj.dti_fit(dwi, mask).fa, lambda mask: fj.adc_fit(dwi, mask)[0], lambda mask: fj.dki_fit(dwi, mask).kt,
                lambda mask: fj.csd_rec(dwi, mask, RESPONSE, lmax=2).sh, lambda mask: fj.gqi_rec(dwi, mask).qa[2],
                lambda mask: fj.dsi_rec(dwi, mask).pdf, lambda mask: fj.rumba_rec(dwi, mask, niter=1).peak[4]):
        assert fit(m).volres == (2.0, 3.0, 4.0) and fit(m.vol[..., 0]).volres == (0.5, 0.5, 0.5)
    assert fj.dki_fit(dwi, m).kt.vol.shape == SHAPE + (15,) and fj.csd_rec(dwi, m, RESPONSE, lmax=2).sh.vol.shape == SHAPE + (6,)
    assert fj.dsi_rec(dwi, m).pdf.vol.shape == SHAPE + (NF,) and fj.gqi_rec(dwi, m).odf.vol.shape == SHAPE + (321,)
    # a tracking result: no lines, the geometry of the mask
    tr = fj.stream(fj.MRI(values(SHAPE + (3,)).astype(np.float32)), mask=m, sublist=SUB)
    assert tr.nstr == 0 and tr.xyz.shape == (0, 3) and tr.seed_index.shape == (0,) and tr.volres == (2.0, 3.0, 4.0) and tr.scalars is None
    tr = fj.prob_stream(ODFS[..., :5].astype(np.float32), fj.sphere_362.vertices[:5], mask=m, sublist=SUB)
    assert tr.nstr == 0 and tr.xyz.shape == (0, 3) and tr.volres == (2.0, 3.0, 4.0)
