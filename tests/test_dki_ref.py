"""CPU tests (no GPU) of the DKI definition: tests/dki_ref.py against known answers in float64, the library's host-side tables
(fib_dki_design) against NumPy's float64 pinv, the refusal of schemes that do not determine the 22 unknowns, the layout of the two new
structs, and the per-voxel rule (clamp, skip, clips, floor) by hand."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import dki_ref as K
import dti_ref as DR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-10
AXES4 = np.array([[0, 0, 1], [1, 0, 0], [0, 0, -1], [-1, 0, 0]], np.float32)       # a "tessellation" of two directions: z and x


def _sphere(fj, name="sphere_642"):
    return getattr(fj, name).vertices


def _rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(b).max()


def _random_v(n, rng, w=2e-7, spread=0.3):
    """kurtosis tensors near the isotropic one (V(n) = w = 0.8 * (0.5e-3)^2): [n, 15] in mm^4/s^2"""
    return K.isotropic_v(w)[None] * (1.0 + spread * rng.uniform(-1, 1, (n, 15))) + spread * w / 6 * rng.uniform(-1, 1, (n, 15))


# ------------------------------------------------------------------------------------------------------------------------------
# known answers, float64
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nvol", [22, 61, 270])
def test_noise_free_signal_returns_its_tensors(fj, nvol):
    bval, bvec = K.scheme(nvol)
    rng = np.random.default_rng(nvol)
    d6 = DR.random_tensors(DR.CLASSES["generic"], 64, rng)
    v15 = _random_v(64, rng)
    s0 = rng.uniform(800, 1200, 64)
    ref = K.dki_fit_ref(K.model_signal(bval, bvec, d6, v15, s0), np.ones(64), bval, bvec, _sphere(fj))
    assert _rel(ref["d"][:, :6], d6) < TOL and _rel(ref["d"][:, 6:21], v15) < TOL and _rel(ref["s0"], s0) < TOL
    md = d6[:, [0, 3, 5]].mean(1)
    assert _rel(ref["md"], md) < TOL and _rel(ref["kt"], v15 / md[:, None] ** 2) < TOL
    # mk against the definition written out directly: the mean of V(n) / D(n)^2 over the half sphere (no clip is active here)
    v = _sphere(fj)[:321].astype(np.float64)
    rows = K.dir_rows(v)
    k = (v15 @ rows[:, 6:].T) / (d6 @ rows[:, :6].T) ** 2
    assert k.min() > -3 / 7 and k.max() < 10
    assert np.abs(ref["mk"] - k.mean(1)).max() < TOL


def _dyadic_scheme(seed=5):
    """a b0 and 30 directions with components k / 4 on each of b = 1000 and 2000 (not unit vectors: the model is algebraic in g):
    every entry b * g_i * g_j of the Float32 DTI design is exact, so dti_ref and dki_ref see the same tensor signal"""
    rng = np.random.default_rng(seed)
    seen, g = set(), []
    while len(g) < 30:
        v = rng.integers(-4, 5, 3)
        key = tuple(v) if tuple(v) > tuple(-v) else tuple(-v)
        if np.abs(v).sum() >= 3 and key not in seen:
            seen.add(key)
            g.append(v / 4.0)
    g = np.array(g)
    bval = np.concatenate([[0.0], np.full(30, 1000.0), np.full(30, 2000.0)]).astype(np.float32)
    return bval, np.vstack([np.zeros((1, 3)), g, g]).astype(np.float32)


def test_zero_kurtosis_is_the_tensor_fit(fj):
    bval, bvec = _dyadic_scheme()
    rng = np.random.default_rng(1)
    d6 = DR.random_tensors(DR.CLASSES["generic"], 48, rng)
    s = K.model_signal(bval, bvec, d6, np.zeros((48, 15)), rng.uniform(800, 1200, 48))
    ref = K.dki_fit_ref(s, np.ones(48), bval, bvec, _sphere(fj))
    dti = DR.dti_fit_ref(s, np.ones(48), bval, bvec)
    for k in ("mk", "ak", "rk"):
        assert np.abs(ref[k]).max() < TOL, k
    assert np.abs(ref["kt"]).max() < TOL
    for k in ("eigval1", "eigval2", "eigval3", "rd", "md"):                              # in units of eigval1
        assert (np.abs(ref[k] - dti[k]) / dti["eigval1"]).max() < TOL, k
    assert _rel(ref["s0"], dti["s0"]) < TOL and np.abs(ref["fa"] - dti["fa"]).max() < TOL
    for k in ("eigvec1", "eigvec2", "eigvec3"):
        assert (1.0 - np.abs((ref[k] * dti[k]).sum(-1))).max() < TOL, k


def test_isotropic_tensor_with_isotropic_kurtosis(fj):
    bval, bvec = K.scheme(61)
    md, w = 1.1e-3, 0.9 * 1.1e-3 ** 2
    d6 = np.tile(np.array([md, 0, 0, md, 0, md]), (4, 1))
    s = K.model_signal(bval, bvec, d6, np.tile(K.isotropic_v(w), (4, 1)), [1.0, 50.0, 1e3, 1e6])
    for name in ("sphere_362", "sphere_642", "sphere_724"):
        ref = K.dki_fit_ref(s, np.ones(4), bval, bvec, _sphere(fj, name))
        for k in ("mk", "ak", "rk"):                                                  # (whatever eigh returns for the eigenvectors)
            assert np.abs(ref[k] - w / md ** 2).max() < TOL * 0.9, (name, k)
    # and K(n) is the same in any direction at all
    n = np.random.default_rng(2).normal(size=(50, 3))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    k = K.kurtosis(K.dir_rows(n), ref["d"], K.DEFAULTS, np.float64)
    assert np.abs(k - w / md ** 2).max() < TOL * 0.9


def test_radial_quadrature_does_not_depend_on_the_starting_angle(fj):
    """D(phi) = a + b cos(2 phi) in the plane of eigvec2 and eigvec3, so the Fourier coefficients of V / D^2 fall off like r^k with
    r = (a - sqrt(a^2 - b^2)) / b and 16 points on the half circle alias harmonic 14 and above.  For eigenvalues (0.5, 0.3)e-3 r is
    0.127 and r^14 is 3e-13: rotating the samples by half their spacing must not move rk by 1e-10.  (At (0.9, 0.3)e-3 it is 1e-8.)"""
    bval, bvec = K.scheme(61)
    rng = np.random.default_rng(3)
    d6 = DR.random_tensors((1.7e-3, 0.5e-3, 0.3e-3), 32, rng)
    s = K.model_signal(bval, bvec, d6, _random_v(32, rng), 1000.0)
    a = K.dki_fit_ref(s, np.ones(32), bval, bvec, _sphere(fj))
    b = K.dki_fit_ref(s, np.ones(32), bval, bvec, _sphere(fj), phi0=np.pi / 32)
    assert np.abs(a["rk"]).min() > 0.05 and np.abs(a["rk"] - b["rk"]).max() < TOL
    assert np.abs(a["rk"] - a["ak"]).max() > 1e-3                                      # (a test that could fail)


# ------------------------------------------------------------------------------------------------------------------------------
# the library's tables (host only)
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nvol", [22, 61, 270])
def test_design_tables_against_float64_pinv(fj, nvol):
    bval, bvec = K.scheme(nvol)
    A, pA, rank = fj.dki_design(bval, bvec)
    assert rank == 22
    assert np.array_equal(A, K.design(bval, bvec).astype(np.float32))
    P64, r64 = K.pinv_scaled(bval, bvec)
    assert r64 == 22
    P32 = P64.astype(np.float32)
    bound = np.spacing(np.abs(P32)) + 1e-10 * np.abs(P64).max(1, keepdims=True)
    assert (np.abs(pA.astype(np.float64) - P32) <= bound).all(), (np.abs(pA - P32) / bound).max()
    # the scaling is what keeps the design away from pinv's cut-off: in s/mm^2 the same scheme loses a dimension
    sv = np.linalg.svd(K.design(bval, bvec) / K.ROW_SCALE[None], compute_uv=False)
    assert (sv > K.EPS32 * 22 * sv.max()).sum() < 22


def _refused(fj, bval, bvec):
    with pytest.raises(fj.FibersError) as e:
        fj.dki_design(bval, bvec)
    assert e.value.code == -1 and "b ~ 0" in e.value.message and "two non-zero shells" in e.value.message, e.value.message
    L = fj.lib()
    rank = C.c_int(-1)
    bv = np.asfortranarray(bvec, np.float32)
    bl = np.ascontiguousarray(bval, np.float32)
    assert L.fib_dki_design(bl.ctypes.data, bv.ctypes.data, len(bl), None, None, C.byref(rank)) == -1
    return rank.value


def test_schemes_that_do_not_determine_the_fit_are_refused(fj):
    from fibers_jl_amd import phantom
    assert _refused(fj, *phantom.scheme_dti(30, 1, 1000.0, 3)) == 16                   # a single shell with a b0
    bval, bvec = K.shells_scheme(1, (30, 30), (1000.0, 2000.0), 3)
    assert _refused(fj, bval[1:], bvec[1:]) == 21                                      # two shells, no b ~ 0 frame
    dirs = phantom.sphere_dirs(14, 3)
    bval = np.concatenate([[0.0], np.full(28, 1000.0), np.full(28, 2000.0)]).astype(np.float32)
    bvec = np.vstack([np.zeros((1, 3), np.float32), dirs, -dirs, dirs, -dirs])
    assert _refused(fj, bval, bvec) < 22                                               # 14 distinct directions
    bval, bvec = K.scheme(22)
    assert _refused(fj, bval[:21], bvec[:21]) <= 21                                    # nvol < 22
    L = fj.lib()
    assert L.fib_dki_design(None, None, 0, None, None, None) == -4 and b"Missing b-value table" in L.fib_last_error()
    assert L.fib_dki_design(bval.ctypes.data, None, 22, None, None, None) == -5 and b"Missing gradient table" in L.fib_last_error()


def test_python_surface_raises_the_reference_error_strings(fj):
    dwi = fj.MRI(np.ones((2, 2, 2, 22), np.float32))
    m = fj.MRI(np.ones((2, 2, 2), np.uint8))
    with pytest.raises(RuntimeError, match="Missing b-value table from input DWI structure"):
        fj.dki_fit(dwi, m)
    dwi.bval = np.ones(22, np.float32)
    with pytest.raises(RuntimeError, match="Missing gradient table from input DWI structure"):
        fj.dki_fit(dwi, m)
    assert [f for f in fj.DKI.__dataclass_fields__][:10] == [f for f in fj.DTI.__dataclass_fields__]
    assert [f for f in fj.DKI.__dataclass_fields__][10:] == ["mk", "ak", "rk", "kt"]


def test_layouts_of_the_dki_structs_match_the_bindings(tmp_path):
    """the method of test_abi.test_struct_layouts_of_the_header_match_the_bindings for fib_dki_params and fib_dki_out"""
    from fibers_jl_amd import _lib
    fields = {"fib_dki_params": ["min_signal", "min_diffusivity", "min_kurtosis", "max_kurtosis"],
              "fib_dki_out": ["s0", "eigval1", "eigval2", "eigval3", "eigvec1", "eigvec2", "eigvec3", "rd", "md", "fa", "mk", "ak", "rk", "kt"]}
    mirrors = {"fib_dki_params": _lib.DkiParams, "fib_dki_out": _lib.DkiOut}
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "fibers_hip.h"', 'int main(void) {']
    for st, fl in fields.items():
        src.append('  printf("%s sizeof %%zu\\n", sizeof(%s));' % (st, st))
        for f in fl:
            src.append('  printf("%s %s %%zu\\n", offsetof(%s, %s));' % (st, f, st, f))
    src += ['  return 0;', '}']
    cfile = tmp_path / "layout.c"
    cfile.write_text("\n".join(src))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(cfile), "-o", str(exe)])
    got = {}
    for ln in subprocess.check_output([str(exe)], text=True).splitlines():
        st, f, v = ln.split()
        got[(st, f)] = int(v)
    jl = open(os.path.join(ROOT, "julia", "FibersHIP.jl")).read()
    for st, fl in fields.items():
        m = mirrors[st]
        assert C.sizeof(m) == got[(st, "sizeof")], (st, C.sizeof(m), got[(st, "sizeof")])
        assert [n for n, _ in m._fields_] == fl
        for f in fl:
            assert getattr(m, f).offset == got[(st, f)], (st, f)
        want = "# layout: %s sizeof %d: %s" % (st, got[(st, "sizeof")], " ".join("%s@%d" % (f, got[(st, f)]) for f in fl))
        assert want in jl, "julia/FibersHIP.jl lacks or misstates: " + want
    assert list(_lib.DkiOut._fields_[:10]) == list(_lib.DtiOut._fields_)


# ------------------------------------------------------------------------------------------------------------------------------
# the per-voxel rule by hand
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_clamp_and_skip_rule(fj, dtype):
    bval, bvec = K.scheme(22)
    rng = np.random.default_rng(4)
    base = K.compartment_signal(bval, bvec, DR.CLASSES["generic"], 1, rng, 1000.0)[0]
    s = np.tile(base, (7, 1))
    s[0, [3, 7, 12]] = (0.0, -5.0, 1e-6)                 # clamped to min_signal
    s[1, [3, 7, 12]] = 1e-4                              # ... which is this voxel
    s[2, 5] = np.nan                                     # skipped
    s[3, 5] = np.inf                                     # solved; nothing is trapped
    s[4] = -np.abs(base)                                 # nothing positive: skipped
    s[4, 2] = 0.0
    s[5, 1:] = -1.0                                      # one positive sample is enough to be solved (21 samples clamped)
    mask = np.ones(7, np.uint8)
    mask[6] = 0
    ref = K.dki_fit_ref(s, mask, bval, bvec, _sphere(fj), dtype=dtype)
    assert ref["branch"].tolist() == [DR.FULL, DR.FULL, DR.ZEROS, DR.FULL, DR.ZEROS, DR.FULL, DR.OUTSIDE]
    for k in K.FIELDS + ("d",):
        assert ref[k].dtype == dtype, k
        assert np.array_equal(ref[k][0], ref[k][1]), k
        assert (ref[k][[2, 4, 6]] == 0).all(), k
    assert np.isfinite(ref["mk"][[0, 5]]).all() and not np.isfinite(ref["d"][3]).all()
    # voxel 5 by hand: log of (s0, 1e-4, 1e-4, ...) through the pseudo-inverse
    pA, _ = K.pinv_scaled(bval, bvec)
    logs = np.log(np.where(s[5] < np.float32(1e-4), np.float32(1e-4), s[5]).astype(np.float64))
    assert np.abs(ref["d"][5] - pA @ logs).max() <= (1e-12 if dtype is np.float64 else 1e-3) * np.abs(pA @ logs).max()
    # a larger min_signal moves the clamp
    ref2 = K.dki_fit_ref(s[:1], mask[:1], bval, bvec, _sphere(fj), dtype=dtype, min_signal=1.0)
    s1 = s[:1].copy()
    s1[0, [3, 7, 12]] = 1.0
    ref3 = K.dki_fit_ref(s1, mask[:1], bval, bvec, _sphere(fj), dtype=dtype)
    assert np.array_equal(ref2["d"], ref3["d"]) and not np.array_equal(ref2["d"][0], ref["d"][0])


def test_clips_by_hand():
    """V(n) = wx x^4 + wy y^4 on an isotropic tensor: K = 40 along x and -4 along y.  Over a fan of directions in the xy plane
    mk must be the mean of the clipped values, and with min_kurtosis >= max_kurtosis of the unclipped ones."""
    bval, bvec = K.scheme(61)
    md = 1e-3
    v15 = np.zeros((1, 15))
    v15[0, 0], v15[0, 1] = 40 * md ** 2, -4 * md ** 2
    s = K.model_signal(bval, bvec, [[md, 0, 0, md, 0, md]], v15, 100.0)
    th = np.pi * np.arange(24) / 24
    half = np.stack([np.cos(th), np.sin(th), 0 * th], 1)
    verts = np.vstack([half, -half]).astype(np.float32)
    h = verts[:24].astype(np.float64)
    raw = (40 * h[:, 0] ** 4 - 4 * h[:, 1] ** 4) / (h ** 2).sum(1) ** 2               # (the float32 vertices are unit vectors to 6e-8)
    assert (raw > 10).sum() >= 3 and (raw < -3 / 7).sum() >= 3 and ((raw > -3 / 7) & (raw < 10)).sum() >= 3
    ref = K.dki_fit_ref(s, [1], bval, bvec, verts)
    lo, hi = float(np.float32(-3 / 7)), 10.0
    assert abs(ref["mk"][0] - np.clip(raw, lo, hi).mean()) < 1e-9
    for lim in ((1.0, 1.0), (2.0, -2.0)):
        ref = K.dki_fit_ref(s, [1], bval, bvec, verts, min_kurtosis=lim[0], max_kurtosis=lim[1])
        assert abs(ref["mk"][0] - raw.mean()) < 1e-9
    ref = K.dki_fit_ref(s, [1], bval, bvec, verts, min_kurtosis=-1.0, max_kurtosis=3.0)
    assert abs(ref["mk"][0] - np.clip(raw, -1.0, 3.0).mean()) < 1e-9
    # NaN passes through both comparisons
    k = K.kurtosis(np.ones((1, 21)), np.full((1, 22), np.nan), K.DEFAULTS, np.float64)
    assert np.isnan(k).all()


def test_diffusivity_floor_by_hand():
    """D = diag(1e-3, 1e-3, 1e-8): along z D(n) is below min_diffusivity = 1e-6 and K(z) = V_zzzz / (1e-6)^2, not / (1e-8)^2"""
    bval, bvec = K.scheme(61)
    v15 = np.zeros((1, 15))
    v15[0, 2], v15[0, 0] = 1e-13, 2e-7
    s = K.model_signal(bval, bvec, [[1e-3, 0, 0, 1e-3, 0, 1e-8]], v15, 100.0)
    ref = K.dki_fit_ref(s, [1], bval, bvec, AXES4)
    floor = float(np.float32(1e-6))
    kz, kx = 1e-13 / floor ** 2, 2e-7 / 1e-6
    assert abs(ref["mk"][0] - 0.5 * (kz + kx)) < 1e-6 * kz
    ref = K.dki_fit_ref(s, [1], bval, bvec, AXES4, min_diffusivity=1e-9, max_kurtosis=1e6)
    assert abs(ref["mk"][0] - 0.5 * (1e-13 / 1e-16 + kx)) < 1e-3 * 1e3
