"""CPU tests (no GPU) of the restatement of dwi_degibbs (tests/degibbs_ref.py): its two routes agree, pick the same candidate in every
pixel and leave a gap that makes the GPU test's rule exclusion-free; the properties the definition promises; the host-only entries of
the library (the refusals, the circulant table)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import degibbs_ref as ref  # noqa: E402

CASES = pytest.mark.parametrize("case", ref.CASES, ids=ref.case_id)
PHANTOMS = pytest.mark.parametrize("case", ref.PHANTOMS, ids=ref.case_id)


@CASES
def test_the_two_routes_agree(case):
    """d and e_t, the figures DESIGN.md §5 quotes: with samples of amplitude 1000 both are rounding of float64 sums of up to 256 terms"""
    r = ref.case_reference(case)
    print("%s: d = %.3g, e_t = %.3g" % (ref.case_id(case), r["d"], r["e_t"]))
    assert r["d"] <= 1e-10 and r["e_t"] <= 1e-9
    assert r["same_pick"], "the routes pick different candidates"


@CASES
def test_the_smallest_gap_exceeds_64_e_t(case):
    """second smallest minus smallest t_j[l] in every pixel: the GPU test leaves no pixel out"""
    r = ref.case_reference(case)
    gap = min(r["gap_u"].min(), r["gap_v"].min())
    print("%s: smallest gap %.3g, 64 e_t = %.3g" % (ref.case_id(case), gap, 64 * r["e_t"]))
    assert gap > 64 * r["e_t"]


@CASES
def test_the_filter_splits_the_slice(case):
    """au + av == a up to d, but for the corner bin's term when both sizes are even"""
    vol, axis = ref.case_volume(case), case[2]
    r = ref.case_reference(case)
    a = np.take(vol[..., 0], 0, axis=axis).astype(np.float64)
    nu, nv = a.shape
    for filt in (ref.filter_a, ref.filter_b):
        au, av = filt(a)
        want = a.copy()
        if nu % 2 == 0 and nv % 2 == 0:
            sign = (-1.0) ** (np.arange(nu)[:, None] + np.arange(nv)[None, :])
            want -= (a * sign).sum() / (nu * nv) * sign
        assert np.abs(au + av - want).max() <= max(r["d"], 1e-12)


@PHANTOMS
def test_the_total_variation_falls(case):
    vol, axis = ref.case_volume(case), case[2]
    out = ref.case_reference(case)["out"]
    assert ref.total_variation(out, axis) < ref.total_variation(vol, axis)


def test_zero_and_constant_slices():
    for shape, axis in (((9, 10, 2), 2), ((16, 16, 1), 2), ((9, 12, 10), 0)):
        z = ref.degibbs(np.zeros(shape + (1,), np.float32), axis)
        assert not z["out"].any() and not z["ju"].any() and not z["jv"].any()
        assert not np.signbit(z["out"]).any()
        c = ref.degibbs(np.full(shape + (1,), 417.25, np.float32), axis)
        d = ref.case_reference(ref.CASES[3])["d"]
        assert np.abs(c["out"] - 417.25).max() <= d


def test_shift_zero_returns_the_row():
    """where j* = 0 the output is r[l] itself, bit for bit"""
    r = np.random.default_rng(5).normal(0, 1, (3, 11))
    out, js, _ = ref.unring(r, 4, 1, 3, ref.candidates_a)
    assert np.array_equal(out[js == 0], r[js == 0])


# ---- the library's host-only entries -------------------------------------------------------------------------------------------------
def test_check_gives_every_refusal(fj):
    from fibers_jl_amd import degibbs
    degibbs.dwi_degibbs_check((9, 9, 2), 1)
    degibbs.dwi_degibbs_check((ref.LIMIT, 9, 1), 1)
    degibbs.dwi_degibbs_check((15, 15, 2), 3, min_w=2, max_w=6)
    degibbs.dwi_degibbs_check((3, 9, 12), 2, slice_axis=0)               # the slice axis itself may be short
    invalid = [dict(shape=(8, 9, 2)), dict(shape=(9, 8, 2)), dict(shape=(9, 2, 9)), dict(shape=(15, 14, 2), min_w=2, max_w=6),
               dict(shape=(9, 9, 8), slice_axis=1), dict(shape=(9, 8, 9), slice_axis=0), dict(shape=(9, 12, 5), slice_axis=0),
               dict(shape=(9, 12, 5), slice_axis=1),
               dict(shape=(9, 9, 2), nshifts=0), dict(shape=(9, 9, 2), nshifts=33), dict(shape=(20, 20, 2), min_w=0),
               dict(shape=(20, 20, 2), min_w=3, max_w=2), dict(shape=(20, 20, 2), max_w=7), dict(shape=(9, 9, 2), slice_axis=3),
               dict(shape=(9, 9, 2), slice_axis=-1), dict(shape=(9, 9, 0)), dict(shape=(9, 9, 2), nframes=0)]
    for kw in invalid:
        kw = dict(kw)
        with pytest.raises(fj.FibersError) as e:
            degibbs.dwi_degibbs_check(kw.pop("shape"), kw.pop("nframes", 1), **kw)
        assert e.value.code == -1, kw
    for shape, axis in (((ref.LIMIT + 1, 9, 1), 2), ((9, ref.LIMIT + 1, 1), 2), ((2, 9, ref.LIMIT + 1), 0)):
        with pytest.raises(fj.FibersError) as e:
            degibbs.dwi_degibbs_check(shape, 1, slice_axis=axis)
        assert e.value.code == -7 and str(ref.LIMIT) in str(e.value)
    assert fj.lib().fib_dwi_degibbs_check(9, 9, 2, 1, None) == 0         # NULL: the default parameters
    assert degibbs.MAX_SIZE == ref.LIMIT


@pytest.mark.parametrize("n, K", [(5, 1), (9, 20), (16, 20), (65, 32), (140, 20), (ref.LIMIT, 20), (ref.LIMIT - 1, 32)])
def test_the_table_builder_against_route_b(fj, n, K):
    """fib_degibbs_table (setup.cpp; extended precision, rounded once) against route B's float64 cosine sum: 2^-50 relative to the
    table's largest entry, which is of order 1 (near the zeros of D a bound relative to the entry itself would hold no table)"""
    from fibers_jl_amd import degibbs
    got, want = degibbs.degibbs_table(n, K), ref.table_b(n, K)
    assert got.shape == want.shape == (2 * K, n)
    print("n = %d, K = %d: %.3g of 2^-50 max|D|" % (n, K, np.abs(got - want).max() / (2.0 ** -50 * np.abs(want).max())))
    assert np.abs(got - want).max() <= 2.0 ** -50 * np.abs(want).max()
    assert fj.lib().fib_degibbs_table(ref.LIMIT + 1, K, got.ctypes.data) == -1
    assert fj.lib().fib_degibbs_table(n, 33, got.ctypes.data) == -1


def test_the_bindings_state_the_params_layout(tmp_path):
    """fib_degibbs_params as the header, the ctypes mirror and the comment of julia/FibersHIP.jl state it"""
    import subprocess
    from fibers_jl_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    fields = ["slice_axis", "nshifts", "minW", "maxW"]
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "fibers_hip.h"', 'int main(void) {',
           '  fib_degibbs_params d = FIB_DEGIBBS_PARAMS_DEFAULT;',
           '  printf("%zu %d %d %d %d\\n", sizeof(fib_degibbs_params), d.slice_axis, d.nshifts, d.minW, d.maxW);']
    src += ['  printf("%%zu\\n", offsetof(fib_degibbs_params, %s));' % f for f in fields] + ['  return 0;', '}']
    (tmp_path / "l.c").write_text("\n".join(src))
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(root, "include"), str(tmp_path / "l.c"), "-o", str(tmp_path / "l")])
    lines = subprocess.check_output([str(tmp_path / "l")], text=True).split("\n")
    assert lines[0] == "16 2 20 1 3"                                     # the default initialiser
    offs = [int(v) for v in lines[1:5]]
    assert C.sizeof(_lib.DegibbsParams) == 16 and [n for n, _ in _lib.DegibbsParams._fields_] == fields
    assert [getattr(_lib.DegibbsParams, f).offset for f in fields] == offs
    want = "# layout: fib_degibbs_params sizeof 16: " + " ".join("%s@%d" % (f, o) for f, o in zip(fields, offs))
    assert want in open(os.path.join(root, "julia", "FibersHIP.jl")).read()
