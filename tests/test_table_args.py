"""One normalisation of the b-table in Python (fibers.jl_amd/dti.py `_table_args`): the bytes the C ABI reads do not depend on how the
caller held the table, and a gradient table whose row count is not nvol is refused before the library is reached (the C side would read
past its end).  No GPU: `_lib.lib` is patched so that reaching the library at all fails the test."""
import numpy as np
import pytest

SENTENCE = r"gradient table must be \[7 x 3\], got \(6, 3\)"


def _table(n=7):
    rng = np.random.default_rng(5)
    g = rng.standard_normal((n, 3))
    g /= np.linalg.norm(g, axis=1, keepdims=True)
    return np.concatenate([[0.0], np.full(n - 1, 1000.0)]), g


def test_table_args_gives_the_same_bytes_for_every_input_form():
    from fibers_jl_amd._host import table_args as _table_args
    bval, g = _table()
    g32 = g.astype(np.float32)
    forms = [(bval.tolist(), g.tolist()),
             (np.ascontiguousarray(bval, np.float64), np.ascontiguousarray(g, np.float64)),
             (np.asfortranarray(bval.astype(np.float32)), np.asfortranarray(g32))]
    want_b, want_g = bval.astype(np.float32).tobytes(), g32.tobytes(order="F")
    for b, v in forms:
        ob, ov = _table_args(b, v)
        assert ob.dtype == np.float32 and ob.ndim == 1 and ob.flags.c_contiguous
        assert ov.dtype == np.float32 and ov.shape == (7, 3) and ov.flags.f_contiguous
        assert ob.tobytes() == want_b
        assert ov.tobytes(order="A") == want_g            # memory order: x column, y column, z column
        assert np.array_equal(ov, g32)
    ob, ov = _table_args(bval, None, need_bvec=False)
    assert ov is None and ob.tobytes() == want_b


PLANS = {
    "DtiPlan": lambda fj, b, g: fj.DtiPlan(b, g),
    "OdfPlan-gqi": lambda fj, b, g: fj.OdfPlan("gqi", b, g),
    "OdfPlan-dsi": lambda fj, b, g: fj.OdfPlan("dsi", b, g),
    "RumbaPlan": lambda fj, b, g: fj.RumbaPlan(b, g),
    "DkiPlan": lambda fj, b, g: fj.DkiPlan(b, g),
    "CsdPlan": lambda fj, b, g: fj.CsdPlan(b, g, (1.7e-3, 0.2e-3, 1.0)),
    "dki_design": lambda fj, b, g: fj.dki_design(b, g),
    "csd_design": lambda fj, b, g: fj.csd_design(b, g, (1.7e-3, 0.2e-3, 1.0)),
}


@pytest.mark.parametrize("name", sorted(PLANS))
def test_a_short_gradient_table_is_refused_before_the_library_is_reached(fj, monkeypatch, name):
    from fibers_jl_amd import _lib
    monkeypatch.setattr(_lib, "lib", lambda: pytest.fail("%s reached the library with a 6-row gradient table" % name))
    bval, g = _table()
    with pytest.raises(ValueError, match=SENTENCE):
        PLANS[name](fj, bval, g[:6])
