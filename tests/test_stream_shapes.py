"""stream() reads every orientation, amplitude and fa volume as the nx * ny * nz voxels of ovec[0]: a volume of another shape is a
ValueError that names the argument and both shapes, before the threshold warnings look at it and before the library is reached (it
would read past the volume's end).  No GPU: `_lib.lib` is patched so that reaching the library at all fails the test."""
import numpy as np
import pytest

SHAPE, OTHER = (3, 2, 4), (3, 2, 3)


def _vol(shape, frames=None):
    n = int(np.prod(shape)) * (frames or 1)
    return (0.25 + np.arange(n, dtype=np.float32) / n).reshape(shape + ((frames,) if frames else ()))


CASES = {
    "ovec[1]": lambda fj, bad: dict(ovec=[fj.MRI(_vol(SHAPE, 3)), bad(3)]),
    "f[1]": lambda fj, bad: dict(ovec=[fj.MRI(_vol(SHAPE, 3)), _vol(SHAPE, 3)], f=[_vol(SHAPE), bad()]),
    "f[0]": lambda fj, bad: dict(ovec=_vol(SHAPE, 3), f=bad()),
    "fa": lambda fj, bad: dict(ovec=_vol(SHAPE, 3), fa=bad()),
}


@pytest.mark.parametrize("as_mri", [False, True])
@pytest.mark.parametrize("name", sorted(CASES))
def test_stream_refuses_a_volume_of_another_shape_before_the_library_is_reached(fj, monkeypatch, capsys, name, as_mri):
    from fibers_jl_amd import _lib
    monkeypatch.setattr(_lib, "lib", lambda: pytest.fail("stream reached the library with a %s of another shape" % name))
    bad = lambda frames=None: fj.MRI(_vol(OTHER, frames)) if as_mri else _vol(OTHER, frames)          # noqa: E731
    kw = CASES[name](fj, bad)
    with pytest.raises(ValueError, match=r"%s shape \(3, 2, 3\) does not match the orientation volume \(3, 2, 4\)" % name.replace("[", r"\[").replace("]", r"\]")):
        fj.stream(kw.pop("ovec"), mask=np.ones(SHAPE, np.uint8), sublist=np.zeros((1, 3), np.float32), **kw)
    assert "WARNING" not in capsys.readouterr().out                      # the refusal comes before the threshold warnings


def test_stream_keeps_its_other_refusals(fj, monkeypatch):
    from fibers_jl_amd import _lib
    monkeypatch.setattr(_lib, "lib", lambda: pytest.fail("stream reached the library"))
    ov, sub = _vol(SHAPE, 3), np.zeros((1, 3), np.float32)
    with pytest.raises(ValueError, match=r"mask shape \(3, 2, 3\) does not match orientation volume \(3, 2, 4\)"):
        fj.stream(ov, mask=np.ones(OTHER, np.uint8), sublist=sub)
    with pytest.raises(RuntimeError, match=r"Dimension mismatch between seed mask \(3, 2, 3\) and brain mask \(3, 2, 4\)"):
        fj.stream(ov, mask=np.ones(SHAPE, np.uint8), seed=fj.MRI(np.ones(OTHER, np.uint8)), sublist=sub)
    with pytest.raises(ValueError, match="need one amplitude volume per orientation volume"):
        fj.stream(ov, f=[_vol(SHAPE), _vol(SHAPE)], mask=np.ones(SHAPE, np.uint8), sublist=sub)
    with pytest.raises(ValueError, match="mask is required"):
        fj.stream(ov, sublist=sub)
