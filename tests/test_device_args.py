"""The device tier rejects host tensors in Python (fibers.jl_amd/_dev.py): every device function that needs no plan, given CPU tensors,
raises ArgError, with `_lib.lib` patched so that reaching the library at all fails the test.  No GPU."""
import pytest
import torch

F, I32, U8 = torch.float32, torch.int32, torch.uint8
SHAPE = (4, 4, 4)
NVOX = 64


def _lines():
    return torch.zeros((6, 3), dtype=F), torch.tensor([5, 1, 0], dtype=I32)


def _calls(fj):
    xyz, npts = _lines()
    vol = torch.zeros(NVOX, dtype=F)
    rows = torch.zeros((3, 4, 3), dtype=F)
    six = [torch.zeros(NVOX, dtype=F) for _ in range(6)]
    return {
        "str_density_device": lambda: fj.str_density_device(xyz, npts, SHAPE),
        "str_sample_device": lambda: fj.str_sample_device(xyz, vol, SHAPE),
        "str_stats_device": lambda: fj.str_stats_device(xyz, npts, (1, 1, 1)),
        "str_roi_pack_device": lambda: fj.str_roi_pack_device(torch.zeros((2, NVOX), dtype=U8)),
        "str_select_device": lambda: fj.str_select_device(xyz, npts, SHAPE),
        "str_gather_device": lambda: fj.str_gather_device(xyz, npts, torch.ones(3, dtype=U8)),
        "str_connectome_device": lambda: fj.str_connectome_device(xyz, npts, SHAPE, torch.zeros(NVOX, dtype=I32), 2),
        "str_resample_device": lambda: fj.str_resample_device(xyz, npts, (1, 1, 1), npoints=4),
        "str_assign_device": lambda: fj.str_assign_device(rows, rows[:2].contiguous(), (1, 1, 1), 5.0),
        "str_centroids_device": lambda: fj.str_centroids_device(rows, torch.zeros(3, dtype=I32), None, 2),
        "vol_xform_device": lambda: fj.vol_xform_device(torch.eye(4).numpy(), vol, SHAPE, SHAPE),
        "xfm_apply": lambda: fj.xfm_apply(fj.Xform(), xyz),
        "st_eigen_device": lambda: fj.st_eigen_device(six),
        "st_recon_device": lambda: fj.st_recon_device(vol, SHAPE, 1.0, 1.0),
        "stream_field_device": lambda: fj.stream_field_device([torch.zeros((3, NVOX), dtype=F)], mask=torch.ones(NVOX, dtype=U8)),
    }


NAMES = ["st_eigen_device", "st_recon_device", "str_assign_device", "str_centroids_device", "str_connectome_device", "str_density_device",
         "str_gather_device", "str_resample_device", "str_roi_pack_device", "str_sample_device", "str_select_device", "str_stats_device",
         "stream_field_device", "vol_xform_device", "xfm_apply"]


@pytest.mark.parametrize("name", NAMES)
def test_host_tensors_are_rejected_before_the_library_is_reached(fj, monkeypatch, name):
    from fibers_jl_amd import _dev, _lib
    monkeypatch.setattr(_lib, "lib", lambda: pytest.fail("%s reached the library with a host tensor" % name))
    calls = _calls(fj)
    assert sorted(calls) == NAMES
    with pytest.raises(_dev.ArgError, match="CUDA tensor"):
        calls[name]()


def test_arg_error_is_both_of_the_errors_callers_catch(fj):
    from fibers_jl_amd._dev import ArgError
    assert issubclass(ArgError, ValueError) and issubclass(ArgError, TypeError)
    for what in (ValueError, TypeError):
        with pytest.raises(what):
            fj.str_sample_device(torch.zeros((2, 3)), torch.zeros(NVOX), SHAPE)
