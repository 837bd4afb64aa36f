"""fibers.jl_amd — MI355X (gfx950) back end for the Fibers.jl reconstruction + tractography hot path.

Host-side mirror of the reference's exported surface for that path (same names, argument meaning and
error behaviour): `MRI`, `ODF`, `sphere_362/642/724`, `DTI`, `dti_fit`, `adc_fit`, ... on top of the
C ABI in include/fibers_hip.h.  All compute happens in libfibers_hip.so (hand-written HIP); there is
no CPU path in this package."""
from ._lib import DEVICE_ALL, FibersError, LIB_PATH, init, lib, shutdown, trim  # noqa: F401
from .mri import MRI  # noqa: F401
from .odf import ODF, sphere_362, sphere_642, sphere_724  # noqa: F401
from .dti import DTI, DtiPlan, adc_fit, adc_fit_device, dti_fit, dti_fit_device  # noqa: F401
from .dki import DKI, DkiPlan, dki_design, dki_fit, dki_fit_device  # noqa: F401
# (the device tier of csd_rec is reached through the module: csd.csd_rec_device)
from . import csd  # noqa: F401
from .csd import CSD, CsdPlan, csd_design, csd_rec, csd_response, csd_write  # noqa: F401
# (the device tier of msmt_rec likewise: msmt.msmt_rec_device)
from . import msmt  # noqa: F401
from .msmt import (MSMT, MsmtPlan, MsmtResponse, msmt_design, msmt_rec, msmt_response, msmt_shells, msmt_wm_response,  # noqa: F401
                   msmt_write)
# (the device tier of dwi_denoise is reached through the module: denoise.dwi_denoise_device)
from . import denoise  # noqa: F401
from .denoise import Denoised, dwi_denoise  # noqa: F401
# (the device tier of the brain mask is reached through the module: mask.dwi_mask_device, mask.vol_median_device, mask.mask_components_device)
from . import mask  # noqa: F401
from .mask import BrainMask, dwi_mask, mask_components, vol_median  # noqa: F401
# (the device tier of the Gibbs-ringing removal is reached through the module: degibbs.dwi_degibbs_device)
from . import degibbs  # noqa: F401
from .degibbs import Degibbsed, dwi_degibbs, dwi_degibbs_check, dwi_degibbs_work_size  # noqa: F401
from .gqi import (DSI, GQI, OdfPlan, dsi_rec, find_peaks, find_peaks_device, find_peaks_work, gqi_rec, odf_rec_device,  # noqa: F401
                  qa_normalize_device)
from .rumba import RUMBASD, RumbaPlan, rumba_rec, rumba_rec_device  # noqa: F401
from .structens import st_eigen, st_eigen_device, st_recon, st_recon_device, st_recon_halo  # noqa: F401
from .tract import Tract  # noqa: F401
from .stream import (StreamBuffers, StreamWorkspace, angles_to_vectors, angles_to_vectors_device, make_sublist, stream,  # noqa: F401
                     stream_device, stream_device_run, stream_device_run_enqueue, stream_field_device)
from .mgh import load_mgh, save_mgh  # noqa: F401
from .nifti import (dsi_write, dti_write, gqi_write, load_nifti, mri_read, mri_read_bfiles, mri_write, rumba_write,  # noqa: F401
                    read_struct)
from .trk import str_add, stream_to_trk, tract_header, trk_read, trk_write  # noqa: F401
from .xform import Xform, str_merge, str_xform, xfm_apply, xfm_compose, xfm_inv, xfm_read, xfm_rotate  # noqa: F401
from .tractmap import (str_density, str_density_device, str_sample, str_sample_device, str_stats, str_stats_device,  # noqa: F401
                       str_work_size)
from .tractsel import (Connectome, str_connectome, str_connectome_device, str_gather_device, str_roi_pack_device, str_select,  # noqa: F401
                       str_select_device, str_select_work_size, str_take)
from .bundle import (Bundles, str_assign_device, str_bundles, str_centroids, str_centroids_device, str_profile, str_resample,  # noqa: F401
                     str_resample_device)
# (the device tier of the tractogram weights is reached through the module: fixel.fixel_assign_device, fixel.fixel_td_device,
# fixel.str_weights_device, fixel.str_weights_work_size)
from . import fixel  # noqa: F401
from .fixel import FixelOverflow, TractWeights, connectome_weighted, str_weights  # noqa: F401
from .volxform import mri_xform, vol_xform_device, vol_xform_matrix, xfm_header  # noqa: F401
# (the device tier of the registration is reached through the module: register.reg_hist_device, register.vol_halve_device,
# register.vol_range_device, register.mri_register_device)
from . import register  # noqa: F401
from .register import Moco, Registration, dwi_moco, mri_register  # noqa: F401
# (the device tier of prob_stream is reached through the module: probtrack.prob_table_device, probtrack.prob_stream_device)
from . import probtrack  # noqa: F401
from .probtrack import ProbPlan, prob_row_pitch, prob_stream, prob_work_size  # noqa: F401
# (the device tier of the warps likewise: warp.warp_pack_device, warp.warp_points_device, warp.warp_volume_device, warp.warp_invert_device)
from . import warp  # noqa: F401
from .warp import Warp, mri_warp, str_warp, warp_invert, warp_read, warp_write  # noqa: F401
# (the device tier of the non-linear registration likewise: nlreg.nlreg_step_device, nlreg.warp_smooth_device, nlreg.warp_upsample_device,
# nlreg.warp_unpack_device, nlreg.warp_jacobian_device, nlreg.mri_nlreg_device)
from . import nlreg  # noqa: F401
from .nlreg import NonlinearRegistration, mri_nlreg, warp_jacobian  # noqa: F401
