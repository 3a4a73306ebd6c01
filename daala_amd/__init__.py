"""daala_amd - MI355X-native block-transform hot path of the Daala encoder.

The product is the C-ABI shared library daala_amd/lib/libdaalahip.so
(include/daala_hip.h).  This package is only the thin host-side mirror used by
tests, bench.py and the frame-sharded driver: it loads the library with ctypes
and passes torch device pointers / streams to it.  PyTorch is plumbing here
(device memory, streams, torch.distributed), not the compute path.

There is NO CPU fallback: importing `daala_amd.api` raises if the HIP library
has not been built, and every call raises if the library reports an error.
"""
from .api import (DaalaHipError, PulseRangeError, ExportRingBusyError, EBUSY, metrics_planes, psnrhvs_windows, psnr_db, psnrhvs_db, PipeMetrics, METRIC_SSE, METRIC_PSNRHVS, METRIC_SSIM, METRIC_MSSSIM, METRIC_FASTSSIM, METRIC_CIEDE, ciede_pictures, ciede_terms, ciede_lab_terms, ciede_score, FASTSSIM_LEVELS, fastssim_level_size, fastssim_tool_exact, fastssim_score, fastssim_planes, fastssim_terms, MSSSIM_SCALES, MSSSIM_MIN_SIZE, msssim_taps, msssim_weights, msssim_score, msssim_planes, msssim_terms, SSIM_MAX_RADIUS, ssim_taps, ssim_weight, ssim_score, ssim_planes, ssim_terms, SAMPLE_U8, SAMPLE_U16, SAMPLE_I16_12, CSF_Y, CSF_CB, CSF_CR, pvq_k_range_take, lib, lib_path, EXPERIMENTS_LIB, init, fdct2d_batch, idct2d_batch,  # noqa: F401
                  fdct2d_plane, idct2d_plane, filter_batch, dering_planes, forward_pyramid, inverse_level,
                  pvq_search_batch, pvq_search_row_batch, copy_ceiling, decode_export_sections, export_layout_make, pvq_band_layout, alloc_pvq_cands, unpack_cands, BAND_RECORD,
                  pvq_noref_bands,
                  pvq_select_synth_noref, PvqJob, pvq_noref_bands_multi,
                  pvq_select_synth_noref_multi, pvq_choose_multi, inverse_level_pvq, inverse_levels_pvq, pvq_profile, pvq_profile_read, pvq_ref_prepare,
                  pvq_ref_candidates, pvq_synthesis, REFPREP_RECORD, REFCAND_RECORD, host,
                  PvqRefJob, pvq_ref_bands_multi, pvq_ref_select_synth_multi,
                  pvq_ref_set_theta_margin, pvq_ref_theta_probe, REF_SLOTS, REFBAND_RECORD,
                  REFITEM_RECORD, REFBAND_R_NULL, REFBAND_THETA, REFBAND_NOREF, REFBAND_FLIP,
                  REFBAND_UNCERTAIN, REFITEM_SEARCHED, REFITEM_WITH_REF, REFITEM_K_RANGE, REFITEM_MOMENT_SHIFT, pvq_ref_profile,
                  pvq_ref_profile_read, image_planes_copy_pad, inverse_levels, pvq_ref_resolve_finish, cfl_refs_from_luma, pvq_ref_set_context,
                  pvq_ref_choose_multi, inverse_levels_pvq_ref, Context, Pipe, PIPE_STAGES,
                  BUF_PIC, BUF_PX, BUF_LEVEL, BUF_RECON, BUF_BAND, BUF_Y, BUF_CHOICE, BUF_ITEMS,
                  BUF_REF, BUF_RATE, compute_dist, set_price_tol_scale, px_dtype,
                  image_planes_copy_pad16, pvq_choose_priced_multi,
                  pvq_ref_choose_priced_multi, pvq_ref_bands_decided_multi, BAND_RECORD,
                  pvq_decode_bands, Y4M, Y4M_ALLOW_444)
from .api import BUF_PRED, mc_predict, mc_leaves, mc_check_grid, MotionRangeError, MV_POINT  # noqa: F401
from .api import MeJob, ME_CAND, me_search, me_limits, me_costs  # noqa: F401
from .api import MeJob2, ME_CHROMA, ME_SATD, me_search2, me_costs2  # noqa: F401
from .api import MeJob3, me_search3, me_costs3, me_downsample  # noqa: F401
from .api import MeJob4, me_search_vbs, me_cell_dist  # noqa: F401
from .api import forward_partition, forward_partition_host  # noqa: F401
from .api import (inverse_partition, PartitionLeaves, PartitionPvq, partition_leaves, partition_leaves_host,  # noqa: F401
                  partition_gather, partition_scatter, pvq_partition_noref, pvq_partition_ref)
from .api import cfl_refs_partition, cfl_refs_partition_host, keyframe_partition_420  # noqa: F401
from ._abi import bind  # noqa: F401
from .quant import QuantTables, OD_PVQ_LAMBDA  # noqa: F401
from .api import HaarJob, haar_planes, haar_encode, haar_decode  # noqa: F401
from .api import (BSIZE_TERMS, bsize_decide, bsize_terms, bsize_decide_host, bsize_terms_host,  # noqa: F401
                  bsize_set_test_hooks)
