"""ctypes binding of libia3.so (C ABI declared in include/ia3.h).

The library is the product: there is no CPU fallback.  Importing this module without a built
``libia3.so`` raises ImportError; calling into it without a HIP device raises RuntimeError.
"""
import ctypes as C
import os
import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("IA3_LIB_PATH") or os.path.join(_HERE, "libia3.so")   # IA3_LIB_PATH: developer builds (scripts/ab_*)

# the #defines of include/ia3.h, under the header's names
IA3_U16, IA3_F32 = 0, 1
IA3_OK, IA3_EINVAL, IA3_EHIP, IA3_ENOMEM, IA3_ECAPACITY, IA3_EUNSUPPORTED = 0, -1, -2, -3, -4, -5
IA3_MODE_REFLECT, IA3_MODE_NEAREST, IA3_MODE_CONSTANT = 0, 1, 2
(IA3_TUNE_GAUSS_CERT, IA3_TUNE_DFT_VALU, IA3_TUNE_UPLOAD_THREADS, IA3_TUNE_SEED_DENSE, IA3_TUNE_FIT_NBLIST, IA3_TUNE_FFT_C2C,
 IA3_TUNE_FIT_FUSE, IA3_TUNE_GAUSS_FOLD, IA3_TUNE_SEED_STRIPS, IA3_TUNE_FIT_WAVES, IA3_TUNE_FIT_MERGE, IA3_TUNE_WARP_ONEPASS,
 IA3_TUNE_FIT_KDQ, IA3_TUNE_FIT_MEMO, IA3_TUNE_SEED_FUSED, IA3_TUNE_SEED_SKIP, IA3_TUNE_COL_RTC, IA3_TUNE_SEED_BGORDER,
 IA3_TUNE_DIST_TILE, IA3_TUNE_FIT_PAIR) = range(1, 21)
IA3_DEBUG_FIT_MAXFEV, IA3_DEBUG_FIT_WAITBOUND = 100, 101
IA3_BLUR_MAX_GB = 32
IA3_BLUR_DIVIDE, IA3_BLUR_SUBTRACT = 0, 1           # ia3_blurnorm2d modes
IA3_OFFSET_ALIGNMENT_TOOLS, IA3_OFFSET_FITTING_V4 = 0, 1    # fftalign_2d offset conventions
IA3_MORPH_ERODE, IA3_MORPH_DILATE, IA3_MORPH_CLOSE = 0, 1, 2   # ia3_binary_morph_dev operations
IA3_SELECT_THREADS, IA3_SELECT_TILE = 256, 256      # spots of a workgroup, candidates of an LDS tile
IA3_SELECT_EMPTY = 1                                # ia3_select_chromosomes_dev: every candidate was removed
IA3_PICK_MAX_CHANNELS = 8
IA3_DENSITY_MAX_CELL = 65536                        # loci of one cell of a DensityPopulation
IA3_MOVIE_MAXCH = 8
IA3_CLOUD_F64, IA3_CLOUD_F32 = 0, 1                 # ia3_cloud_render modes
IA3_CLOUD_MAX_S, IA3_CLOUD_MAX_KER_S, IA3_CLOUD_MAX_IMAGES, IA3_CLOUD_MAX_DIM = 4096, 511, 65535, 4096
IA3_DOMAIN_MAX_WINDOW, IA3_DOMAIN_MAX_WINDOWS, IA3_DOMAIN_MAX_R = 16, 16, 16384   # window size, sizes per call, loci of a copy
(IA3_DOMAIN_WINDOW_MEDIAN, IA3_DOMAIN_WINDOW_MEAN, IA3_DOMAIN_WINDOW_KS, IA3_DOMAIN_WINDOW_NORMED_INSULATION,
 IA3_DOMAIN_WINDOW_INSULATION) = range(5)
IA3_DOMAIN_DIST_MEDIAN, IA3_DOMAIN_DIST_ABSOLUTE_MEDIAN, IA3_DOMAIN_DIST_INSULATION = range(3)
IA3_SCORE_MAX_PER_REGION, IA3_SCORE_MAX_LOCAL = 64, 33   # rows of one region id in a chromosome, local_size
(IA3_SCORE_KIND_DIST_LINEAR, IA3_SCORE_KIND_DIST_CDF, IA3_SCORE_KIND_INT_LINEAR, IA3_SCORE_KIND_INT_CDF,
 IA3_SCORE_KIND_CUM_PROB) = range(5)
IA3_SCORE_REF_MEDIAN, IA3_SCORE_REF_MEAN, IA3_SCORE_REF_RG, IA3_SCORE_REF_CDF = range(4)
IA3_CELLPICK_MAX_CHROM, IA3_CELLPICK_MAX_SPOTS = 6, 64   # chromosomes of a cell, merged spots of a region
IA3_CELLPICK_NAIVE_OWN, IA3_CELLPICK_NAIVE_MERGED = 0, 1
IA3_CELLPICK_MAX_TUPLES = 4194304                        # index tuples one spot of the next region may walk
# the names this module gave some of them before
MODE_REFLECT, MODE_NEAREST, MODE_CONSTANT = IA3_MODE_REFLECT, IA3_MODE_NEAREST, IA3_MODE_CONSTANT
BLUR_DIVIDE, BLUR_SUBTRACT, BLUR_MAX_GB = IA3_BLUR_DIVIDE, IA3_BLUR_SUBTRACT, IA3_BLUR_MAX_GB
OFFSET_ALIGNMENT_TOOLS, OFFSET_FITTING_V4 = IA3_OFFSET_ALIGNMENT_TOOLS, IA3_OFFSET_FITTING_V4
MORPH_ERODE, MORPH_DILATE, MORPH_CLOSE = IA3_MORPH_ERODE, IA3_MORPH_DILATE, IA3_MORPH_CLOSE
SELECT_THREADS, SELECT_TILE = IA3_SELECT_THREADS, IA3_SELECT_TILE
PICK_MAX_CHANNELS, MOVIE_MAXCH = IA3_PICK_MAX_CHANNELS, IA3_MOVIE_MAXCH


class SeedParams(C.Structure):
    _fields_ = [("th_seed", C.c_double), ("gfilt_size", C.c_double), ("background_gfilt_size", C.c_double),
                ("filt_size", C.c_int), ("min_edge_distance", C.c_int), ("use_dynamic_th", C.c_int),
                ("dynamic_niters", C.c_int), ("min_dynamic_seeds", C.c_int), ("remove_hot_pixel", C.c_int),
                ("hot_pixel_th", C.c_int), ("max_num_seeds", C.c_int), ("th_compare_f32", C.c_int),
                ("w_front", C.POINTER(C.c_double)), ("r_front", C.c_int),
                ("w_back", C.POINTER(C.c_double)), ("r_back", C.c_int)]


class LegacySeedParams(C.Structure):
    _fields_ = [("num_seeds", C.c_int), ("seed_radius", C.c_double), ("gfilt_size", C.c_double),
                ("background_gfilt_size", C.c_double), ("filt_size", C.c_int), ("th_seed", C.c_double),
                ("dynamic", C.c_int), ("dynamic_iters", C.c_int), ("min_dynamic_seeds", C.c_int),
                ("hot_pix_th", C.c_int)]


class FitParams(C.Structure):
    _fields_ = [("radius_fit", C.c_int), ("min_delta_center", C.c_double), ("max_delta_center", C.c_double),
                ("n_max_iter", C.c_int), ("max_dist_th", C.c_double), ("min_w", C.c_double),
                ("max_w", C.c_double), ("init_w", C.c_double),
                ("model_variant", C.c_int), ("init_w_zxy", C.c_double * 3)]


class FovJob(C.Structure):
    _fields_ = [("host", C.c_void_p), ("dev", C.c_void_p), ("rows", C.c_void_p), ("capacity", C.c_int),
                ("n_rows", C.c_int), ("n_seeds", C.c_int), ("n_iter", C.c_int), ("rc", C.c_int),
                ("fits", C.c_longlong), ("nfev", C.c_longlong), ("voxel_evals", C.c_longlong)]


class ChromParams(C.Structure):
    """ia3_chrom_params (include/ia3.h)."""
    _fields_ = [("filt_size", C.c_int), ("morphology_size", C.c_int), ("min_label_size", C.c_int),
                ("binary_per_th", C.c_double)]


class MovieParams(C.Structure):
    """ia3_movie_params (include/ia3.h)."""
    _fields_ = [("frames", C.c_int), ("X", C.c_int), ("Y", C.c_int), ("Z", C.c_int),
                ("n_load", C.c_int), ("load_start", C.c_int * MOVIE_MAXCH), ("load_step", C.c_int),
                ("n_sel", C.c_int), ("sel", C.c_int * MOVIE_MAXCH),
                ("hot_pixel_corr", C.c_int), ("hot_pixel_th", C.c_double), ("z_shift_corr", C.c_int),
                ("n_bleed", C.c_int), ("bleed_idx", C.c_int * MOVIE_MAXCH),
                ("bleed_profile", C.c_void_p), ("bleed_dtype", C.c_int),
                ("illum_profile", C.c_void_p * MOVIE_MAXCH), ("illum_dtype", C.c_int * MOVIE_MAXCH),
                ("drift_idx", C.c_int), ("ref_bead", C.c_void_p), ("drift_ref", C.c_void_p),
                ("n_crops", C.c_int), ("crops", C.c_int * 48),
                ("precision_fold", C.c_int), ("normalization", C.c_int), ("min_good_drifts", C.c_int),
                ("drift_diff_th", C.c_double),
                ("warp", C.c_int), ("warp_always", C.c_int * MOVIE_MAXCH),
                ("chrom_field", C.c_void_p * MOVIE_MAXCH), ("chrom_dtype", C.c_int * MOVIE_MAXCH),
                ("highpass_sigma", C.c_double), ("highpass_truncate", C.c_double),
                ("fit_spots", C.c_int),
                ("seed", SeedParams * MOVIE_MAXCH), ("fit", FitParams),
                ("normalize", C.c_int), ("bg_crop_size", C.c_int), ("bg_edges", C.POINTER(C.c_double)),
                ("bg_n_edges", C.c_int), ("bg_max_iter", C.c_int),
                ("correct_threads", C.c_int), ("fit_group_images", C.c_int), ("upload_ahead", C.c_int)]


class MovieJob(C.Structure):
    """ia3_movie_job (include/ia3.h)."""
    _fields_ = [("host_raw", C.c_void_p), ("path", C.c_char_p), ("offset_bytes", C.c_longlong), ("big_endian", C.c_int),
                ("drift_in", C.c_double * 3), ("measure_drift", C.c_int),
                ("images_out", C.c_void_p * MOVIE_MAXCH),
                ("rows", C.c_void_p * MOVIE_MAXCH), ("capacity", C.c_int * MOVIE_MAXCH),
                ("drift", C.c_double * 3), ("drift_flag", C.c_int),
                ("n_rows", C.c_int * MOVIE_MAXCH), ("n_seeds", C.c_int * MOVIE_MAXCH), ("n_iter", C.c_int * MOVIE_MAXCH),
                ("rc", C.c_int),
                ("t_upload_ms", C.c_double), ("t_correct_ms", C.c_double), ("t_fit_ms", C.c_double),
                ("stamps", C.c_double * 6)]


# Every entry of include/ia3.h: name -> (restype, [argtypes]); lib() declares them to ctypes.  A C type maps to ONE
# ctypes type, here and in tests/test_abi_cpu.py, which reads the header:
#   int, double, long long, size_t             c_int, c_double, c_longlong, c_size_t
#   char*                                      c_char_p
#   pointer to an arithmetic type              POINTER of its ctypes type (const ignored); uint8_t and unsigned char are
#                                              c_ubyte; long long and int64_t are BOTH c_int64, the type of a NumPy int64
#                                              array (c_longlong is another class of the same size on this platform)
#   pointer to a parameter struct              POINTER of its mirror above
#   void*, an opaque handle, T**               c_void_p
assert C.sizeof(C.c_int64) == C.sizeof(C.c_longlong) == 8
_I, _D, _LL, _SZ, _S, _H = C.c_int, C.c_double, C.c_longlong, C.c_size_t, C.c_char_p, C.c_void_p
_DP, _IP, _FP, _BP = C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_float), C.POINTER(C.c_ubyte)
_LP, _ULP = C.POINTER(C.c_int64), C.POINTER(C.c_uint64)
_SEED, _FIT, _LSEED, _CHROM = C.POINTER(SeedParams), C.POINTER(FitParams), C.POINTER(LegacySeedParams), C.POINTER(ChromParams)
_FOVJ, _MOVJ, _MOVP = C.POINTER(FovJob), C.POINTER(MovieJob), C.POINTER(MovieParams)
PROTOTYPES = {
    # runtime
    "ia3_init": (_I, [_I]),
    "ia3_last_error": (_S, []),
    "ia3_version": (_S, []),
    "ia3_device_name": (_I, [_S, _I]),
    "ia3_sync": (_I, []),
    "ia3_stream": (_H, []),
    "ia3_release_workspace": (_I, []),
    "ia3_prepare_depth": (_I, [_I, _I]),
    "ia3_col_guard": (_I, [_I, _I, _I]),
    "ia3_col_weights": (_I, [_I, _I, _I, _DP, _DP, _I]),
    "ia3_workspace_stats": (_I, [_DP]),
    "ia3_seed_skip_stats": (_I, [_DP]),
    "ia3_seed_bg_stats": (_I, [_DP]),
    "ia3_profile_enable": (_I, [_I]),
    "ia3_profile_collect": (_I, [_S, _I]),
    "ia3_set_tuning": (_I, [_I, _I]),
    # device-resident stacks
    "ia3_stack_upload": (_I, [_H, _I, _I, _I, _I, _H]),
    "ia3_stack_alloc": (_I, [_I, _I, _I, _I, _H]),
    "ia3_stack_load_file": (_I, [_S, _LL, _I, _I, _I, _I, _H]),
    "ia3_stack_wrap": (_I, [_H, _I, _I, _I, _I, _H]),
    "ia3_stack_deinterleave": (_I, [_H, _I, _I, _I, _H]),
    "ia3_buffer_upload": (_I, [_H, _SZ, _H]),
    "ia3_buffer_free": (None, [_H]),
    "ia3_buffer_alloc": (_I, [_SZ, _H]),
    "ia3_buffer_download": (_I, [_H, _SZ, _H]),
    "ia3_stack_download": (_I, [_H, _H]),
    "ia3_stack_info": (_I, [_H, _IP, _IP, _IP, _IP, _H]),
    "ia3_stack_free": (None, [_H]),
    # filters
    "ia3_gaussian_filter": (_I, [_H, _I, _I, _I, _I, _D, _D, _I, _DP, _I, _H]),
    "ia3_gaussian_filter_dev": (_I, [_H, _D, _D, _I, _DP, _I, _H]),
    "ia3_gaussian_highpass": (_I, [_H, _I, _I, _I, _I, _D, _D, _DP, _I, _H]),
    "ia3_gaussian_highpass_dev": (_I, [_H, _D, _D, _DP, _I, _H]),
    "ia3_remove_hot_pixels": (_I, [_H, _I, _I, _I, _I, _D, _D, _H, _IP]),
    "ia3_z_shift_correction": (_I, [_H, _I, _I, _I, _I, _H, _FP]),
    "ia3_illumination_correct": (_I, [_H, _I, _I, _I, _H, _I, _H]),
    "ia3_bleedthrough_correct": (_I, [_H, _I, _I, _I, _I, _H, _I, _H]),
    # order statistics of a resident stack and illumination profiles
    "ia3_stack_order_stats_dev": (_I, [_H, _LP, _I, _H]),
    "ia3_stack_percentiles_dev": (_I, [_H, _DP, _I, _DP]),
    "ia3_clip_sum_z_dev": (_I, [_H, _I, _D, _D, _DP]),
    "ia3_gaussian_filter2d_f64_dev": (_I, [_DP, _I, _I, _D, _D, _I, _DP, _I, _DP]),
    "ia3_gaussian_filter2d_f64": (_I, [_DP, _I, _I, _D, _D, _I, _DP, _I, _DP]),
    "ia3_illumination_image_profile_dev": (_I, [_H, _I, _D, _D, _D, _DP, _I, _DP]),
    # seeding
    "ia3_dog_seed": (_I, [_H, _I, _I, _I, _I, _SEED, _DP, _I, _IP, _DP]),
    "ia3_dog_seed_dev": (_I, [_H, _SEED, _DP, _I, _IP, _DP]),
    "ia3_dog_filters_dev": (_I, [_H, _D, _D, _H, _H]),
    # chromatic-aberration and bleedthrough profile generation
    "ia3_crop_pairs_dev": (_I, [_H, _H, _DP, _DP, _I, _IP, _H, _H, _DP, _DP, _DP]),
    "ia3_poly_field_dev": (_I, [_DP, _IP, _IP, _DP, _I, _I, _I, _I, _H]),
    "ia3_bleedthrough_profile_dev": (_I, [_DP, _BP, _I, _I, _DP, _I, _I, _I, _I, _I, _I, _H, _LP]),
    # the pre-correction chain on resident stacks
    "ia3_remove_hot_pixels_dev": (_I, [_H, _D, _D, _I, _IP]),
    "ia3_z_shift_correction_dev": (_I, [_H, _H]),
    "ia3_illumination_correct_dev": (_I, [_H, _H, _I, _H]),
    "ia3_bleedthrough_correct_dev": (_I, [_H, _I, _H, _I, _H]),
    "ia3_illumination_rescale_dev": (_I, [_H, _H, _I, _I, _H]),
    "ia3_bleedthrough_rescale_dev": (_I, [_H, _I, _H, _I, _I, _H]),
    # background level
    "ia3_find_background": (_I, [_H, _I, _I, _I, _I, _DP, _I, _I, _DP]),
    "ia3_find_background_dev": (_I, [_H, _DP, _I, _I, _DP]),
    "ia3_local_background_dev": (_I, [_H, _FP, _I, _I, _DP, _I, _I, _DP]),
    # legacy per-cell seeding
    "ia3_seed_in_distance": (_I, [_H, _I, _I, _I, _I, _DP, _LSEED, _LP, _I, _IP]),
    # fitting
    "ia3_fit_create": (_I, [_H, _DP, _I, _FIT, _H]),
    "ia3_fit_first": (_I, [_H]),
    "ia3_fit_repeat": (_I, [_H, _IP]),
    "ia3_fit_run": (_I, [_H]),
    "ia3_fit_results": (_I, [_H, _FP, _BP, _IP]),
    "ia3_fit_results_ex": (_I, [_H, _FP, _BP, _IP, _IP]),
    "ia3_fit_nfev": (_I, [_H, _IP]),
    "ia3_fit_stats": (_I, [_H, _LP, _LP]),
    "ia3_fit_counters": (_I, [_H, _ULP]),
    "ia3_fit_destroy": (None, [_H]),
    # views of a finished fit
    "ia3_fit_snapshot": (_I, [_H]),
    "ia3_fit_view_voxels": (_I, [_H, _IP, _IP, _DP]),
    "ia3_fit_view_recs": (_I, [_H, _I, _IP, _BP, _DP, _DP]),
    "ia3_fit_view_residual": (_I, [_H, _I, _DP]),
    "ia3_fit_view_residual_dev": (_I, [_H, _I, _H]),
    "ia3_fit_create_fovs": (_I, [_H, _H, _IP, _I, _FIT, _H]),
    "ia3_gaussfit_voxels": (_I, [_DP, _IP, _IP, _I, _DP, _DP, _IP, _FP, _DP, _IP]),
    "ia3_fit_seeds": (_I, [_H, _I, _I, _I, _I, _DP, _I, _FIT, _FP, _BP, _IP]),
    "ia3_fit_fov_dev": (_I, [_H, _SEED, _FIT, _FP, _I, _IP, _IP, _IP]),
    "ia3_fit_fov_stats": (_I, [_LP, _LP, _LP]),
    "ia3_fit_fov_wait_share": (_I, [_LP, _LP]),
    "ia3_fit_fovs": (_I, [_FOVJ, _I, _I, _I, _I, _I, _SEED, _FIT, _I]),
    # drift
    "ia3_fftalign_2d": (_I, [_DP, _I, _I, _DP, _I, _I, _DP, _D, _IP]),
    "ia3_fft3d_from2d": (_I, [_H, _H, _I, _I, _I, _I, _D, _IP]),
    "ia3_fft3d_from2d_dev": (_I, [_H, _H, _D, _IP]),
    "ia3_blurnorm2d": (_I, [_FP, _I, _I, _I, _I, _FP]),
    "ia3_fftalign_2d_ex": (_I, [_DP, _I, _I, _DP, _I, _I, _DP, _D, _I, _IP, _DP]),
    "ia3_fft3d_from2d_ex": (_I, [_H, _H, _I, _I, _I, _I, _I, _I, _I, _D, _IP, _DP]),
    "ia3_fft3d_from2d_dev_ex": (_I, [_H, _H, _I, _I, _I, _D, _IP, _DP]),
    "ia3_phase_xcorr3d": (_I, [_H, _H, _I, _I, _I, _I, _I, _I, _DP, _DP, _DP]),
    "ia3_phase_xcorr3d_dev": (_I, [_H, _H, _I, _I, _DP, _DP, _DP]),
    "ia3_align_image_dev": (_I, [_H, _H, _IP, _I, _I, _I, _I, _D, _DP, _IP, _DP, _IP]),
    "ia3_drift_ref_create": (_I, [_H, _IP, _I, _H]),
    "ia3_drift_ref_free": (None, [_H]),
    "ia3_align_image_ref": (_I, [_H, _H, _I, _I, _I, _D, _DP, _IP, _DP, _IP]),
    # Fitting_v4's fast path
    "ia3_fastfit_normalize_dev": (_I, [_H, _I, _H]),
    "ia3_fastfit_seeds_dev": (_I, [_H, _I, _I, _D, _I, _I, _DP, _I, _IP, _DP]),
    "ia3_fastfit_moments_dev": (_I, [_H, _DP, _I, _I, _I, _I, _D, _DP, _IP, _DP, _IP]),
    "ia3_fastfit_voxels": (_I, [_DP, _IP, _I, _I, _D, _DP]),
    # warp
    "ia3_warp3d": (_I, [_H, _I, _I, _I, _I, _DP, _H, _I, _I, _I, _D, _H]),
    "ia3_warp3d_dev": (_I, [_H, _DP, _H, _I, _I, _I, _D, _H]),
    "ia3_stack_crop": (_I, [_H, _I, _I, _I, _I, _I, _I, _H]),
    # segmentation label images
    "ia3_label_boxes_dev": (_I, [_H, _I, _IP]),
    "ia3_cube_labels_dev": (_I, [_H, _DP, _I, _I, _IP, _IP]),
    "ia3_cube_max_dev": (_I, [_H, _DP, _I, _I, _H]),
    "ia3_cube_gather_dev": (_I, [_H, _DP, _I, _I, _H]),
    # candidate chromosomes
    "ia3_plane_medians_dev": (_I, [_H, _DP]),
    "ia3_chrom_seed_mask_dev": (_I, [_H, _I, _D, _H, _DP]),
    "ia3_binary_morph_dev": (_I, [_H, _I, _I, _I, _H]),
    "ia3_binary_fill_holes_dev": (_I, [_H, _H]),
    "ia3_label_dev": (_I, [_H, _IP, _IP, _H]),
    "ia3_label_centers_dev": (_I, [_H, _I, _I, _I, _I, _I, _DP, _LP]),
    "ia3_remove_small_labels_dev": (_I, [_H, _I, _I, _I, _I, _I, _LL, _H]),
    "ia3_find_candidate_chromosomes_dev": (_I, [_H, _CHROM, _DP, _I, _IP, _DP, _H]),
    # the chromosome image
    "ia3_chrom_image_create": (_I, [_I, _I, _I, _H]),
    "ia3_chrom_image_free": (None, [_H]),
    "ia3_chrom_image_upload": (_I, [_H, _DP]),
    "ia3_chrom_image_download": (_I, [_H, _DP]),
    "ia3_stack_median_dev": (_I, [_H, _DP]),
    "ia3_chrom_image_add_dev": (_I, [_H, _H, _IP, _IP, _I, _DP]),
    "ia3_find_candidate_chromosomes_f64_dev": (_I, [_H, _CHROM, _DP, _I, _IP, _DP, _H]),
    # chromosome selection by candidate spots
    "ia3_assign_nearest_dev": (_I, [_DP, _I, _DP, _I, _IP]),
    "ia3_select_chromosomes_dev": (_I, [_DP, _IP, _I, _DP, _I, _D, _IP, _IP, _IP, _IP, _IP, _LP, _DP]),
    # population spot picking
    "ia3_pick_create": (_I, [_DP, _I, _IP, _BP, _I, _I, _IP, _I, _H]),
    "ia3_pick_free": (None, [_H]),
    "ia3_pick_by_intensity_dev": (_I, [_H]),
    "ia3_pick_set_rows": (_I, [_H, _I, _DP]),
    "ia3_pick_reference_dev": (_I, [_H, _IP, _IP, _I, _DP, _I, _IP]),
    "ia3_pick_set_sorted": (_I, [_H, _I, _I, _DP, _I]),
    "ia3_pick_scores_dev": (_I, [_H, _IP, _IP, _I, _I, _D, _D, _DP, _I, _H, _IP, _I]),
    "ia3_pick_difference_dev": (_I, [_H, _IP]),
    "ia3_pick_download": (_I, [_H, _I, _H]),
    "ia3_pick_download_sorted": (_I, [_H, _I, _I, _DP]),
    "ia3_pick_cum_vals_dev": (_I, [_DP, _I, _DP, _I, _IP]),
    # summaries of population distance maps
    "ia3_dist_create": (_I, [_DP, _IP, _I, _H]),
    "ia3_dist_free": (None, [_H]),
    "ia3_dist_summary_dev": (_I, [_H, _IP, _IP, _I, _I, _I, _I, _I, _D, _DP, _IP, _IP]),
    "ia3_dist_contact_stack_dev": (_I, [_DP, _LL, _LL, _D, _DP, _IP, _IP]),
    # A/B compartment densities of traced cells
    "ia3_density_create": (_I, [_DP, _IP, _IP, _IP, _I, _I, _H]),
    "ia3_density_free": (None, [_H]),
    "ia3_density_scores_dev": (_I, [_H, _BP, _DP, _I, _I, _I, _DP, _IP]),
    # density clouds of traced chromosomes
    "ia3_cloud_render_dev": (_I, [_DP, _IP, _I, _I, _I, _I, _I, _I, _H]),
    "ia3_cloud_render": (_I, [_DP, _IP, _I, _I, _I, _I, _I, _H, _H]),
    "ia3_cloud_gauss_ker": (_I, [_DP, _I, _DP, _DP]),
    # domain distances of traced chromosomes
    "ia3_domain_create": (_I, [_DP, _I, _I, _I, _DP, _H]),
    "ia3_domain_free": (None, [_H]),
    "ia3_domain_slide_dev": (_I, [_H, _IP, _I, _I, _I, _DP]),
    "ia3_domain_dists_dev": (_I, [_H, _IP, _I, _I, _I, _I, _DP, _IP]),
    "ia3_domain_contacts_dev": (_I, [_H, _IP, _I, _D, _DP, _IP]),
    # chromosomal spot scores
    "ia3_score_create": (_I, [_DP, _LP, _IP, _DP, _LP, _IP, _DP, _IP, _I, _DP, _H]),
    "ia3_score_replace_selected": (_I, [_H, _DP, _LP, _IP]),
    "ia3_score_free": (None, [_H]),
    "ia3_score_refs_dev": (_I, [_H, _I, _I, _D, _I, _DP, _IP, _DP]),
    "ia3_score_scores_dev": (_I, [_H, _I, _I, _I, _LL, _D, _D, _I, _DP, _D, _D, _DP, _DP, _BP, _IP]),
    "ia3_score_values_dev": (_I, [_DP, _I, _D, _DP, _I, _I, _D, _D, _D, _DP, _BP, _IP]),
    "ia3_score_neighbor_lists_dev": (_I, [_H, _LL, _D, _IP, _IP, _DP, _DP]),
    # per-cell spot pickers
    "ia3_cellpick_create": (_I, [_DP, _BP, _IP, _IP, _IP, _DP, _IP, _IP, _I, _I, _DP, _H]),
    "ia3_cellpick_free": (None, [_H]),
    "ia3_cellpick_merge_dev": (_I, [_H, _I, _D, _I, _D, _IP, _IP, _IP]),
    "ia3_cellpick_naive_dev": (_I, [_H, _I, _IP, _IP]),
    "ia3_cellpick_plan": (_I, [_H, _IP, _IP, _LP]),
    "ia3_cellpick_forward_dev": (_I, [_H, _IP, _I, _DP, _I, _DP, _IP, _DP, _DP, _D, _D, _D, _I, _DP, _BP, _IP]),
    # whole round-folder movies
    "ia3_process_movies": (_I, [_MOVJ, _I, _MOVP]),
}
EXPORTS = list(PROTOTYPES)

_lib = None


def lib():
    """Load libia3.so (once).  Fails loudly when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.isfile(LIB_PATH):
            raise ImportError(
                "imageanalysis3_amd: %s not found. Build it with `python -c 'import __graft_entry__ as g; "
                "g.build()'` or `make -C imageanalysis3_amd/csrc`. There is no CPU fallback." % LIB_PATH)
        # streams of concurrent host threads onto separate hardware queues (see runtime.cpp do_init); must be in the
        # environment before the HIP runtime starts, hence also here, before anything is loaded
        os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in PROTOTYPES.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = res, args
        _lib = L
    return _lib


class IA3Error(RuntimeError):
    pass


def check(rc, allow=()):
    if rc == IA3_OK or rc in allow:
        return rc
    msg = lib().ia3_last_error().decode("utf-8", "replace")
    if rc == IA3_EINVAL:
        raise ValueError(msg)
    if rc == IA3_ENOMEM:
        raise MemoryError(msg)
    if rc == IA3_EUNSUPPORTED:
        raise NotImplementedError(msg)
    raise IA3Error("libia3 error %d: %s" % (rc, msg))


def dtype_code(arr):
    if arr.dtype == np.uint16:
        return IA3_U16
    if arr.dtype == np.float32:
        return IA3_F32
    raise TypeError("imageanalysis3_amd kernels take uint16 or float32 stacks, got %s" % arr.dtype)


def as_stack_array(im):
    """C-contiguous uint16/float32 3-D view/copy of ``im`` (the caller's array is never modified)."""
    if not isinstance(im, np.ndarray):
        raise TypeError("image given should be a numpy.ndarray, but %s is given." % type(im))
    if im.ndim != 3:
        raise IndexError("a 3-D (z,x,y) stack is required, got ndim=%d" % im.ndim)
    if im.dtype == np.uint8:
        im = im.astype(np.uint16)
    dtype_code(im)
    return np.ascontiguousarray(im)


def ptr(a):
    """Pointer to the data of an ndarray, typed by its dtype (float64: ``double*``, int32: ``int*``, ...): an entry that
    declares another element type refuses it.  An array that is to be read as another type says so with ``.view()``."""
    return a.ctypes.data_as(C.POINTER(np.ctypeslib.as_ctypes_type(a.dtype)))


dptr = _iptr = ptr   # the names callers used before the pointer carried the dtype


class Owner(object):
    """Base of the classes that own one library handle: ``_release(handle)`` hands it to the entry that frees it,
    ``_handle`` names the attribute that holds it (None once it is freed; absent when ``__init__`` never got that far)."""
    _handle = "_h"

    def _release(self, handle):
        raise NotImplementedError

    def free(self):
        h = getattr(self, self._handle, None)
        if h is not None:
            setattr(self, self._handle, None)
            self._keep = None
            self._release(h)

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.free()


class DeviceStack(Owner):
    """A (Z,X,Y) stack resident in HBM (owner of an ``ia3_stack`` handle)."""

    def __init__(self, handle, shape, dtype, keepalive=None):
        self._h = handle
        self.shape = tuple(shape)
        self.dtype = np.dtype(dtype)
        self._keep = keepalive

    @classmethod
    def upload(cls, im):
        a = as_stack_array(im)
        h = C.c_void_p()
        check(lib().ia3_stack_upload(ptr(a), dtype_code(a), a.shape[0], a.shape[1], a.shape[2], C.byref(h)))
        return cls(h, a.shape, a.dtype)

    @classmethod
    def empty(cls, shape, dtype):
        dt = np.dtype(dtype)
        code = dtype_code(np.empty(0, dt))
        h = C.c_void_p()
        check(lib().ia3_stack_alloc(code, int(shape[0]), int(shape[1]), int(shape[2]), C.byref(h)))
        return cls(h, shape, dt)

    @classmethod
    def wrap_torch(cls, t):
        """Borrow the memory of a contiguous CUDA/HIP torch tensor (uint16 as int16/uint16, or float32)."""
        import torch
        if not t.is_cuda or not t.is_contiguous() or t.dim() != 3:
            raise ValueError("need a contiguous 3-D device tensor")
        if t.dtype == torch.float32:
            dt = np.float32
        elif t.dtype in (torch.int16, getattr(torch, "uint16", torch.int16)):
            dt = np.uint16
        else:
            raise TypeError("unsupported tensor dtype %s" % t.dtype)
        h = C.c_void_p()
        code = IA3_F32 if dt == np.float32 else IA3_U16
        check(lib().ia3_stack_wrap(C.c_void_p(t.data_ptr()), code, t.shape[0], t.shape[1], t.shape[2], C.byref(h)))
        return cls(h, tuple(t.shape), dt, keepalive=t)

    @classmethod
    def from_file(cls, path, frames, X, Y, offset_bytes=0, big_endian=False):
        """Resident uint16 (frames, X, Y) stack read straight from a raw movie file (pipelined read + upload)."""
        import os
        h = C.c_void_p()
        check(lib().ia3_stack_load_file(os.fsencode(path), int(offset_bytes), int(frames), int(X), int(Y),
                                        1 if big_endian else 0, C.byref(h)))
        return cls(h, (int(frames), int(X), int(Y)), np.dtype(np.uint16))

    def crop(self, lims):
        """New resident stack = self[z0:z1, x0:x1, y0:y1]; ``lims`` is a (3,2) [start, stop) array."""
        l = np.array(lims, dtype=int)
        l[:, 0] = np.maximum(l[:, 0], 0)
        l[:, 1] = np.minimum(l[:, 1], np.array(self.shape))
        h = C.c_void_p()
        check(lib().ia3_stack_crop(self._h, int(l[0, 0]), int(l[0, 1]), int(l[1, 0]), int(l[1, 1]),
                                   int(l[2, 0]), int(l[2, 1]), C.byref(h)))
        return DeviceStack(h, tuple(int(b - a) for a, b in l), self.dtype)

    def download(self):
        out = np.empty(self.shape, dtype=self.dtype)
        check(lib().ia3_stack_download(self._h, ptr(out)))
        return out

    def order_stats(self, ranks):
        """``np.sort(stack, axis=None)[ranks]`` (at most 16 ranks) selected on the device: array of the stack dtype."""
        r = np.ascontiguousarray(ranks, dtype=np.int64).ravel()
        out = np.empty(len(r), dtype=self.dtype)
        check(lib().ia3_stack_order_stats_dev(self._h, ptr(r), len(r), ptr(out)))
        return out

    def percentiles(self, pers):
        """``[scipy.stats.scoreatpercentile(stack, p) for p in pers]`` (at most 8) from exact order statistics selected
        on the device: float64 array."""
        p = np.ascontiguousarray(pers, dtype=np.float64).ravel()
        out = np.empty(len(p), dtype=np.float64)
        check(lib().ia3_stack_percentiles_dev(self._h, ptr(p), len(p), ptr(out)))
        return out

    def _release(self, handle):
        lib().ia3_stack_free(handle)


class DeviceImage64(object):
    """A float64 (X, Y) image resident in HBM (what ``ia3_clip_sum_z_dev`` writes and ``ia3_gaussian_filter2d_f64_dev``
    reads and writes), kept in a library allocation of the same size.  ``devptr`` is the device address as a ``double*``
    (``POINTER(c_double)``, what those entries declare), not a ``c_void_p``."""

    def __init__(self, shape, _store=None):
        self.shape = (int(shape[0]), int(shape[1]))
        # X * Y * 8 bytes, as a (2, X, Y) float32 stack of the library
        self._store = DeviceStack.empty((2,) + self.shape, np.float32) if _store is None else _store
        d = C.c_void_p()
        check(lib().ia3_stack_info(self._store._h, None, None, None, None, C.byref(d)))
        self.devptr = C.cast(d, _DP)

    @classmethod
    def upload(cls, im):
        a = np.ascontiguousarray(im, dtype=np.float64)
        if a.ndim != 2:
            raise IndexError("a 2-D image is required, got ndim=%d" % a.ndim)
        raw = np.frombuffer(a.tobytes(), dtype=np.float32).reshape((2,) + a.shape)
        return cls(a.shape, _store=DeviceStack.upload(raw))

    def download(self):
        return np.frombuffer(self._store.download().tobytes(), dtype=np.float64).reshape(self.shape).copy()

    def free(self):
        self._store.free()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.free()


def clip_sum_z(stack, limits=None):
    """``np.sum(np.clip(float64(stack), lo, hi), axis=0)`` (no clip for ``limits=None``) of a resident stack, planes added
    in z order: a resident ``DeviceImage64``."""
    out = DeviceImage64(stack.shape[1:])
    lo, hi = (0.0, 0.0) if limits is None else (float(limits[0]), float(limits[1]))
    try:
        check(lib().ia3_clip_sum_z_dev(stack._h, 0 if limits is None else 1, lo, hi, out.devptr))
    except Exception:
        out.free()
        raise
    return out


def taps_argument(sigma, truncate=4.0, max_radius=1024):
    """(weights pointer or None, radius, keep-alive) for the entries that take SciPy's taps from NumPy: the taps of
    ``gaussian_taps``; None where the library refuses the filter anyway (no positive sigma, radius above its maximum)."""
    sigma, truncate = float(sigma), float(truncate)
    if not (sigma > 0 and truncate > 0) or truncate * sigma + 0.5 >= max_radius + 1:
        return None, 0, None
    w, r = gaussian_taps(sigma, truncate)
    return ptr(w), int(r), w


def gaussian_filter2d_f64(im, sigma, truncate=4.0, mode=MODE_REFLECT):
    """``scipy.ndimage.gaussian_filter`` of a float64 2-D image in float64, bit for bit: an ndarray in gives an ndarray
    (``ia3_gaussian_filter2d_f64``), a ``DeviceImage64`` a new ``DeviceImage64`` (``ia3_gaussian_filter2d_f64_dev``)."""
    wp, r, _keep = taps_argument(sigma, truncate)
    if isinstance(im, DeviceImage64):
        out = DeviceImage64(im.shape)
        try:
            check(lib().ia3_gaussian_filter2d_f64_dev(im.devptr, im.shape[0], im.shape[1], float(sigma),
                                                      float(truncate), int(mode), wp, r, out.devptr))
        except Exception:
            out.free()
            raise
        return out
    a = np.ascontiguousarray(im, dtype=np.float64)
    if a.ndim != 2:
        raise IndexError("a 2-D image is required, got ndim=%d" % a.ndim)
    out = np.empty_like(a)
    check(lib().ia3_gaussian_filter2d_f64(ptr(a), a.shape[0], a.shape[1], float(sigma),
                                          float(truncate), int(mode), wp, r, ptr(out)))
    return out


CROP_MAX = 15   # largest box of ia3_crop_pairs_dev along an axis


def crop_pairs(stack_a, centers_a, crop, stack_b=None, centers_b=None, regress=False):
    """``ia3_crop_pairs_dev``: the boxes ``crop_neighboring_area(stack, centre, crop)`` of the reference for every row of
    ``centers_a`` on the resident ``stack_a`` (and of ``centers_b`` on ``stack_b``), one call for all of them.  Returns
    ``(boxes_a, boxes_b, regression)``: (n,) + crop arrays of the stack dtype (``boxes_b`` None without a second stack) and,
    with ``regress``, the float64 arrays ``(slope, intercept, rsq)`` of box b on box a, else None."""
    crop = np.ascontiguousarray(crop, dtype=np.int32)
    ca = np.ascontiguousarray(centers_a, dtype=np.float64).reshape(-1, 3)
    n = len(ca)
    shape = (n,) + tuple(int(c) for c in crop)
    boxes_a = np.empty(shape, dtype=stack_a.dtype)
    boxes_b, cb, reg = None, None, None
    if stack_b is not None:
        cb = np.ascontiguousarray(centers_b, dtype=np.float64).reshape(-1, 3)
        if len(cb) != n:
            raise ValueError("crop_pairs: %d centres for the first stack, %d for the second" % (n, len(cb)))
        if tuple(stack_b.shape) != tuple(stack_a.shape) or np.dtype(stack_b.dtype) != np.dtype(stack_a.dtype):
            raise ValueError("crop_pairs: the two stacks must have the same shape and dtype")
        boxes_b = np.empty(shape, dtype=stack_b.dtype)
    if regress:
        reg = tuple(np.empty(n, dtype=np.float64) for _ in range(3))
    check(lib().ia3_crop_pairs_dev(stack_a._h, None if stack_b is None else stack_b._h, ptr(ca),
                                   None if cb is None else ptr(cb), n, ptr(crop),
                                   ptr(boxes_a), None if boxes_b is None else ptr(boxes_b),
                                   *([ptr(r) for r in reg] if regress else [None, None, None])))
    return boxes_a, boxes_b, reg


CUBE_MAX_RADIUS = 10          # largest search radius of the cube lookups (csrc/ia3_labels.h)


def _centres(centers_zxy):
    """(n, 3) C-contiguous float64 copy of a table of z, x, y centres."""
    c = np.ascontiguousarray(centers_zxy, dtype=np.float64)
    if c.ndim != 2 or c.shape[1] != 3:
        raise ValueError("centres should be an (n, 3) table of z, x, y, got shape %s" % (c.shape,))
    return c


def label_boxes(labels, max_label=65535):
    """``ia3_label_boxes_dev``: the (max_label + 1, 7) int32 table [count, z0, z1, x0, x1, y0, y1] of a resident uint16
    label stack, row l for label l ([start, stop) bounds without a margin; zeros for a label that does not occur)."""
    out = np.empty((int(max_label) + 1, 7), dtype=np.int32)
    check(lib().ia3_label_boxes_dev(labels._h, int(max_label), ptr(out)))
    return out


def cube_labels(labels, centers_zxy, radius, target=None):
    """``ia3_cube_labels_dev``: per centre the most frequent positive label of the clamped cube of ``radius`` around it
    (-1: none), or, with ``target`` (one label per centre), 1 where the cube holds that label and -1 where not.  int32."""
    c = _centres(centers_zxy)
    out = np.empty(len(c), dtype=np.int32)
    t = None
    if target is not None:
        t = np.ascontiguousarray(target, dtype=np.int32).ravel()
        if len(t) != len(c):
            raise ValueError("cube_labels: %d centres, %d target labels" % (len(c), len(t)))
    check(lib().ia3_cube_labels_dev(labels._h, ptr(c), len(c), int(radius),
                                    None if t is None else ptr(t), ptr(out)))
    return out


def cube_max(stack, centers_zxy, radius):
    """``ia3_cube_max_dev``: per centre the largest value of the clamped cube of ``radius`` around it, in the stack dtype
    (NaN where a float32 cube holds one)."""
    c = _centres(centers_zxy)
    out = np.empty(len(c), dtype=stack.dtype)
    check(lib().ia3_cube_max_dev(stack._h, ptr(c), len(c), int(radius), ptr(out)))
    return out


def cube_gather(stack, centers_zxy, radius):
    """``ia3_cube_gather_dev``: the (n, (2 radius + 1)^3) matrix of the clamped cubes, in the stack dtype; columns in C
    order of the offsets (dz, dx, dy)."""
    c = _centres(centers_zxy)
    out = np.empty((len(c), (2 * int(radius) + 1) ** 3), dtype=stack.dtype)
    check(lib().ia3_cube_gather_dev(stack._h, ptr(c), len(c), int(radius), ptr(out)))
    return out


MORPH_MAX_RADIUS = 2                               # largest ball of the bit-row operators
CHROM_FILT_SIZES = (1, 5)                          # _filt_size range of the range filter
MAX_LABELS16 = 65535


def stack_devptr(stack):
    """Device pointer (``c_void_p``) of the voxels of a resident stack."""
    d = C.c_void_p()
    check(lib().ia3_stack_info(stack._h, None, None, None, None, C.byref(d)))
    return C.c_void_p(d.value)


class DeviceLabels(Owner):
    """int32 labels of a (Z, X, Y) volume in a device buffer (what ``ia3_label_dev`` writes); ``n`` = number of labels."""
    _handle = "devptr"

    def __init__(self, shape, n=0):
        self.shape = tuple(int(v) for v in shape)
        self.dtype = np.dtype(np.int32)
        self.n = int(n)
        p = C.c_void_p()
        check(lib().ia3_buffer_alloc(4 * int(np.prod(self.shape)), C.byref(p)))
        self.devptr = p

    @classmethod
    def upload(cls, labels, n=None):
        a = np.ascontiguousarray(labels, dtype=np.int32)
        if a.ndim != 3:
            raise IndexError("a 3-D (z,x,y) label volume is required, got ndim=%d" % a.ndim)
        out = cls.__new__(cls)
        out.shape, out.dtype = tuple(a.shape), np.dtype(np.int32)
        out.n = int(a.max()) if n is None and a.size else int(n or 0)
        p = C.c_void_p()
        check(lib().ia3_buffer_upload(ptr(a), a.nbytes, C.byref(p)))
        out.devptr = p
        return out

    def download(self):
        out = np.empty(self.shape, dtype=np.int32)
        check(lib().ia3_buffer_download(self.devptr, out.nbytes, ptr(out)))
        return out

    def _release(self, handle):
        lib().ia3_buffer_free(handle)


def plane_medians(stack):
    """``ia3_plane_medians_dev``: ``[np.median(plane) for plane in stack]`` of a resident stack, widened to float64."""
    out = np.empty(stack.shape[0], dtype=np.float64)
    check(lib().ia3_plane_medians_dev(stack._h, ptr(out)))
    return out


def chrom_seed_mask(stack, filt_size, binary_per_th):
    """``ia3_chrom_seed_mask_dev``: (resident uint16 0 / 1 mask, threshold as ``np.float64``)."""
    out = DeviceStack.empty(stack.shape, np.uint16)
    th = C.c_double(0)
    try:
        check(lib().ia3_chrom_seed_mask_dev(stack._h, int(filt_size), float(binary_per_th), out._h, C.byref(th)))
    except Exception:
        out.free()
        raise
    return out, np.float64(th.value)


def binary_morph(mask, op, radius, border=0):
    """``ia3_binary_morph_dev`` on a resident uint16 mask: a new resident 0 / 1 mask."""
    out = DeviceStack.empty(mask.shape, np.uint16)
    try:
        check(lib().ia3_binary_morph_dev(mask._h, int(op), int(radius), 1 if border else 0, out._h))
    except Exception:
        out.free()
        raise
    return out


def binary_fill_holes(mask):
    """``ia3_binary_fill_holes_dev`` on a resident uint16 mask: a new resident 0 / 1 mask."""
    out = DeviceStack.empty(mask.shape, np.uint16)
    try:
        check(lib().ia3_binary_fill_holes_dev(mask._h, out._h))
    except Exception:
        out.free()
        raise
    return out


def label(mask, labels16=False):
    """``ia3_label_dev``: ``DeviceLabels`` (int32, ``.n`` components) of a resident uint16 mask; with ``labels16`` also
    the uint16 label stack: ``(labels, stack)``.  More than 65535 components do not fit that stack: NotImplementedError."""
    lab = DeviceLabels(mask.shape)
    out16 = DeviceStack.empty(mask.shape, np.uint16) if labels16 else None
    n = C.c_int(0)
    try:
        check(lib().ia3_label_dev(mask._h, C.cast(lab.devptr, _IP), C.byref(n), None if out16 is None else out16._h))
    except Exception:
        lab.free()
        if out16 is not None:
            out16.free()
        raise
    lab.n = n.value
    return (lab, out16) if labels16 else lab


def _label_volume(labels):
    """(device pointer, width in bits, shape) of a ``DeviceLabels`` or a resident uint16 label stack."""
    if isinstance(labels, DeviceLabels):
        return labels.devptr, 32, labels.shape
    if np.dtype(labels.dtype) != np.uint16:
        raise TypeError("a resident label stack is uint16, got %s" % labels.dtype)
    return stack_devptr(labels), 16, labels.shape


def label_centers(labels, max_label):
    """``ia3_label_centers_dev``: ((max_label, 3) float64 centres, (max_label,) int64 voxel counts) of labels
    1..max_label of a ``DeviceLabels`` or a resident uint16 label stack."""
    p, bits, shape = _label_volume(labels)
    max_label = int(max_label)
    cen = np.empty((max_label, 3), dtype=np.float64)
    cnt = np.empty(max_label, dtype=np.int64)
    check(lib().ia3_label_centers_dev(p, bits, shape[0], shape[1], shape[2], max_label, ptr(cen), ptr(cnt)))
    return cen, cnt


def remove_small_labels(labels, max_label, min_size):
    """``ia3_remove_small_labels_dev``: a new volume of the input's kind in which the labels 1..max_label with fewer than
    ``min_size`` voxels are 0."""
    p, bits, shape = _label_volume(labels)
    out = DeviceLabels(shape, labels.n) if bits == 32 else DeviceStack.empty(shape, np.uint16)
    try:
        check(lib().ia3_remove_small_labels_dev(p, bits, shape[0], shape[1], shape[2], int(max_label), int(min_size),
                                                out.devptr if bits == 32 else stack_devptr(out)))
    except Exception:
        out.free()
        raise
    return out


CHROM_ADD_BATCH = 16   # images of one launch of ia3_chrom_image_add_dev


def stack_median(stack):
    """``ia3_stack_median_dev``: ``np.median`` of a whole resident stack, as ``np.float64``."""
    out = C.c_double(0)
    check(lib().ia3_stack_median_dev(stack._h, C.byref(out)))
    return np.float64(out.value)


class ChromImage(Owner):
    """A float64 (Z, X, Y) volume resident in HBM (owner of an ``ia3_chrom_image`` handle): the chromosome image that
    ``Field_of_View._generate_chrom_im_from_data`` sums up, and what ``find_candidate_chromosomes`` reads in float64."""

    def __init__(self, handle, shape):
        self._h = handle
        self.shape = tuple(int(v) for v in shape)
        self.dtype = np.dtype(np.float64)

    @classmethod
    def empty(cls, shape):
        """``np.zeros(shape)`` on the device."""
        shape = tuple(int(v) for v in shape)
        if len(shape) != 3:
            raise IndexError("a 3-D (z,x,y) shape is required, got %s" % (shape,))
        h = C.c_void_p()
        check(lib().ia3_chrom_image_create(shape[0], shape[1], shape[2], C.byref(h)))
        return cls(h, shape)

    @classmethod
    def upload(cls, im):
        """A resident copy of a float64 (z, x, y) ndarray (values are not converted: the array must be float64)."""
        if not isinstance(im, np.ndarray):
            raise TypeError("image given should be a numpy.ndarray, but %s is given." % type(im))
        if im.dtype != np.float64:
            raise TypeError("a chromosome image is float64, got %s" % im.dtype)
        if im.ndim != 3:
            raise IndexError("a 3-D (z,x,y) stack is required, got ndim=%d" % im.ndim)
        a = np.ascontiguousarray(im)
        out = cls.empty(a.shape)
        try:
            check(lib().ia3_chrom_image_upload(out._h, ptr(a)))
        except Exception:
            out.free()
            raise
        return out

    def download(self):
        out = np.empty(self.shape, dtype=np.float64)
        check(lib().ia3_chrom_image_download(self._h, ptr(out)))
        return out

    def add(self, stacks, flags, shifts):
        """``ia3_chrom_image_add_dev``: add the resident uint16 ``stacks``; ``flags[k] == 2``: as it is, otherwise moved by
        the integer ``shifts[k]`` (z, x, y: out[j] += im[j + shift]) and filled up with its median.  Returns the medians
        used (0 for a flag-2 image) as a float64 array."""
        stacks = list(stacks)
        n = len(stacks)
        fl = np.ascontiguousarray(flags, dtype=np.int32).ravel()
        sh = np.ascontiguousarray(shifts, dtype=np.int32).reshape(-1, 3) if n else np.zeros((0, 3), np.int32)
        if len(fl) != n or len(sh) != n:
            raise ValueError("ChromImage.add: %d stacks, %d flags, %d shifts" % (n, len(fl), len(sh)))
        bg = np.zeros(n, dtype=np.float64)
        if n == 0:
            return bg
        hs = (C.c_void_p * n)(*[s._h for s in stacks])
        check(lib().ia3_chrom_image_add_dev(self._h, hs, ptr(fl), ptr(sh), n, ptr(bg)))
        return bg

    def _release(self, handle):
        lib().ia3_chrom_image_free(handle)


def find_candidate_chromosomes(stack, filt_size, binary_per_th, morphology_size, min_label_size, return_label=False,
                               capacity=4096):
    """``ia3_find_candidate_chromosomes_dev`` on a resident stack, ``ia3_find_candidate_chromosomes_f64_dev`` on a
    ``ChromImage``: ((n, 3) float64 centres, threshold as ``np.float64``, resident uint16 kept-label stack or None)."""
    p = ChromParams(int(filt_size), int(morphology_size), int(min_label_size), float(binary_per_th))
    kept = DeviceStack.empty(stack.shape, np.uint16) if return_label else None
    entry = (lib().ia3_find_candidate_chromosomes_f64_dev if isinstance(stack, ChromImage)
             else lib().ia3_find_candidate_chromosomes_dev)
    n, th = C.c_int(0), C.c_double(0)
    try:
        while True:
            coords = np.empty((capacity, 3), dtype=np.float64)
            rc = entry(stack._h, C.byref(p), ptr(coords), int(capacity), C.byref(n),
                       C.byref(th), None if kept is None else kept._h)
            if rc == IA3_ECAPACITY and n.value > capacity:
                capacity = n.value
                continue
            check(rc)
            break
    except Exception:
        if kept is not None:
            kept.free()
        raise
    return coords[:n.value].copy(), np.float64(th.value), kept


def _scaled_table(zxy, what):
    """(n, 3) C-contiguous float64 table of scaled coordinates, as ``cdist`` takes its arguments."""
    t = np.ascontiguousarray(zxy, dtype=np.float64)
    if t.ndim != 2 or t.shape[1] != 3:
        raise ValueError("%s should be an (n, 3) table of scaled z, x, y, got shape %s" % (what, t.shape))
    return t


def assign_nearest(spots_zxy, cands_zxy):
    """``ia3_assign_nearest_dev``: per row of ``spots_zxy`` the index of its nearest row of ``cands_zxy``
    (``np.argmin(cdist(spots_zxy, cands_zxy), axis=1)``, int32)."""
    s, c = _scaled_table(spots_zxy, "spots"), _scaled_table(cands_zxy, "candidates")
    owner = np.empty(len(s), dtype=np.int32)
    check(lib().ia3_assign_nearest_dev(ptr(s), len(s), ptr(c), len(c), ptr(owner)))
    return owner


def select_chromosomes(spots_zxy, round_start, cands_zxy, loss_th, return_owner=False, times=False):
    """``ia3_select_chromosomes_dev``: dict with ``removed`` (original indices in removal order), ``removed_lost`` (their
    lost rounds when removed), ``lost`` (per candidate: the final count of a kept one, the count at its removal of a removed
    one), ``visits``, ``empty`` (every candidate was removed), and on request ``owner`` (final owner per spot) and
    ``times_ms`` (upload, first pass, removal loop)."""
    s, c = _scaled_table(spots_zxy, "spots"), _scaled_table(cands_zxy, "candidates")
    rs = np.ascontiguousarray(round_start, dtype=np.int32).ravel()
    if len(rs) < 1 or rs[0] != 0 or rs[-1] != len(s) or (np.diff(rs) < 0).any():
        raise ValueError("round_start should rise from 0 to the number of spots (%d)" % len(s))
    removed, removed_lost = np.empty(len(c), dtype=np.int32), np.empty(len(c), dtype=np.int32)
    lost = np.empty(len(c), dtype=np.int32)
    owner = np.empty(len(s), dtype=np.int32) if return_owner else None
    n, visits, t = C.c_int(0), C.c_int64(0), np.zeros(3, dtype=np.float64)
    rc = check(lib().ia3_select_chromosomes_dev(ptr(s), ptr(rs), len(rs) - 1, ptr(c), len(c), float(loss_th),
                                                ptr(removed), ptr(removed_lost), C.byref(n), ptr(lost),
                                                None if owner is None else ptr(owner), C.byref(visits),
                                                ptr(t) if times else None), allow=(IA3_SELECT_EMPTY,))
    removed, removed_lost = removed[:n.value].copy(), removed_lost[:n.value].copy()
    lost[removed] = removed_lost
    out = dict(removed=removed, removed_lost=removed_lost, lost=lost, visits=int(visits.value),
               empty=rc == IA3_SELECT_EMPTY)
    if return_owner:
        out["owner"] = owner
    if times:
        out["times_ms"] = t
    return out


PICK_KEYS = PICK_MAX_CHANNELS + 1        # keys per kind in the flat [kind][key] tables of ia3_pick_*
PICK_KINDS = ("ct", "lc", "int")         # kind 0, 1, 2: centre distance, local-centre distance, intensity
PICK_ROWS_PICKS, PICK_ROWS_PREV, PICK_ROWS_REF = 0, 1, 2
(PICK_GET_PICKS, PICK_GET_PREV, PICK_GET_SEL_SCORES, PICK_GET_PICK_INDEX, PICK_GET_SCORES, PICK_GET_MIDS,
 PICK_GET_CAND_DISTS, PICK_GET_REF_CT, PICK_GET_REF_LOCAL, PICK_GET_REF_INT) = range(10)
PICK_NITER_MAX = 15                      # cum_val's niter_max (picking.py:1879)


def cum_vals(sorted_vals, targets):
    """``ia3_pick_cum_vals_dev``: per target the last ``mid`` of the reference's ``cum_val`` search (int32)."""
    v = np.ascontiguousarray(sorted_vals, dtype=np.float64).ravel()
    t = np.ascontiguousarray(targets, dtype=np.float64).ravel()
    if len(v) == 0:
        raise IndexError("index 0 is out of bounds for axis 0 with size 0")
    mids = np.empty(len(t), dtype=np.int32)
    check(lib().ia3_pick_cum_vals_dev(ptr(v), len(v), ptr(t), len(t), ptr(mids)))
    return mids


def pick_search_nodes(n):
    """``mid`` of every node that a ``cum_val`` search in ``n`` sorted values can visit, indexed by heap number (root 1, a
    true compare goes to 2 * node + 1; -1: not reachable).  At most 2^16 entries whatever ``n`` is: the search stops after
    16 iterations.  One level of (m, M) pairs per pass."""
    n = int(n)
    if n < 1:
        raise IndexError("index 0 is out of bounds for axis 0 with size 0")
    node, m, M = np.array([1], dtype=np.int64), np.array([0], dtype=np.int64), np.array([n - 1], dtype=np.int64)
    found = []
    for it in range(PICK_NITER_MAX + 1):
        mid = (m + M) >> 1
        found.append((node, mid))
        if it == PICK_NITER_MAX:
            break
        node = np.concatenate([2 * node + 1, 2 * node])
        m, M = np.concatenate([mid, m]), np.concatenate([M, mid])
        live = M - m >= 2
        node, m, M = node[live], m[live], M[live]
        if len(node) == 0:
            break
    size = 2
    while size <= int(found[-1][0].max()):
        size *= 2
    mids = np.full(size, -1, dtype=np.int64)
    for node, mid in found:
        mids[node] = mid
    return mids


def pick_log_tables(n):
    """(``np.log(mid / n)``, ``np.log(1 - mid / n)``) per heap number of ``pick_search_nodes(n)``, with ``mid = 0.5`` where the
    node's mid is 0 (picking.py:1895-1899) and NaN for a number that no search reaches: this host's ``np.log``."""
    mids = pick_search_nodes(n)
    v = mids.astype(np.float64)
    v[mids == 0] = 0.5
    v = v / float(n)
    v[mids < 0] = np.nan
    with np.errstate(invalid="ignore"):
        return np.log(v), np.log(1 - v)


class PickPopulation(Owner):
    """A population of P chromosomes x R regions with its candidate spots resident in HBM (owner of an
    ``ia3_pick_population`` handle), and on it the steps of the reference's population picker (picking.py:1567-2342).
    Keys of the reference arrays are channel numbers ``0..n_channels-1`` and ``n_channels`` for 'all'."""

    def __init__(self, handle, P, R, n, n_channels):
        self._h = handle
        self.P, self.R, self.n, self.n_channels = P, R, n, n_channels
        self.lengths = np.full((3, PICK_KEYS), -1, dtype=np.int32)   # of the resident sorted reference arrays
        self._logs = {}                                             # (kind, key) -> (length, log table)

    @classmethod
    def upload(cls, cands, region_start, row_1d, P, R, channel=None, n_channels=0):
        """``cands``: (n, 4) float64 (h, z, x, y in nm) packed in (chromosome, region) order; ``region_start``: P*R + 1
        offsets; ``row_1d``: P*R flags, 1 where the entry was ONE 1-D row; ``channel``: R small ints or None."""
        t = np.ascontiguousarray(cands, dtype=np.float64).reshape(-1, 4)
        rs = np.ascontiguousarray(region_start, dtype=np.int32).ravel()
        fl = np.ascontiguousarray(row_1d, dtype=np.uint8).ravel()
        P, R = int(P), int(R)
        if len(rs) != P * R + 1 or len(fl) != P * R:
            raise ValueError("PickPopulation.upload: %d offsets and %d flags for %d x %d regions" % (len(rs), len(fl), P, R))
        ch = None
        if channel is not None:
            ch = np.ascontiguousarray(channel, dtype=np.int32).ravel()
            if len(ch) != R:
                raise ValueError("PickPopulation.upload: %d channels for %d regions" % (len(ch), R))
        h = C.c_void_p()
        check(lib().ia3_pick_create(ptr(t), len(t), ptr(rs), ptr(fl), P, R,
                                    None if ch is None else ptr(ch), int(n_channels) if ch is not None else 0, C.byref(h)))
        return cls(h, P, R, len(t), int(n_channels) if ch is not None else 0)

    def _rows(self, rows):
        t = np.ascontiguousarray(rows, dtype=np.float64)
        if t.size != self.P * self.R * 4:
            raise ValueError("a (%d, %d, 4) table is required, got shape %s" % (self.P, self.R, t.shape))
        return t

    def set_rows(self, which, rows):
        check(lib().ia3_pick_set_rows(self._h, int(which), ptr(self._rows(rows))))

    def pick_by_intensity(self):
        check(lib().ia3_pick_by_intensity_dev(self._h))

    @staticmethod
    def _window(win_start, win_idx, R):
        ws = np.ascontiguousarray(win_start, dtype=np.int32).ravel()
        wi = np.ascontiguousarray(win_idx, dtype=np.int32).ravel()
        if len(ws) != R + 1 or ws[-1] != len(wi):
            raise ValueError("a window table of %d + 1 offsets is required" % R)
        return ws, wi

    def _centers(self, centers):
        if centers is None:
            return None
        c = np.ascontiguousarray(centers, dtype=np.float64)
        if c.shape != (self.P, 3):
            raise ValueError("centres should be (%d, 3), got %s" % (self.P, c.shape))
        return c

    def reference(self, win_start, win_idx, split=False, centers=None, ref_is_picks=True):
        """E-step on the resident picks; returns the (3, PICK_KEYS) lengths of the sorted reference arrays (-1: not made)."""
        ws, wi = self._window(win_start, win_idx, self.R)
        c = self._centers(centers)
        lengths = np.full((3, PICK_KEYS), -1, dtype=np.int32)
        check(lib().ia3_pick_reference_dev(self._h, ptr(ws), ptr(wi), 1 if split else 0, None if c is None else ptr(c),
                                           1 if ref_is_picks else 0, ptr(lengths)))
        self.lengths = lengths
        return lengths

    def set_sorted(self, kind, key, values):
        v = np.ascontiguousarray(values, dtype=np.float64).ravel()
        check(lib().ia3_pick_set_sorted(self._h, int(kind), int(key), ptr(v), len(v)))
        self.lengths[kind, key] = len(v)

    def scores(self, win_start, win_idx, split_int=False, split_dist=False, center_weight=1.0, local_weight=1.0, centers=None,
               ref_is_picks=True, dist_only=False):
        """M-step with the resident reference arrays.  The log tables of the arrays a score reads are made here from their
        lengths (kept while a length stays the same).  IndexError when such an array is empty, as in the reference."""
        ws, wi = self._window(win_start, win_idx, self.R)
        c = self._centers(centers)
        tabs, sizes, keep = (C.c_void_p * (3 * PICK_KEYS))(), np.zeros(3 * PICK_KEYS, dtype=np.int32), []
        if not dist_only:
            for kind in range(3):
                if (kind == 0 and center_weight == 0) or (kind == 1 and local_weight == 0):
                    continue
                split = split_int if kind == 2 else split_dist
                for key in (range(self.n_channels) if split else (self.n_channels,)):
                    n = int(self.lengths[kind, key])
                    if n < 1:
                        raise IndexError("index 0 is out of bounds for axis 0 with size 0")
                    if self._logs.get((kind, key), (None,))[0] != n:
                        lo, lo1 = pick_log_tables(n)
                        self._logs[(kind, key)] = (n, np.ascontiguousarray(lo if kind == 2 else lo1))
                    t = self._logs[(kind, key)][1]
                    keep.append(t)
                    tabs[kind * PICK_KEYS + key] = t.ctypes.data
                    sizes[kind * PICK_KEYS + key] = len(t)
        check(lib().ia3_pick_scores_dev(self._h, ptr(ws), ptr(wi), 1 if split_int else 0, 1 if split_dist else 0,
                                        float(center_weight), float(local_weight), None if c is None else ptr(c),
                                        1 if ref_is_picks else 0, tabs, ptr(sizes), 1 if dist_only else 0))

    def difference(self):
        """(rows whose pick moved by less than 0.01, rows whose distance is not NaN) between the previous and the current
        picks: the 8-byte record of ``ia3_pick_difference_dev``."""
        out = np.zeros(2, dtype=np.int32)
        check(lib().ia3_pick_difference_dev(self._h, ptr(out)))
        return int(out[0]), int(out[1])

    def download(self, what):
        PR, n = self.P * self.R, self.n
        shape, dt = {PICK_GET_PICKS: ((self.P, self.R, 4), np.float64), PICK_GET_PREV: ((self.P, self.R, 4), np.float64),
                     PICK_GET_SEL_SCORES: ((self.P, self.R), np.float64), PICK_GET_PICK_INDEX: ((self.P, self.R), np.int32),
                     PICK_GET_SCORES: ((n,), np.float64), PICK_GET_MIDS: ((n, 3), np.int32),
                     PICK_GET_CAND_DISTS: ((n, 2), np.float64), PICK_GET_REF_CT: ((self.P, self.R), np.float64),
                     PICK_GET_REF_LOCAL: ((self.P, self.R), np.float64), PICK_GET_REF_INT: ((self.P, self.R), np.float64)}[what]
        out = np.empty(shape, dtype=dt)
        check(lib().ia3_pick_download(self._h, int(what), ptr(out)))
        return out

    def sorted_reference(self, kind, key):
        n = int(self.lengths[kind, key])
        if n < 0:
            raise KeyError((kind, key))
        out = np.empty(n, dtype=np.float64)
        check(lib().ia3_pick_download_sorted(self._h, int(kind), int(key), ptr(out)))
        return out

    def _release(self, handle):
        lib().ia3_pick_free(handle)


def poly_columns(order):
    """Columns of ``generate_polynomial_data`` for three coordinates and ``order``."""
    order = int(order)
    return (order + 1) * (order + 2) * (order + 3) // 6


def poly_field(constants, orders, ref_center, shape, dtype=np.float64):
    """``ia3_poly_field_dev``: device pointer (``c_void_p``, free with ``ia3_buffer_free``) of the (3,) + shape field of
    the per-axis polynomial ``constants`` (chromatic.py:282-289), float64 or float32."""
    dt = np.dtype(dtype)
    if dt not in (np.dtype(np.float32), np.dtype(np.float64)):
        raise TypeError("a polynomial field is float32 or float64, got %s" % dt)
    if len(constants) != 3 or len(orders) != 3 or len(ref_center) != 3 or len(shape) != 3:
        raise ValueError("a polynomial field takes three axes: constants, orders, ref_center and shape of length 3")
    cs = [np.ascontiguousarray(c, dtype=np.float64).ravel() for c in constants]
    flat = np.ascontiguousarray(np.concatenate(cs))
    ncol = np.array([len(c) for c in cs], dtype=np.int32)
    od = np.array([int(o) for o in orders], dtype=np.int32)
    rc = np.ascontiguousarray(ref_center, dtype=np.float64)
    p = C.c_void_p()
    check(lib().ia3_poly_field_dev(ptr(flat), ptr(ncol), ptr(od), ptr(rc), int(shape[0]), int(shape[1]), int(shape[2]),
                                   1 if dt == np.float32 else 2, C.byref(p)))
    return p


def bleedthrough_profile(consts, present, order, ref_center, shape, mean_z=True, invert=True, dtype=np.float64):
    """``ia3_bleedthrough_profile_dev``: device pointer (``c_void_p``, for ``DeviceBuffer.adopt``) of the (C, C, X, Y)
    (``mean_z``) or (C, C, Z, X, Y) bleedthrough profile of bleedthrough.py:451-486.  ``consts``: (C, C, n_cols) float64,
    ``consts[tar, ref]`` the polynomial of the slope profile from channel ref into channel tar; ``present``: (C, C), 0 for
    a direction whose profile is zero; the diagonal is 1 whatever is given there.  ``invert``: every C x C matrix is
    replaced by its inverse; ``np.linalg.LinAlgError("Singular matrix")`` when one has a zero pivot, as ``np.linalg.inv``
    raises for the first such pixel (``.n_singular`` holds their number)."""
    dt = np.dtype(dtype)
    if dt not in (np.dtype(np.float32), np.dtype(np.float64)):
        raise TypeError("a bleedthrough profile is float32 or float64, got %s" % dt)
    cs = np.ascontiguousarray(consts, dtype=np.float64)
    pr = np.ascontiguousarray(np.asarray(present) != 0, dtype=np.uint8)
    if cs.ndim != 3 or cs.shape[0] != cs.shape[1] or pr.shape != cs.shape[:2]:
        raise ValueError("a bleedthrough profile takes (C, C, n_cols) constants and a (C, C) present table")
    order = int(order)
    if 0 <= order <= 3 and cs.shape[2] != poly_columns(order):
        raise ValueError("%d constants given for order %d, %d expected" % (cs.shape[2], order, poly_columns(order)))
    if len(ref_center) != 3 or len(shape) != 3:
        raise ValueError("a bleedthrough profile takes ref_center and shape of the three axes z, x, y")
    rc = np.ascontiguousarray(ref_center, dtype=np.float64)
    p, ns = C.c_void_p(), C.c_int64(0)
    check(lib().ia3_bleedthrough_profile_dev(ptr(cs), ptr(pr), int(cs.shape[0]), order, ptr(rc),
                                            int(shape[0]), int(shape[1]), int(shape[2]), 1 if mean_z else 0,
                                            1 if invert else 0, 1 if dt == np.float32 else 2, C.byref(p), C.byref(ns)))
    if ns.value > 0:
        lib().ia3_buffer_free(p)
        err = np.linalg.LinAlgError("Singular matrix")
        err.n_singular = int(ns.value)
        raise err
    return p


def profile_enable(on=True):
    check(lib().ia3_profile_enable(1 if on else 0))


def profile_collect():
    """{kernel: (launches, total_ms)} measured with HIP events on the library stream since the last call."""
    buf = C.create_string_buffer(1 << 16)
    check(lib().ia3_profile_collect(buf, len(buf)))
    out = {}
    for line in buf.value.decode().splitlines():
        name, n, ms = line.rsplit(",", 2)
        out[name] = (int(n), float(ms))
    return out


def gaussian_taps(sigma, truncate=4.0):
    """scipy.ndimage._filters._gaussian_kernel1d(order=0) — the taps SciPy would use, from NumPy on
    this host, handed to the kernels verbatim."""
    sigma = float(sigma)
    radius = int(float(truncate) * sigma + 0.5)
    x = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    return np.ascontiguousarray(phi / phi.sum(), dtype=np.float64), radius


def make_seed_params(th_seed, gfilt_size=0.75, background_gfilt_size=7.5, filt_size=3, min_edge_distance=2,
                     use_dynamic_th=True, dynamic_niters=10, min_dynamic_seeds=1, remove_hot_pixel=True,
                     hot_pixel_th=3, max_num_seeds=None):
    """Build an ia3_seed_params (+ the arrays it points to, which the caller must keep alive)."""
    keep = []
    p = SeedParams()
    p.th_seed = float(th_seed)
    # NumPy >= 2 promotion: a Python float/int threshold is a weak scalar (compare in float32), a
    # NumPy float64 scalar is strong (compare in float64); float32/16 scalars compare in float32.
    strong64 = isinstance(th_seed, np.floating) and np.dtype(type(th_seed)).itemsize >= 8
    p.th_compare_f32 = 0 if strong64 else 1
    p.gfilt_size = float(gfilt_size) if gfilt_size else 0.0
    p.background_gfilt_size = float(background_gfilt_size) if background_gfilt_size else 0.0
    p.filt_size = int(filt_size)
    p.min_edge_distance = int(np.ceil(min_edge_distance)) if min_edge_distance > 0 else 0
    p.use_dynamic_th = 1 if use_dynamic_th else 0
    p.dynamic_niters = int(dynamic_niters)
    p.min_dynamic_seeds = int(min_dynamic_seeds)
    p.remove_hot_pixel = 1 if remove_hot_pixel else 0
    p.hot_pixel_th = int(np.ceil(hot_pixel_th))   # counts >= th (fitting.py:136) on integers
    p.max_num_seeds = int(max_num_seeds) if (max_num_seeds is not None and max_num_seeds > 0) else 0
    if p.gfilt_size > 0:
        w, r = gaussian_taps(p.gfilt_size)
        keep.append(w)
        p.w_front, p.r_front = ptr(w), r
    if p.background_gfilt_size > 0:
        w, r = gaussian_taps(p.background_gfilt_size)
        keep.append(w)
        p.w_back, p.r_back = ptr(w), r
    return p, keep


def make_fit_params(radius_fit=5, min_delta_center=1., max_delta_center=2.5, n_max_iter=10, max_dist_th=0.1,
                    min_w=0.5, max_w=4, init_w=1.5, model_variant=0, init_w_zxy=(1.35, 1.9, 1.9)):
    p = FitParams()
    p.model_variant = int(model_variant)
    for k in range(3):
        p.init_w_zxy[k] = float(init_w_zxy[k])
    p.radius_fit = int(radius_fit)
    p.min_delta_center = float(min_delta_center)
    p.max_delta_center = float(max_delta_center)
    p.n_max_iter = int(n_max_iter)
    p.max_dist_th = float(max_dist_th)
    p.min_w, p.max_w, p.init_w = float(min_w), float(max_w), float(init_w)
    return p


def fit_fovs(ims, seed_params, fit_params, in_flight=4, capacity=16384):
    """``ia3_fit_fovs`` on a list of same-shape, same-dtype images (ndarrays and/or resident ``DeviceStack``s):
    list of (M,11) float32 tables in input order + per-image dicts (n_seeds, n_iter, fits, nfev, voxel_evals).
    One C call; uploads, filters and fits of different images overlap on library-owned threads and streams."""
    ims = list(ims)
    if not ims:
        return [], []
    arrs = [im if isinstance(im, DeviceStack) else as_stack_array(im) for im in ims]
    shape, dt = tuple(arrs[0].shape), np.dtype(arrs[0].dtype)
    for a in arrs:
        if tuple(a.shape) != shape or np.dtype(a.dtype) != dt:
            raise ValueError("fit_fovs: every image of a batch must have the same shape and dtype")
    code = IA3_F32 if dt == np.float32 else IA3_U16
    n = len(arrs)
    while True:
        jobs = (FovJob * n)()
        rows = [np.empty((capacity, 11), dtype=np.float32) for _ in range(n)]
        for j, a, r in zip(jobs, arrs, rows):
            if isinstance(a, DeviceStack):
                j.dev = a._h
            else:
                j.host = a.ctypes.data
            j.rows, j.capacity = r.ctypes.data, capacity
        rc = lib().ia3_fit_fovs(jobs, n, code, shape[0], shape[1], shape[2], C.byref(seed_params), C.byref(fit_params),
                                int(in_flight))
        need = max(j.n_rows for j in jobs)
        if rc == IA3_ECAPACITY and need > capacity:   # a row table was too small (the seed stage reports the same code
            capacity = need                           # for "too many candidates", with n_rows = 0: that one is an error)
            continue
        check(rc)
        break
    tables = [r[:j.n_rows].copy() for j, r in zip(jobs, rows)]
    info = [dict(n_seeds=j.n_seeds, n_iter=j.n_iter, fits=j.fits, nfev=j.nfev, voxel_evals=j.voxel_evals) for j in jobs]
    return tables, info


def process_movies(params, movies, drifts_in=None, measure_drift=True, want_images=False, capacity=16384):
    """``ia3_process_movies``: ``movies`` = raw (frames, X, Y) uint16 arrays and/or .dax paths (``(path, offset_bytes,
    big_endian)`` tuples or plain strings), all of the layout ``params`` (a filled ``MovieParams``) describes.  Returns
    one dict per movie: ``tables`` (list of (M,11) float32 per selected channel), ``drift``, ``drift_flag``, ``images``
    (list of (Z,X,Y) uint16 or None), ``n_seeds``, ``n_iter``, ``ms`` (host wall time per stage).  ``drifts_in``: per movie
    a drift to use (or start from); ``measure_drift``: bool or per-movie list."""
    n = len(movies)
    if n == 0:
        return []
    n_sel = int(params.n_sel)
    Z, X, Y = int(params.Z), int(params.X), int(params.Y)
    keep = []
    while True:
        jobs = (MovieJob * n)()
        rows = [[np.empty((capacity, 11), dtype=np.float32) for _ in range(n_sel)] for _ in range(n)]
        images = [[np.empty((Z, X, Y), dtype=np.uint16) if want_images else None for _ in range(n_sel)] for _ in range(n)]
        for k, (j, m) in enumerate(zip(jobs, movies)):
            if isinstance(m, np.ndarray):
                if m.dtype != np.uint16 or m.ndim != 3 or tuple(m.shape) != (int(params.frames), X, Y):
                    raise TypeError("the raw movie should be a (%d, %d, %d) uint16 array" % (int(params.frames), X, Y))
                a = np.ascontiguousarray(m)
                keep.append(a)
                j.host_raw = a.ctypes.data
            else:
                path, off, big = (m, 0, False) if isinstance(m, (str, bytes)) else m
                j.path = os.fsencode(path)
                j.offset_bytes, j.big_endian = int(off), 1 if big else 0
            md = measure_drift[k] if isinstance(measure_drift, (list, tuple)) else measure_drift
            j.measure_drift = 1 if md else 0
            if drifts_in is not None and drifts_in[k] is not None:
                for a_ in range(3):
                    j.drift_in[a_] = float(drifts_in[k][a_])
            for s_ in range(n_sel):
                j.rows[s_], j.capacity[s_] = rows[k][s_].ctypes.data, capacity
                if want_images:
                    j.images_out[s_] = images[k][s_].ctypes.data
        rc = lib().ia3_process_movies(jobs, n, C.byref(params))
        need = max(max(j.n_rows[s_] for s_ in range(n_sel)) for j in jobs)
        if rc == IA3_ECAPACITY and need > capacity:
            capacity = need
            continue
        check(rc)
        break
    out = []
    for k, j in enumerate(jobs):
        out.append(dict(tables=[rows[k][s_][:j.n_rows[s_]].copy() for s_ in range(n_sel)],
                        drift=np.array([j.drift[0], j.drift[1], j.drift[2]]), drift_flag=int(j.drift_flag),
                        images=images[k] if want_images else None,
                        n_seeds=[int(j.n_seeds[s_]) for s_ in range(n_sel)], n_iter=[int(j.n_iter[s_]) for s_ in range(n_sel)],
                        ms=dict(upload=j.t_upload_ms, correct=j.t_correct_ms, fit=j.t_fit_ms),
                        stamps=[float(v) for v in j.stamps]))
    return out


DIST_NANMEDIAN, DIST_NANMEAN, DIST_CONTACT = 0, 1, 2      # IA3_DIST_*


class DistancePopulation(Owner):
    """The (rows, 3) float64 coordinate tables of M chromosome copies resident in HBM (owner of an
    ``ia3_dist_population`` handle), and on it the summaries of structure_tools/distance.py over pairs of copies."""

    def __init__(self, handle, rows):
        self._h = handle
        self.rows = rows                  # rows of every copy (int32)
        self.M = len(rows)

    @classmethod
    def upload(cls, tables):
        """``tables``: a sequence of M (rows, 3) arrays, one per chromosome copy (z, x, y)."""
        ts = []
        for t in tables:
            a = np.ascontiguousarray(t, dtype=np.float64)
            if a.ndim != 2 or a.shape[1] != 3:
                raise ValueError("DistancePopulation.upload: a (rows, 3) table is required, got shape %s" % (a.shape,))
            ts.append(a)
        if len(ts) < 1:
            raise ValueError("DistancePopulation.upload: no tables")
        rows = np.array([len(a) for a in ts], dtype=np.int32)
        start = np.zeros(len(ts) + 1, dtype=np.int32)
        np.cumsum(rows, out=start[1:])
        packed = np.ascontiguousarray(np.concatenate(ts, axis=0)) if start[-1] > 0 else np.zeros((1, 3))
        h = C.c_void_p()
        check(lib().ia3_dist_create(ptr(packed), ptr(start), len(ts), C.byref(h)))
        return cls(h, rows)

    def summary(self, pair_a, pair_b, function=DIST_NANMEDIAN, contact_th=None, same=False, return_counts=False):
        """``ia3_dist_summary_dev`` over the pairs (pair_a[n], pair_b[n]): the (Ra, Rb) float64 summary, with
        ``return_counts`` also (n_finite, n_contact) as int32.  ValueError for no pair, an index outside the population and
        pairs whose tables differ in rows."""
        a = np.ascontiguousarray(pair_a, dtype=np.int32).ravel()
        b = np.ascontiguousarray(pair_b, dtype=np.int32).ravel()
        if len(a) != len(b) or len(a) < 1:
            raise ValueError("DistancePopulation.summary: %d and %d copy indices (at least one pair is required)" % (len(a), len(b)))
        if a.min() < 0 or b.min() < 0 or a.max() >= self.M or b.max() >= self.M:
            raise ValueError("DistancePopulation.summary: a copy index outside 0..%d" % (self.M - 1))
        Ra, Rb = int(self.rows[a[0]]), int(self.rows[b[0]])
        if (self.rows[a] != Ra).any() or (self.rows[b] != Rb).any():
            raise ValueError("DistancePopulation.summary: the tables of the pairs do not all have %d and %d rows" % (Ra, Rb))
        if Ra < 1 or Rb < 1:
            raise ValueError("DistancePopulation.summary: a %d x %d summary" % (Ra, Rb))
        out = np.empty((Ra, Rb), dtype=np.float64)
        nf = np.empty((Ra, Rb), dtype=np.int32) if return_counts else None
        nc = np.empty((Ra, Rb), dtype=np.int32) if return_counts else None
        th = float("nan") if contact_th is None else float(contact_th)
        check(lib().ia3_dist_summary_dev(self._h, ptr(a), ptr(b), len(a), Ra, Rb, 1 if same else 0, int(function),
                                         th, ptr(out), None if nf is None else ptr(nf), None if nc is None else ptr(nc)))
        return (out, nf, nc) if return_counts else out

    def _release(self, handle):
        lib().ia3_dist_free(handle)


def dist_contact_stack(stack, contact_th, return_counts=False):
    """``ia3_dist_contact_stack_dev``: ``contact_prob`` along axis 0 of an (N, ...) float64 stack."""
    v = np.ascontiguousarray(stack, dtype=np.float64)
    if v.ndim < 1 or v.shape[0] < 1 or v.size < 1:
        raise ValueError("dist_contact_stack: a stack of at least one value is required, got shape %s" % (v.shape,))
    N, K = v.shape[0], v.size // v.shape[0]
    prob = np.empty(v.shape[1:], dtype=np.float64)
    nf, nc = np.empty(v.shape[1:], dtype=np.int32), np.empty(v.shape[1:], dtype=np.int32)
    check(lib().ia3_dist_contact_stack_dev(ptr(v), N, K, float(contact_th), ptr(prob), ptr(nf), ptr(nc)))
    return (prob, nf, nc) if return_counts else prob


class DensityLayout(object):
    """The loci of a list of cells (each a dict ``chr -> (H, R, 3)`` coordinates) packed for ``ia3_density_create``, host
    arrays only.  Points run cell by cell, inside a cell chromosome by chromosome in the dict's order, then homolog, then
    region.  ``copy_of`` numbers the (chromosome, homolog) of a point within its cell, ``locus_of`` is ``first_id[chr] +
    region`` with the chromosomes laid out in the order of ``chrs`` and ``regions[chr]`` the largest R any cell has;
    ``least_regions[chr]`` is the smallest, the bound an index of the labels must respect.  ``blocks[cell]`` lists
    ``(chr, H, R, first point)``."""

    def __init__(self, cells, chrs):
        chrs = list(chrs)
        known = set(chrs)
        self.chrs = chrs
        self.regions = {c: 0 for c in chrs}
        self.least_regions = {}
        tables, self.blocks = [], []
        start = [0]
        for i, cell in enumerate(cells):
            blocks, at = [], start[-1]
            for c, zxys in cell.items():
                if c not in known:
                    raise KeyError(c)
                a = np.asarray(zxys, dtype=np.float64)
                if a.ndim != 3 or a.shape[0] < 1 or a.shape[1] < 1 or a.shape[2] != 3:
                    raise ValueError("cell %d, chromosome %r: (homologs >= 1, regions >= 1, 3) coordinates are required, got "
                                     "shape %s" % (i, c, a.shape))
                H, R = a.shape[:2]
                self.regions[c] = max(self.regions[c], R)
                self.least_regions[c] = min(self.least_regions.get(c, R), R)
                blocks.append((c, H, R, at))
                tables.append(a.reshape(-1, 3))
                at += H * R
            if at - start[-1] > IA3_DENSITY_MAX_CELL:
                raise ValueError("cell %d has %d loci (at most %d are built)" % (i, at - start[-1], IA3_DENSITY_MAX_CELL))
            self.blocks.append(blocks)
            start.append(at)
        self.first_id, n = {}, 0
        for c in chrs:
            self.first_id[c] = n
            n += self.regions[c]
        self.n_loci = n
        self.cell_start = np.array(start, dtype=np.int32)
        self.n_points = int(start[-1])
        self.zxys = np.ascontiguousarray(np.concatenate(tables, axis=0)) if tables else np.zeros((0, 3))
        self.copy_of = np.zeros(self.n_points, dtype=np.int32)
        self.locus_of = np.zeros(self.n_points, dtype=np.int32)
        self.n_copies = np.zeros(len(self.blocks), dtype=np.int32)
        for i, blocks in enumerate(self.blocks):
            copy = 0
            for c, H, R, at in blocks:
                self.copy_of[at:at + H * R] = copy + np.repeat(np.arange(H, dtype=np.int32), R)
                self.locus_of[at:at + H * R] = self.first_id[c] + np.tile(np.arange(R, dtype=np.int32), H)
                copy += H
            self.n_copies[i] = copy

    def multiplicities(self, chr_2_AB_dict):
        """The (n_loci, 2) uint8 table of a scoring call: how often region r of a chromosome is listed under 'A' and 'B'.
        KeyError for a chromosome of the cells that the dict lacks; IndexError for an index outside 0..R-1 (negative ones
        too: the reference wraps them for trans and drops them for cis, which is not restated) or one that is no integer."""
        mult = np.zeros((max(self.n_loci, 1), 2), dtype=np.uint8)
        for c, R in self.least_regions.items():
            labels = chr_2_AB_dict[c]
            for k, key in enumerate(('A', 'B')):
                idx = np.asarray(labels[key])
                if idx.size == 0:
                    continue
                if idx.dtype.kind not in "iu":
                    raise IndexError("chr_2_AB_dict[%r][%r]: arrays used as indices must be of integer type" % (c, key))
                idx = idx.astype(np.int64).ravel()
                if idx.min() < 0 or idx.max() >= R:
                    raise IndexError("chr_2_AB_dict[%r][%r]: an index outside 0..%d" % (c, key, R - 1))
                n = np.bincount(idx, minlength=self.regions[c])
                if n.max() > 255:
                    raise NotImplementedError("chr_2_AB_dict[%r][%r] lists a region %d times (at most 255 are built)" % (c, key, n.max()))
                mult[self.first_id[c]:self.first_id[c] + self.regions[c], k] = n
        return mult

    def unpack(self, values):
        """``values``: (2, n_points).  The reference's list of per-cell dicts ``chr -> {'A': (H, R), 'B': (H, R)}``."""
        return [{c: {'A': values[0, at:at + H * R].reshape(H, R).copy(), 'B': values[1, at:at + H * R].reshape(H, R).copy()}
                 for c, H, R, at in blocks} for blocks in self.blocks]


class DensityPopulation(Owner):
    """The loci of a list of cells resident in HBM (owner of an ``ia3_density_population`` handle); ``scores`` gives every
    locus its A and B sums for one set of labels, sigmas and flags without moving a coordinate again."""

    def __init__(self, handle, layout):
        self._h = handle
        self.layout = layout
        self.n_points = layout.n_points

    @classmethod
    def upload(cls, cells, chr_2_AB_dict_layout):
        """``cells``: dicts ``chr -> (H, R, 3)``; ``chr_2_AB_dict_layout``: the chromosomes that the label dicts of the
        scoring calls will name, in the order of the locus table (a ``chr_2_AB_dict`` itself will do).  KeyError for a
        chromosome of a cell that is not among them."""
        layout = cells if isinstance(cells, DensityLayout) else DensityLayout(cells, chr_2_AB_dict_layout)
        if len(layout.blocks) < 1:
            raise ValueError("DensityPopulation.upload: no cells")
        h = C.c_void_p()
        zxys = layout.zxys if layout.n_points else np.zeros((1, 3))
        copy_of = layout.copy_of if layout.n_points else np.zeros(1, dtype=np.int32)
        locus_of = layout.locus_of if layout.n_points else np.zeros(1, dtype=np.int32)
        check(lib().ia3_density_create(ptr(zxys), ptr(layout.cell_start), ptr(copy_of), ptr(locus_of), len(layout.blocks),
                                       max(layout.n_loci, 1), C.byref(h)))
        return cls(h, layout)

    def scores(self, mult, s2, use_cis=False, use_trans=True, exclude_self=True):
        """``ia3_density_scores_dev``: (sums (2, n_points) float64, counts (2, n_points) int32), row 0 for A and row 1 for
        B, from the (n_loci, 2) uint8 multiplicities and the three squared sigmas."""
        mult = np.ascontiguousarray(mult, dtype=np.uint8)
        s2 = np.ascontiguousarray(s2, dtype=np.float64)
        if mult.shape != (max(self.layout.n_loci, 1), 2) or s2.shape != (3,):
            raise ValueError("DensityPopulation.scores: multiplicities of shape %s and sigmas of shape %s" % (mult.shape, s2.shape))
        sums = np.zeros((2, self.n_points), dtype=np.float64)
        counts = np.zeros((2, self.n_points), dtype=np.int32)
        check(lib().ia3_density_scores_dev(self._h, ptr(mult), ptr(s2), 1 if use_cis else 0, 1 if use_trans else 0,
                                           1 if exclude_self else 0, ptr(sums), ptr(counts)))
        return sums, counts

    def _release(self, handle):
        lib().ia3_density_free(handle)


def cloud_sources(pos, h, sig, size_fold):
    """The (n, 8) float64 source table of ``ia3_cloud_render``: pos[3], h, sig[3], size_fold per row; ``h``, ``sig`` (three
    values) and ``size_fold`` are one value for all rows or one per row.  ValueError, before any device call, for a
    position, sigma or size_fold that is not finite and for a box ``int(max(sig) * size_fold) + 1`` outside 1 ..
    IA3_CLOUD_MAX_S + 1 (the library refuses the same)."""
    pos = np.asarray(pos, dtype=np.float64)
    if pos.ndim != 2 or pos.shape[1] != 3:
        raise ValueError("cloud sources: positions of shape (n, 3) are required, got %s" % (pos.shape,))
    n = len(pos)
    t = np.empty((n, 8), dtype=np.float64)
    t[:, :3] = pos
    try:
        t[:, 3] = np.asarray(h, dtype=np.float64)
        t[:, 4:7] = np.asarray(sig, dtype=np.float64)
        t[:, 7] = np.asarray(size_fold, dtype=np.float64)
    except ValueError:
        raise ValueError("cloud sources: h of shape () or (n,), sig of shape (3,) or (n, 3) and size_fold of shape () or (n,) "
                         "are required for %d positions" % n)
    if not np.isfinite(t[:, [0, 1, 2, 4, 5, 6, 7]]).all():
        raise ValueError("cloud sources: a position, sigma or size_fold that is not finite")
    with np.errstate(over="ignore"):
        s = t[:, 4:7].max(axis=1) * t[:, 7] if n else np.zeros(0)
    if not ((s > -1.0) & (s < IA3_CLOUD_MAX_S + 1.0)).all():
        raise ValueError("cloud sources: a box of int(max(sig) * size_fold) + 1 outside 1 to %d" % (IA3_CLOUD_MAX_S + 1))
    return t


def _cloud_call(sources, image_start, shape, rounding):
    sources = np.ascontiguousarray(sources, dtype=np.float64)
    start = np.ascontiguousarray(image_start, dtype=np.int32)
    shape = tuple(int(v) for v in shape)
    if sources.ndim != 2 or sources.shape[1] != 8 or start.ndim != 1 or len(start) < 2 or start[0] != 0 \
            or start[-1] != len(sources) or (np.diff(start) < 0).any():
        raise ValueError("cloud render: an (n, 8) source table and offsets 0 .. n of its images are required")
    if len(shape) != 3 or min(shape) < 1 or max(shape) > IA3_CLOUD_MAX_DIM or len(start) - 1 > IA3_CLOUD_MAX_IMAGES:
        raise ValueError("cloud render: %d images of shape %s" % (len(start) - 1, shape))
    dt = np.dtype(np.float64 if rounding is None else rounding)
    if dt not in (np.dtype(np.float64), np.dtype(np.float32)):
        raise ValueError("cloud render: rounding is None (float64) or numpy.float32, got %s" % (rounding,))
    if len(sources) == 0:
        sources = np.zeros((1, 8))     # a pointer for the call; no row of it is named
    return sources, start, shape, dt, (IA3_CLOUD_F32 if dt == np.float32 else IA3_CLOUD_F64)


def cloud_render(sources, image_start, shape, rounding=None, init=None):
    """``ia3_cloud_render``: the (n_images,) + shape images of the source table ``sources`` (``cloud_sources``), image i from
    the rows image_start[i] .. image_start[i + 1] in that order, started from ``init`` (same shape) or from zeros.
    ``rounding`` None: float64 sums; ``numpy.float32``: float32 images rounded after every source."""
    sources, start, shape, dt, mode = _cloud_call(sources, image_start, shape, rounding)
    out = np.empty((len(start) - 1,) + shape, dtype=dt)
    if init is not None:
        init = np.ascontiguousarray(init, dtype=dt)
        if init.shape != out.shape:
            raise ValueError("cloud render: init of shape %s for images of shape %s" % (init.shape, out.shape))
    check(lib().ia3_cloud_render(ptr(sources), ptr(start), len(start) - 1, shape[0], shape[1], shape[2], mode,
                                 None if init is None else C.c_void_p(init.ctypes.data), C.c_void_p(out.ctypes.data)))
    return out


class CloudImages(Owner):
    """Device memory for the images of ``ia3_cloud_render_dev`` (an ``ia3_buffer_alloc`` allocation of ``capacity`` bytes),
    kept by a caller that renders many cells one after the other."""
    _handle = "devptr"

    def __init__(self, capacity):
        self.capacity = int(capacity)
        p = C.c_void_p()
        check(lib().ia3_buffer_alloc(max(self.capacity, 8), C.byref(p)))
        self.devptr = p

    def render(self, sources, image_start, shape, rounding=None):
        """Zero the first n_images images of ``shape``, render into them and download them."""
        sources, start, shape, dt, mode = _cloud_call(sources, image_start, shape, rounding)
        out = np.empty((len(start) - 1,) + shape, dtype=dt)
        if out.nbytes > self.capacity:
            raise ValueError("CloudImages.render: %d bytes of images in a buffer of %d" % (out.nbytes, self.capacity))
        check(lib().ia3_cloud_render_dev(ptr(sources), ptr(start), len(start) - 1, shape[0], shape[1], shape[2], mode, 1,
                                         self.devptr))
        check(lib().ia3_buffer_download(self.devptr, out.nbytes, C.c_void_p(out.ctypes.data)))
        return out

    def _release(self, handle):
        lib().ia3_buffer_free(handle)


def cloud_gauss_ker(sig, s, disp):
    """``ia3_cloud_gauss_ker``: the (s + 1,) * 3 float64 kernel of the reference's ``gauss_ker(sig, s, disp)``."""
    sig = np.ascontiguousarray(sig, dtype=np.float64)
    disp = np.ascontiguousarray(disp, dtype=np.float64)
    s = int(s)
    if sig.shape != (3,) or disp.shape != (3,):
        raise ValueError("gauss_ker: three sigmas and three displacements are required, got %s and %s" % (sig.shape, disp.shape))
    if s < 0 or s > IA3_CLOUD_MAX_KER_S:
        raise ValueError("gauss_ker: sxyz %d (0 to %d)" % (s, IA3_CLOUD_MAX_KER_S))
    out = np.empty((s + 1,) * 3, dtype=np.float64)
    check(lib().ia3_cloud_gauss_ker(ptr(sig), s, ptr(disp), ptr(out)))
    return out


# ---- domain distances of traced chromosomes (csrc/domain.hip) -----------------------------------------------------------------
DOMAIN_WINDOW_METRICS = {'median': IA3_DOMAIN_WINDOW_MEDIAN, 'mean': IA3_DOMAIN_WINDOW_MEAN, 'ks': IA3_DOMAIN_WINDOW_KS,
                         'normed_insulation': IA3_DOMAIN_WINDOW_NORMED_INSULATION, 'insulation': IA3_DOMAIN_WINDOW_INSULATION}
DOMAIN_DIST_METRICS = {'median': IA3_DOMAIN_DIST_MEDIAN, 'absolute_median': IA3_DOMAIN_DIST_ABSOLUTE_MEDIAN,
                       'insulation': IA3_DOMAIN_DIST_INSULATION}


def domain_rows(R):
    """The number of loci of a copy: ValueError below 1, NotImplementedError above IA3_DOMAIN_MAX_R."""
    R = int(R)
    if R < 1:
        raise ValueError("domain distances: a chromosome of %d loci" % R)
    if R > IA3_DOMAIN_MAX_R:
        raise NotImplementedError("domain distances: %d loci (at most %d are built: a quadruple's entries are counted in "
                                  "32 bits and a distance map is one allocation)" % (R, IA3_DOMAIN_MAX_R))
    return R


def domain_normalization(normalization, R):
    """The (R, R) float64 normalisation map, or None.  ValueError for another shape and, with the words of
    scipy.spatial.distance.squareform (which the reference runs on its diagonal blocks), for a map that is not symmetric
    or whose diagonal is not zero."""
    if normalization is None:
        return None
    m = np.ascontiguousarray(normalization, dtype=np.float64)
    if m.shape != (R, R):
        raise ValueError("Wrong shape of normalization:%s, should be equal to %s" % (m.shape, (R, R)))
    if not (m == m.T).all():
        raise ValueError("Distance matrix 'X' must be symmetric.")
    if not (m[np.diag_indices(R)] == 0).all():
        raise ValueError("Distance matrix 'X' diagonal must be zero.")
    return m


def domain_window_sizes(window_sizes):
    """1 to IA3_DOMAIN_MAX_WINDOWS window sizes as int32 (``int(wd)`` each): ValueError for none, too many or one below 1,
    NotImplementedError for one above IA3_DOMAIN_MAX_WINDOW."""
    wds = np.array([int(w) for w in np.atleast_1d(window_sizes)], dtype=np.int64)
    if wds.ndim != 1 or len(wds) < 1 or len(wds) > IA3_DOMAIN_MAX_WINDOWS:
        raise ValueError("sliding windows: %d window sizes (1 to %d per call)" % (wds.size, IA3_DOMAIN_MAX_WINDOWS))
    if wds.min() < 1:
        raise ValueError("sliding windows: window size %d" % wds.min())
    if wds.max() > IA3_DOMAIN_MAX_WINDOW:
        raise NotImplementedError("sliding windows: window size %d (at most %d is built: a wavefront keeps the two sets of a "
                                  "window in LDS)" % (wds.max(), IA3_DOMAIN_MAX_WINDOW))
    return wds.astype(np.int32)


def domain_quads(quads, N, R):
    """(Q, 5) int32 entries (copy, s1, e1, s2, e2) of a population of N copies x R loci: ValueError for another shape, no
    entry, a copy outside 0..N-1 and bounds that are not 0 <= s <= e <= R (a slice the reference would clip or wrap)."""
    q = np.asarray(quads)
    if q.ndim != 2 or q.shape[1] != 5 or len(q) < 1:
        raise ValueError("domain entries: a (Q, 5) table of (copy, s1, e1, s2, e2) with Q >= 1 is required, got shape %s" % (q.shape,))
    q = q.astype(np.int64)
    if q[:, 0].min() < 0 or q[:, 0].max() >= N:
        raise ValueError("domain entries: a copy outside 0..%d" % (N - 1))
    if q[:, 1:].min() < 0 or q[:, 1:].max() > R or (q[:, 2] < q[:, 1]).any() or (q[:, 4] < q[:, 3]).any():
        raise ValueError("domain entries: bounds that are not 0 <= start <= end <= %d" % R)
    return np.ascontiguousarray(q, dtype=np.int32)


class DomainPopulation(Owner):
    """N chromosome copies x R loci resident in HBM (owner of an ``ia3_domain_create`` handle): their (N, R, 3) float64
    coordinates, NaN for a missing locus, or one (R, R) distance map (N = 1); optionally one (R, R) normalisation map shared
    by all copies.  ``slide``, ``distances`` and ``contacts`` are the three kernels of domain_tools/distance.py."""

    def __init__(self, handle, N, R, is_matrix, has_norm):
        self._h = handle
        self.N, self.R, self.is_matrix, self.has_norm = N, R, is_matrix, has_norm

    @classmethod
    def _create(cls, data, N, R, is_matrix, normalization):
        norm = domain_normalization(normalization, R)
        h = C.c_void_p()
        check(lib().ia3_domain_create(ptr(data.reshape(-1)), N, R, 1 if is_matrix else 0, None if norm is None else ptr(norm.reshape(-1)),
                                      C.byref(h)))
        return cls(h, N, R, is_matrix, norm is not None)

    @classmethod
    def upload(cls, zxys, normalization=None):
        """``zxys``: (N, R, 3) coordinates, or (R, 3) for one copy."""
        a = np.ascontiguousarray(zxys, dtype=np.float64)
        if a.ndim == 2:
            a = a[None]
        if a.ndim != 3 or a.shape[2] != 3 or a.shape[0] < 1:
            raise ValueError("DomainPopulation.upload: (N, R, 3) coordinates are required, got shape %s" % (a.shape,))
        return cls._create(a, a.shape[0], domain_rows(a.shape[1]), False, normalization)

    @classmethod
    def upload_matrix(cls, mat, normalization=None):
        """``mat``: one (R, R) distance map; entry [i, j] is the distance the reference reads as ``_mat[i, j]``."""
        a = np.ascontiguousarray(mat, dtype=np.float64)
        if a.ndim != 2 or a.shape[0] != a.shape[1]:
            raise ValueError("DomainPopulation.upload_matrix: an (R, R) distance map is required, got shape %s" % (a.shape,))
        return cls._create(a, 1, domain_rows(a.shape[0]), True, normalization)

    def _use_norm(self, normalize):
        if normalize is None:
            return 1 if self.has_norm else 0
        if normalize and not self.has_norm:
            raise ValueError("DomainPopulation: the population holds no normalisation map")
        return 1 if normalize else 0

    def slide(self, window_sizes, metric='median', normalize=False):
        """``ia3_domain_slide_dev``: the (N, W, R) float64 sliding-window distances of every copy."""
        wds = domain_window_sizes(window_sizes)
        if metric not in DOMAIN_WINDOW_METRICS:
            raise ValueError(f"Wrong input _dist_metric")
        use_norm = self._use_norm(normalize)
        out = np.empty((self.N, len(wds), self.R), dtype=np.float64)
        check(lib().ia3_domain_slide_dev(self._h, ptr(wds), len(wds), DOMAIN_WINDOW_METRICS[metric], use_norm, ptr(out.reshape(-1))))
        return out

    def distances(self, quads, metric='median', allow_minus=True, normalize=None):
        """``ia3_domain_dists_dev``: (values (Q,) float64, int_zero (Q,) bool) of the (Q, 5) entries (copy, s1, e1, s2, e2);
        ``int_zero`` marks where the reference returns Python's integer 0.  ``normalize`` None: divide when the population
        holds a normalisation map."""
        q = domain_quads(quads, self.N, self.R)
        if metric not in DOMAIN_DIST_METRICS:
            raise ValueError("Wrong input _metric type:%s" % (metric,))
        use_norm = self._use_norm(normalize)
        out = np.empty(len(q), dtype=np.float64)
        flag = np.empty(len(q), dtype=np.int32)
        check(lib().ia3_domain_dists_dev(self._h, ptr(q.reshape(-1)), len(q), DOMAIN_DIST_METRICS[metric], 1 if allow_minus else 0,
                                         use_norm, ptr(out), ptr(flag)))
        return out, flag != 0

    def contacts(self, quads, contact_th=400, return_counts=False):
        """``ia3_domain_contacts_dev``: per entry the share of the block [s1:e1, s2:e2] that is <= ``contact_th``; with
        ``return_counts`` also the int32 counts."""
        q = domain_quads(quads, self.N, self.R)
        freq = np.empty(len(q), dtype=np.float64)
        cnt = np.empty(len(q), dtype=np.int32)
        check(lib().ia3_domain_contacts_dev(self._h, ptr(q.reshape(-1)), len(q), float(contact_th), ptr(freq), ptr(cnt)))
        return (freq, cnt) if return_counts else freq

    def _release(self, handle):
        lib().ia3_domain_free(handle)


# ---- chromosomal spot scores (csrc/score.hip) ---------------------------------------------------------------------------------
SCORE_REF_METRICS = {'median': IA3_SCORE_REF_MEDIAN, 'mean': IA3_SCORE_REF_MEAN, 'rg': IA3_SCORE_REF_RG, 'cdf': IA3_SCORE_REF_CDF}
SCORE_VALUE, SCORE_LOG, SCORE_NEG_INF, SCORE_NAN_IN = 0, 1, 2, 4   # the class byte of a value (ia3_score_scores_dev)
_SCORE_CDF_KINDS = (IA3_SCORE_KIND_DIST_CDF, IA3_SCORE_KIND_INT_CDF, IA3_SCORE_KIND_CUM_PROB)


def score_half(local_size):
    """``int((local_size - 1) / 2)`` of _local_distance: IndexError below 0 (np.delete of an empty range, as in the
    reference), NotImplementedError above what IA3_SCORE_MAX_LOCAL gives."""
    half = int((local_size - 1) / 2)
    if half < 0:
        raise IndexError("index %d is out of bounds for axis 0 with size 0" % half)
    if half > (IA3_SCORE_MAX_LOCAL - 1) // 2:
        raise NotImplementedError("spot scores: local_size %s (at most %d is built: a spot gathers the rows of at most %d "
                                  "neighbouring regions)" % (local_size, IA3_SCORE_MAX_LOCAL, IA3_SCORE_MAX_LOCAL - 1))
    return half


def score_step(neighbor_step):
    step = int(neighbor_step)
    if abs(step) > 2**31 - 1:
        raise ValueError("spot scores: neighbor_step %d" % step)
    return step


def score_table(rows_list, ids_list, what):
    """The CSR form of one table: ((n, 4) float64 rows (h, z, x, y), (n,) int64 region ids, (C + 1,) int32 offsets).
    ``ids_list[c]`` None: 0 .. len - 1.  IndexError for rows that are not 2-D with four columns or more or whose ids differ
    in number, ValueError for no chromosome, a chromosome without a row and an id outside int32, NotImplementedError for
    more than IA3_SCORE_MAX_PER_REGION rows of one region id in a chromosome."""
    rows_list = list(rows_list)
    ids_list = [None] * len(rows_list) if ids_list is None else list(ids_list)
    if len(rows_list) < 1 or len(ids_list) != len(rows_list):
        raise ValueError("spot scores: %d %s tables with %d lists of ids" % (len(rows_list), what, len(ids_list)))
    rows, ids, start = [], [], [0]
    for c, (r, i) in enumerate(zip(rows_list, ids_list)):
        r = np.asarray(r, dtype=np.float64)
        if r.ndim != 2 or r.shape[1] < 4:
            raise IndexError("Wrong shape of %s spots of chromosome %d, should be 2d array of (h, z, x, y, ...) rows, got %s" % (what, c, r.shape))
        i = np.arange(len(r), dtype=np.int64) if i is None else np.asarray(i)
        if i.ndim != 1 or len(i) != len(r):
            raise IndexError("Wrong input length of %s spots and ids of chromosome %d, length should match!" % (what, c))
        if len(r) < 1:
            raise ValueError("spot scores: chromosome %d has no %s spot" % (c, what))
        if i.dtype.kind == 'f' and not np.isfinite(i).all():
            raise ValueError("spot scores: a region id of chromosome %d is not a number" % c)
        i = i.astype(np.int64)
        if i.min() < -2**31 or i.max() > 2**31 - 1:
            raise ValueError("spot scores: a region id of chromosome %d lies outside int32" % c)
        most = int(np.unique(i, return_counts=True)[1].max())
        if most > IA3_SCORE_MAX_PER_REGION:
            raise NotImplementedError("spot scores: %d %s spots of one region in chromosome %d (at most %d are built: a median is "
                                      "ranked within one wavefront)" % (most, what, c, IA3_SCORE_MAX_PER_REGION))
        rows.append(r[:, :4])
        ids.append(i)
        start.append(start[-1] + len(r))
    if start[-1] > 2**31 - 1:
        raise NotImplementedError("spot scores: %d %s rows in one population" % (start[-1], what))
    return np.ascontiguousarray(np.concatenate(rows)), np.ascontiguousarray(np.concatenate(ids)), np.array(start, dtype=np.int32)


def score_values(x, kind, ref_array=None, ref_scalar=0.0, weight=1.0, limit_lo=-np.inf, limit_hi=np.inf):
    """``ia3_score_values_dev``: (values, class bytes, number of reference values that are not NaN) for the 1-D float64 ``x``
    against one reference: ``ref_array`` for the cdf kinds, ``ref_scalar`` for the linear ones."""
    x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1)
    val = np.empty(len(x), dtype=np.float64)
    cls = np.empty(len(x), dtype=np.uint8)
    cnt = np.zeros(1, dtype=np.int32)
    if len(x) == 0:
        return val, cls, 0
    ref = None
    if kind in _SCORE_CDF_KINDS:
        ref = np.ascontiguousarray(ref_array, dtype=np.float64).reshape(-1)
        if len(ref) < 1:
            raise ValueError("spot scores: an empty reference array")
    check(lib().ia3_score_values_dev(None if ref is None else ptr(ref), 0 if ref is None else len(ref), float(ref_scalar), ptr(x), len(x), int(kind),
                                     float(weight), float(limit_lo), float(limit_hi), ptr(val), ptr(cls), ptr(cnt)))
    return val, cls, int(cnt[0])


class ScorePopulation(Owner):
    """C traced chromosomes resident in HBM (owner of an ``ia3_score_create`` handle): per chromosome its candidate spots and
    its currently selected spots, (h, z, x, y) rows in pixels with a region id each, optionally a centre in pixels, and the
    pixel sizes.  ``replace_selected`` swaps the selected spots, which is all an EM iteration of the per-cell pickers
    changes."""

    def __init__(self, handle, cand_ids, cand_start, sel_start):
        self._h = handle
        self.cand_ids, self.cand_start, self.sel_start = cand_ids, cand_start, sel_start
        self.C, self.N, self.S = len(cand_start) - 1, int(cand_start[-1]), int(sel_start[-1])

    @classmethod
    def upload(cls, cand_spots, cand_ids, sel_spots, sel_ids=None, chr_centers=None, distance_zxy=(200, 108, 108)):
        """Lists of C tables each; ``chr_centers``: None, or a list of C entries, each None or a (z, x, y) centre in pixels."""
        cand, cid, cstart = score_table(cand_spots, cand_ids, "candidate")
        sel, sid, sstart = score_table(sel_spots, sel_ids, "selected")
        n_chrom = len(cstart) - 1
        if len(sstart) - 1 != n_chrom:
            raise ValueError("spot scores: %d candidate tables and %d selected tables" % (n_chrom, len(sstart) - 1))
        dz = np.ascontiguousarray(distance_zxy, dtype=np.float64).reshape(-1)
        if len(dz) != 3:
            raise ValueError("spot scores: distance_zxy of %d values" % len(dz))
        centers, has = None, None
        if chr_centers is not None:
            chr_centers = list(chr_centers)
            if len(chr_centers) != n_chrom:
                raise ValueError("spot scores: %d centres for %d chromosomes" % (len(chr_centers), n_chrom))
            centers, has = np.zeros((n_chrom, 3)), np.zeros(n_chrom, dtype=np.int32)
            for c, ctr in enumerate(chr_centers):
                if ctr is not None:
                    centers[c] = np.asarray(ctr, dtype=np.float64).reshape(3)
                    has[c] = 1
        h = C.c_void_p()
        check(lib().ia3_score_create(ptr(cand.reshape(-1)), ptr(cid), ptr(cstart), ptr(sel.reshape(-1)), ptr(sid), ptr(sstart),
                                     None if centers is None else ptr(centers.reshape(-1)), None if has is None else ptr(has), n_chrom, ptr(dz),
                                     C.byref(h)))
        return cls(h, cid, cstart, sstart)

    def replace_selected(self, sel_spots, sel_ids=None):
        sel, sid, sstart = score_table(sel_spots, sel_ids, "selected")
        if len(sstart) - 1 != self.C:
            raise ValueError("spot scores: %d selected tables for %d chromosomes" % (len(sstart) - 1, self.C))
        check(lib().ia3_score_replace_selected(self._h, ptr(sel.reshape(-1)), ptr(sid), ptr(sstart)))
        self.sel_start, self.S = sstart, int(sstart[-1])

    @staticmethod
    def _ref_metric(ref_metric):
        m = str(ref_metric).lower()
        if m not in SCORE_REF_METRICS:
            raise ValueError(f"Not supported yet!")
        return SCORE_REF_METRICS[m]

    def references(self, ref_metric='median', local_size=5, intensity_th=0., ignore_nan=True):
        """``ia3_score_refs_dev``: (arrays, counts (C, 4), scalars (C, 4)); ``arrays[c][a]`` is what the reference keeps of the
        centre, local and neighbour distances and the intensities of chromosome c (with ``ignore_nan`` without NaNs, the
        fallback value where nothing is left: its count is -1)."""
        metric, half = self._ref_metric(ref_metric), score_half(local_size)
        arrays = np.empty((4, self.S), dtype=np.float64)
        counts = np.empty((self.C, 4), dtype=np.int32)
        scalars = np.empty((self.C, 4), dtype=np.float64)
        check(lib().ia3_score_refs_dev(self._h, metric, half, float(intensity_th), 1 if ignore_nan else 0, ptr(arrays.reshape(-1)),
                                       ptr(counts.reshape(-1)), ptr(scalars.reshape(-1))))
        s = self.sel_start
        return [[arrays[a, s[c]:s[c] + abs(counts[c, a])].copy() for a in range(4)] for c in range(self.C)], counts, scalars

    def geometry(self, local_size=5, neighbor_step=1, invalid_dist=np.nan):
        """(5, N) float64: the centre, local, forward, reverse and mean neighbour distance of every candidate."""
        half, step = score_half(local_size), score_step(neighbor_step)
        geom = np.empty((5, self.N), dtype=np.float64)
        check(lib().ia3_score_scores_dev(self._h, -1, 0, half, step, float(invalid_dist), 0., 1, None, 0., 0., ptr(geom.reshape(-1)), None, None, None))
        return geom

    def scores(self, score_metric='cdf', ref_metric=None, local_size=5, intensity_th=0., ignore_nan=True, weights=(1., 1., 1., 1.),
               distance_limits=(0, np.inf)):
        """``ia3_score_scores_dev``: (values (4, N), class bytes (4, N), reference counts (C, 4)) of the centre, local,
        neighbour and intensity score of every candidate, up to the argument of np.log."""
        score_metric = str(score_metric).lower()
        if score_metric not in ('linear', 'cdf'):
            raise ValueError(f"metric type:{score_metric} has not been supported yet!")
        kind = IA3_SCORE_KIND_DIST_CDF if score_metric == 'cdf' else IA3_SCORE_KIND_DIST_LINEAR
        metric = self._ref_metric(score_metric if ref_metric is None else ref_metric)
        if (metric == IA3_SCORE_REF_CDF) != (score_metric == 'cdf'):
            raise ValueError("spot scores: the %s metric with %s references" % (score_metric, ref_metric))
        half = score_half(local_size)
        w = np.ascontiguousarray([float(v) for v in weights], dtype=np.float64)
        if len(w) != 4:
            raise ValueError("spot scores: %d weights" % len(w))
        lo, hi = float(min(distance_limits)), float(max(distance_limits))
        val = np.empty((4, self.N), dtype=np.float64)
        cls = np.empty((4, self.N), dtype=np.uint8)
        cnt = np.empty((self.C, 4), dtype=np.int32)
        check(lib().ia3_score_scores_dev(self._h, kind, metric, half, 1, float('nan'), float(intensity_th), 1 if ignore_nan else 0, ptr(w), lo, hi,
                                         None, ptr(val.reshape(-1)), ptr(cls.reshape(-1)), ptr(cnt.reshape(-1))))
        return val, cls, cnt

    def neighbor_lists(self, neighbor_step=1, invalid_dist=np.nan):
        """neighboring_distances(use_median=False) of every chromosome: two lists of C float64 vectors (forward, reverse)."""
        step = score_step(neighbor_step)
        nf, nr = np.zeros(self.N, dtype=np.int64), np.zeros(self.N, dtype=np.int64)
        for c in range(self.C):
            a, b = self.cand_start[c], self.cand_start[c + 1]
            ids = self.cand_ids[a:b]
            u, k = np.unique(ids, return_counts=True)

            def count(q):
                at = np.minimum(np.searchsorted(u, q), len(u) - 1)
                return np.where(u[at] == q, k[at], 0)
            f = count(ids + step)
            nf[a:b] = np.where(f > 0, f, 1)
            nr[a:b] = np.where(f > 0, count(ids - step), 1)
        if max(nf.sum(), nr.sum()) > 2**31 - 1:
            raise NotImplementedError("spot scores: %d neighbour distances in one call" % max(nf.sum(), nr.sum()))
        of = np.concatenate([[0], np.cumsum(nf)]).astype(np.int32)
        orv = np.concatenate([[0], np.cumsum(nr)]).astype(np.int32)
        fwd, rev = np.empty(max(of[-1], 1), dtype=np.float64), np.empty(max(orv[-1], 1), dtype=np.float64)
        check(lib().ia3_score_neighbor_lists_dev(self._h, step, float(invalid_dist), ptr(of), ptr(orv), ptr(fwd), ptr(rev)))
        s = self.cand_start
        return ([fwd[of[s[c]]:of[s[c + 1]]].copy() for c in range(self.C)], [rev[orv[s[c]]:orv[s[c + 1]]].copy() for c in range(self.C)])

    def _release(self, handle):
        lib().ia3_score_free(handle)


# ---- per-cell spot pickers (csrc/cellpick.hip) ----------------------------------------------------------------------------------
def cellpick_cdf_table(ref, weight, limit_lo, limit_hi):
    """(sorted reference values, table) of one chromosome's 'cdf' neighbour reference: ``table[k]`` is distance_score of a
    distance with k reference values ``<=`` it, ``np.log(1 - _cum_prob) * weight`` (-inf where nothing is left), in the
    arithmetic of csrc/ia3_score.h sc_cum_prob with this host's ``np.log``."""
    s = np.sort(np.asarray(ref, dtype=np.float64).reshape(-1))
    n = len(s)
    with np.errstate(all="ignore"):
        p = np.arange(n + 1) / np.float64(n)
        min_p = np.float64(np.searchsorted(s, limit_lo, side='right')) / np.float64(n)
        max_p = np.float64(np.searchsorted(s, limit_hi, side='right')) / np.float64(n)
        r = p - min_p if max_p <= min_p else (p - min_p) / (max_p - min_p)
        r[r <= 0.] = 0.
        r[np.isnan(r)] = 1. / np.float64(n)
        r[r >= 1.] = 1.
        cdf = 1 - r
        table = np.full(n + 1, -np.inf)
        table[cdf > 0] = np.log(cdf[cdf > 0]) * float(weight)
    return s, table


class CellPickPopulation(Owner):
    """The candidate spots of many cells resident in HBM (owner of an ``ia3_cellpick_create`` handle): CSR over cell x region
    x chromosome of (h, z, x, y) rows in pixels, the cells' region ids and chromosome coordinates and the pixel sizes.
    ``merge`` makes the merged lists on the device, where they stay; ``forward`` takes per-spot scores up and brings
    dynamic scores and pointers back.  The host keeps the callers' full-width rows, from which results are put together."""

    def __init__(self, handle):
        self._h = handle
        self.merged = False

    @classmethod
    def upload(cls, cells, distance_zxy):
        """``cells``: a list of ``(cell_cand_spots, region_ids, chrom_coords)``; ``cell_cand_spots[region][chromosome]`` is a
        table of spots (intensity, z, x, y, ...) or empty, ``chrom_coords`` a list of (z, x, y) in pixels or None.
        NotImplementedError for more than IA3_CELLPICK_MAX_CHROM chromosomes in a cell."""
        MC = IA3_CELLPICK_MAX_CHROM
        if len(cells) < 1:
            raise ValueError("cell pickers: no cell")
        dz = np.ascontiguousarray(distance_zxy, dtype=np.float64).reshape(-1)
        if len(dz) != 3:
            raise ValueError("cell pickers: distance_zxy of %d values" % len(dz))
        self = cls(None)
        self.n_cells = len(cells)
        self.n_chrom = np.zeros(self.n_cells, dtype=np.int32)
        self.has_coords = np.zeros(self.n_cells, dtype=np.int32)
        self.coords = np.zeros((self.n_cells, MC, 3))
        self.region_ids, self.width, self.cell_rows = [], [], []
        counts, parts, region_start = [], [], [0]
        for k, (cand, ids, coords) in enumerate(cells):
            C_k = len(coords) if coords is not None else len(cand[0])
            if C_k > MC:
                raise NotImplementedError("cell pickers: %d chromosomes in cell %d (at most %d are built: a spot of the next region "
                                          "walks up to C^C index tuples)" % (C_k, k, MC))
            if C_k < 1 or len(cand) < 1:
                raise ValueError("cell pickers: cell %d has no chromosome or no region" % k)
            if len(ids) != len(cand):
                raise ValueError("cell pickers: cell %d has %d regions and %d region ids" % (k, len(cand), len(ids)))
            self.n_chrom[k] = C_k
            if coords is not None:
                self.has_coords[k] = 1
                self.coords[k, :C_k] = np.array([np.asarray(c, dtype=np.float64).reshape(3) for c in coords])
            ids = np.array(ids)
            if ids.dtype.kind == 'f' and not np.isfinite(ids).all():
                raise ValueError("cell pickers: a region id of cell %d is not a number" % k)
            ids = ids.astype(np.int64)
            if len(ids) and (ids.min() < -2**31 or ids.max() > 2**31 - 1):
                raise ValueError("cell pickers: a region id of cell %d lies outside int32" % k)
            self.region_ids.append(ids)
            width, rows_k = None, []
            for r, lists in enumerate(cand):
                if len(lists) != C_k:
                    raise NotImplementedError("cell pickers: region %d of cell %d has %d spot lists for %d chromosomes" % (r, k, len(lists), C_k))
                for c in range(MC):
                    if c >= C_k or len(lists[c]) == 0:
                        counts.append(0)
                        continue
                    t = np.array(lists[c], dtype=np.float64)
                    if t.ndim != 2 or t.shape[1] < 4:
                        raise IndexError("cell pickers: the spots of region %d, chromosome %d of cell %d have shape %s" % (r, c, k, t.shape))
                    if width is None:
                        width = t.shape[1]
                    elif width != t.shape[1]:
                        raise ValueError(f"_spot object length is not unique, exit")
                    rows_k.append(t)
                    counts.append(len(t))
            self.width.append(11 if width is None else width)
            self.cell_rows.append(np.concatenate(rows_k) if rows_k else np.zeros((0, self.width[-1])))
            parts.append(self.cell_rows[-1][:, :4])
            region_start.append(region_start[-1] + len(cand))
        self.G = region_start[-1]
        self.region_start = np.array(region_start, dtype=np.int32)
        total = np.concatenate([[0], np.cumsum(np.array(counts, dtype=np.int64))])
        if total[-1] > 2**31 - 1 or self.G * MC + 1 > 2**31 - 1:
            raise NotImplementedError("cell pickers: %d candidate rows in one population" % total[-1])
        self.cand_start = total.astype(np.int32)
        self.cell_cand0 = self.cand_start[self.region_start * MC]
        self.rows = np.ascontiguousarray(np.concatenate(parts)) if total[-1] else np.zeros((0, 4))
        self.row_nan = np.ascontiguousarray(np.concatenate([np.isnan(t).any(axis=1) for t in self.cell_rows]).astype(np.uint8))
        self.region_cell = np.repeat(np.arange(self.n_cells), np.diff(self.region_start))
        per_region = self.cand_start[MC::MC] - self.cand_start[:-1:MC]
        cap = np.concatenate([[0], np.cumsum(per_region.astype(np.int64) + 2 * self.n_chrom[self.region_cell])])
        if cap[-1] * MC > 2**31 - 1:   # the planes of a forward pass, at their most
            raise NotImplementedError("cell pickers: room for %d merged rows in one population" % cap[-1])
        self.cap_start = cap.astype(np.int32)
        self.cap = int(cap[-1])
        self.planes = int(self.n_chrom.max())             # score / pointer planes of a forward pass
        self.dzxy = dz
        h = C.c_void_p()
        rows = self.rows.reshape(-1) if self.rows.size else np.zeros(1)
        nan = self.row_nan if self.row_nan.size else np.zeros(1, dtype=np.uint8)
        check(lib().ia3_cellpick_create(ptr(rows), ptr(nan), ptr(self.cand_start), ptr(self.region_start), ptr(self.n_chrom),
                                        ptr(self.coords.reshape(-1)), ptr(self.has_coords), ptr(self.cap_start), self.n_cells, self.G, ptr(dz), C.byref(h)))
        self._h = h
        return self

    def merge(self, intensity_th=0., hard_intensity_th=True, dist_th=0.1):
        """``ia3_cellpick_merge_dev``: merge_spot_list of every region; sets ``mcount`` / ``mvalid`` (G) and ``msrc``."""
        self.mcount = np.zeros(self.G, dtype=np.int32)
        self.mvalid = np.zeros(self.G, dtype=np.int32)
        self.msrc = np.zeros(max(self.cap, 1), dtype=np.int32)
        check(lib().ia3_cellpick_merge_dev(self._h, 0 if intensity_th is None else 1, 0. if intensity_th is None else float(intensity_th),
                                           1 if hard_intensity_th else 0, float(dist_th), ptr(self.mcount), ptr(self.mvalid), ptr(self.msrc)))
        self.merged = True
        # the places of the merged rows among the room the regions were given, region after region
        region = np.repeat(np.arange(self.G), np.diff(self.cap_start))
        self.mpos = np.where(np.arange(self.cap) - self.cap_start[region] < self.mcount[region])[0]
        self.mregion = region[self.mpos]
        self.mstart = np.concatenate([[0], np.cumsum(self.mcount)])     # offsets into mpos per region

    def merged_rows4(self):
        """(M, 4) rows (h, z, x, y) of all merged spots, region after region: what the device keeps."""
        src = self.msrc[self.mpos]
        out = np.zeros((len(src), 4))
        real = src >= 0
        out[real] = self.rows[src[real]]
        out[~real, 1:4] = self.coords[self.region_cell[self.mregion[~real]], -(src[~real] + 1)]
        return out

    def merged_region(self, g):
        """The merged spots of region g as the reference returns them: (K, width) rows, ``np.array([])`` for none."""
        k = self.region_cell[g]
        src = self.msrc[self.cap_start[g]:self.cap_start[g] + self.mcount[g]]
        if len(src) == 0:
            return np.array([])
        MC = IA3_CELLPICK_MAX_CHROM
        width = self.width[k] if self.cand_start[(g + 1) * MC] > self.cand_start[g * MC] else 11
        out = np.full((len(src), width), np.nan)
        for i, s in enumerate(src):
            if s >= 0:
                out[i] = self.cell_rows[k][s - self.cell_cand0[k]]
            else:
                out[i, 0] = 0
                out[i, 1:4] = self.coords[k, -(s + 1)]
        return out

    def naive(self, mode):
        """``ia3_cellpick_naive_dev``: (pick, sub), each (G, IA3_CELLPICK_MAX_CHROM)."""
        pick = np.zeros((self.G, IA3_CELLPICK_MAX_CHROM), dtype=np.int32)
        sub = np.zeros((self.G, IA3_CELLPICK_MAX_CHROM), dtype=np.int32)
        check(lib().ia3_cellpick_naive_dev(self._h, int(mode), ptr(pick.reshape(-1)), ptr(sub.reshape(-1))))
        return pick, sub

    def plan(self, vstart, vreg, vgap):
        vstart = np.ascontiguousarray(vstart, dtype=np.int32)
        vreg = np.ascontiguousarray(vreg if len(vreg) else [0], dtype=np.int32)
        vgap = np.ascontiguousarray(vgap if len(vgap) else [0], dtype=np.int64)
        check(lib().ia3_cellpick_plan(self._h, ptr(vstart), ptr(vreg), ptr(vgap)))

    def forward(self, cells, scores, score_metric, refs, weight, limit_hi, nan_mask, share):
        """``ia3_cellpick_forward_dev``.  ``scores``: (planes, cap), one plane per chromosome up to the largest number of
        chromosomes a cell of the population has; ``refs[(cell, chromosome)]``: the
        reference distance ('linear') or the (sorted values, table) of ``cellpick_cdf_table`` ('cdf').
        Returns (dy, ptr, err): the dynamic scores, the pointers (255: none) and the error code of every cell."""
        MC = IA3_CELLPICK_MAX_CHROM
        cells = np.ascontiguousarray(cells, dtype=np.int32)
        scores = np.ascontiguousarray(scores, dtype=np.float64)
        if scores.shape != (self.planes, self.cap):
            raise ValueError("cell pickers: scores of shape %s" % (scores.shape,))
        J = self.n_cells * MC
        scal, rstart, srt, tab = None, None, None, None
        if score_metric == 'linear':
            kind = IA3_SCORE_KIND_DIST_LINEAR
            scal = np.ones(J)
            for (k, c), v in refs.items():
                scal[k * MC + c] = v
        else:
            kind = IA3_SCORE_KIND_DIST_CDF
            n = np.zeros(J, dtype=np.int64)
            for (k, c), (s, t) in refs.items():
                n[k * MC + c] = len(s)
            rs = np.concatenate([[0], np.cumsum(n)])
            if rs[-1] + J > 2**31 - 1:
                raise NotImplementedError("cell pickers: %d reference values in one call" % rs[-1])
            rstart = rs.astype(np.int32)
            srt, tab = np.zeros(max(int(rs[-1]), 1)), np.zeros(int(rs[-1]) + J + 1)
            for (k, c), (s, t) in refs.items():
                j = k * MC + c
                srt[rs[j]:rs[j + 1]] = s
                tab[rs[j] + j:rs[j + 1] + j + 1] = t
        dy = np.empty((self.planes, self.cap))
        pt = np.empty((self.planes, self.cap), dtype=np.uint8)
        err = np.zeros(self.n_cells, dtype=np.int32)
        check(lib().ia3_cellpick_forward_dev(self._h, ptr(cells), len(cells), ptr(scores.reshape(-1)) if scores.size else ptr(np.zeros(1)), kind,
                                             None if scal is None else ptr(scal), None if rstart is None else ptr(rstart),
                                             None if srt is None else ptr(srt), None if tab is None else ptr(tab), float(weight), float(limit_hi),
                                             float(nan_mask), 1 if share else 0, ptr(dy.reshape(-1)) if dy.size else ptr(np.zeros(1)),
                                             ptr(pt.reshape(-1)) if pt.size else ptr(np.zeros(1, dtype=np.uint8)), ptr(err)))
        return dy, pt, err

    def _release(self, handle):
        lib().ia3_cellpick_free(handle)
