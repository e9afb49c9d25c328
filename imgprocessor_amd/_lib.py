"""ctypes binding of libimgproc_hip.so (C ABI: include/imgproc_hip.h).

The library is the product: if it is missing or cannot be loaded this module
raises — there is no CPU or numpy fallback anywhere in the package.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# IMGPROC_HIP_LIB selects another build of the SAME library (tuning A/B variants)
LIB_PATH = os.environ.get('IMGPROC_HIP_LIB') or os.path.join(_HERE, 'libimgproc_hip.so')

# enums of include/imgproc_hip.h
U8, U16, F32, F64 = 0, 1, 2, 3
INTER_NEAREST, INTER_LINEAR, INTER_CUBIC_CV, INTER_LANCZOS4, INTER_CUBIC_KEYS = 0, 1, 2, 4, 5
INTER_Q5 = 0x100
BORDER_CONSTANT, BORDER_REPLICATE, BORDER_REFLECT, BORDER_WRAP, BORDER_REFLECT101 = 0, 1, 2, 3, 4

# ipa_stencil_op of ipa_stencil_path
(STENCIL_LOCAL_STD, STENCIL_MASKED_MEAN_FILL, STENCIL_MASKED_MEDIAN, STENCIL_NAN_MAX,
 STENCIL_CLOSEST_DISTANCE, STENCIL_POS_INTENSITY_UNC, STENCIL_MEDIAN_THRESHOLD,
 STENCIL_VAR_Y_GAUSS, STENCIL_CONV_YDEP) = range(9)

# ipa_cv_table_id of ipa_cv_table
CV_TABLE_ROWS, CV_TABLE_U8_CUBIC, CV_TABLE_U8_LANCZOS4 = range(3)

# ipa_conv_op of ipa_conv_path
CONV_CONV2D, CONV_SEPCONV2D, CONV_SEPCONV2D_LDS = range(3)

# ipa_interp_op / ipa_interp_const of ipa_interp_path
(INTERP_CONST, INTERP_CROSS_FASTDIV, INTERP_CIRCULAR_FASTDIV, INTERP_FASTDIV_MUL, INTERP_POWER,
 INTERP_POINT_SPREAD_ROWS, INTERP_STAT_SAMPLES, INTERP_RESIZE_VEC4, INTERP_RESIZE_AREA,
 INTERP_RESIZE_LINEAR) = range(10)
(INTERP_K_CROSS_SEG, INTERP_K_CROSS_BALLOT_STEPS, INTERP_K_CROSS_SEARCH_PASS,
 INTERP_K_FASTDIV_SHIFT, INTERP_K_PS_WAVES, INTERP_K_PS_MAX_ROWS, INTERP_K_STAT_MAX) = range(7)

# ipa_resize_interp of ipa_resize (cv2's INTER_* numbers); the `fn` of ipa_fast_filter_stat
RESIZE_LINEAR, RESIZE_CUBIC, RESIZE_AREA, RESIZE_LANCZOS4 = 1, 2, 3, 4
STAT_MEDIAN, STAT_NANMEDIAN, STAT_MEAN, STAT_NANMEAN = range(4)

# ipa_nlf_kind of ipa_nlf_threshold_dev
NLF_BOUNDED_SQRT, NLF_CLIPPED_POLY, NLF_CONSTANT = range(3)

# ipa_extremum_mode of ipa_strided_extremum_dev
EXTREMUM_MEDIAN_MAX, EXTREMUM_MIN = range(2)

# ipa_poly_mode of ipa_poly2d_eval_dev
POLY_FILL, POLY_ALL, POLY_GRID = range(3)

# ipa_fn2d_model of ipa_fn2d_normal_dev / ipa_fn2d_eval_dev
FN2D_KW, FN2D_AOV = range(2)

# IPA_REMAP_PATH_* bits of the read-only tuning word "remap_path"
(REMAP_PATH_GATHER, REMAP_PATH_REST, REMAP_PATH_RING, REMAP_PATH_TILE, REMAP_PATH_TILE_MAP,
 REMAP_PATH_STORED, REMAP_PATH_U8_LZ_LDS, REMAP_PATH_STRIP, REMAP_PATH_STRIP_INT, REMAP_PATH_LENS_MAP,
 REMAP_PATH_FRAMES_INNER) = (1 << k for k in range(11))
# IPA_CHAIN_PATH_* bits of the read-only tuning word "chain_path"
(CHAIN_PATH_RESIDENT, CHAIN_PATH_STREAMED, CHAIN_PATH_SEP, CHAIN_PATH_TWO_LAUNCHES, CHAIN_PATH_RANK1,
 CHAIN_PATH_LENS_MAP, CHAIN_PATH_ROTATED, CHAIN_PATH_STORED, CHAIN_PATH_SPLIT, CHAIN_PATH_FRAMES_WG,
 CHAIN_PATH_PER_FRAME) = (1 << k for k in range(11))

OK, ERR_BAD_ARG, ERR_UNSUPPORTED, ERR_HIP, ERR_OOM, ERR_NO_DEVICE = 0, -1, -2, -3, -4, -5

_vp, _i, _l, _d, _sz = C.c_void_p, C.c_int, C.c_long, C.c_double, C.c_size_t
_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)

# name -> argtypes; every function returns int (ipa_status) unless noted
PROTOTYPES = {
    'ipa_version': [],
    'ipa_device_count': [C.POINTER(_i)],
    'ipa_device_pci_bus_id': [_i, C.c_char_p, C.c_size_t],
    'ipa_ctx_create': [_i, C.POINTER(_vp)],
    'ipa_ctx_destroy': [_vp],
    'ipa_ctx_synchronize': [_vp],
    'ipa_ctx_set_tuning': [_vp, C.c_char_p, _i],
    'ipa_ctx_get_tuning': [_vp, C.c_char_p, C.POINTER(_i)],
    'ipa_ctx_device_info': [_vp, C.c_char_p, _sz, C.POINTER(_i), C.POINTER(_sz)],
    'ipa_mem_info': [_vp, C.POINTER(_sz), C.POINTER(_sz)],
    'ipa_malloc': [_vp, _sz, C.POINTER(_vp)],
    'ipa_free': [_vp, _vp],
    'ipa_host_alloc': [_vp, _sz, C.POINTER(_vp)],
    'ipa_host_free': [_vp, _vp],
    'ipa_memcpy_h2d': [_vp, _vp, _vp, _sz],
    'ipa_memcpy_d2h': [_vp, _vp, _vp, _sz],
    'ipa_memcpy_d2d': [_vp, _vp, _vp, _sz],
    'ipa_memset': [_vp, _vp, _i, _sz],
    'ipa_event_create': [_vp, C.POINTER(_vp)],
    'ipa_event_destroy': [_vp, _vp],
    'ipa_event_record': [_vp, _vp],
    'ipa_event_elapsed_ms': [_vp, _vp, _vp, C.POINTER(C.c_float)],
    'ipa_build_undistort_map_dev': [_vp, _dp, _dp, _dp, _i, _i, _vp, _vp, _l],
    'ipa_build_undistort_map': [_vp, _dp, _dp, _dp, _i, _i, _vp, _vp],
    'ipa_remap_dev': [_vp, _vp, _i, _i, _i, _l, _vp, _vp, _l, _vp, _i, _i, _i, _l, _i, _l, _l,
                      _i, _i, _d],
    'ipa_remap': [_vp, _vp, _i, _i, _i, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _d],
    'ipa_cv_table': [_i, _vp, _sz],
    'ipa_undistort_dev': [_vp, _vp, _i, _i, _i, _l, _dp, _dp, _dp, _vp, _i, _i, _i, _l, _i, _l,
                          _l, _i, _i, _d],
    'ipa_undistort': [_vp, _vp, _i, _i, _i, _dp, _dp, _dp, _vp, _i, _i, _i, _i, _i, _i, _d],
    'ipa_warp_perspective_dev': [_vp, _vp, _i, _i, _i, _l, _dp, _vp, _i, _i, _i, _l, _i, _l, _l,
                                 _i, _i, _d],
    'ipa_warp_perspective': [_vp, _vp, _i, _i, _i, _dp, _vp, _i, _i, _i, _i, _i, _i, _d],
    'ipa_warp_grid_dev': [_vp, _vp, _i, _i, _i, _l, _ip, _dp, _i, _vp, _i, _i, _i, _l, _i, _l, _l,
                          _i, _i, _d],
    'ipa_warp_grid': [_vp, _vp, _i, _i, _i, _ip, _dp, _i, _vp, _i, _i, _i, _i, _i, _i, _d],
    'ipa_warp_grid_plan': [_ip, _i, _i, _i, _vp, _vp, _vp, _ip, _ip],
    'ipa_conv2d_dev': [_vp, _vp, _i, _i, _i, _l, _dp, _i, _i, _vp, _l, _vp, _l, _i, _l, _l, _i,
                       _i, _d],
    'ipa_conv2d': [_vp, _vp, _i, _i, _i, _dp, _i, _i, _vp, _vp, _i, _i, _i, _d],
    'ipa_sepconv2d_dev': [_vp, _vp, _i, _i, _i, _l, _dp, _i, _dp, _i, _vp, _l, _i, _l, _l, _i, _i,
                          _d],
    'ipa_sepconv2d': [_vp, _vp, _i, _i, _i, _dp, _i, _dp, _i, _vp, _i, _i, _i, _d],
    'ipa_extend_array_dev': [_vp, _vp, _i, _i, _i, _l, _i, _i, _i, _i, _vp, _l],
    'ipa_deinterleave_dev': [_vp, _vp, _i, _i, _i, _i, _l, _vp, _l, _l],
    'ipa_interleave_dev': [_vp, _vp, _i, _i, _i, _i, _l, _l, _vp, _l],
    'ipa_conv_ydep_dev': [_vp, _vp, _i, _i, _i, _l, _vp, _i, _i, _i, _i, _vp, _l],
    'ipa_var_y_gauss_dev': [_vp, _vp, _i, _i, _i, _l, C.c_double, C.c_double, _i,
                            C.POINTER(C.c_double), _i, _i, _i, _vp, _l],
    'ipa_local_std_dev': [_vp, _vp, _vp, _i, _i, _i, _l, _l, _i, _i, _vp, _l],
    'ipa_masked_mean_dev': [_vp, _vp, _i, _vp, _i, _i, _l, _l, _i, _i, _vp, _l],
    'ipa_masked_median_dev': [_vp, _vp, _i, _vp, _i, _i, _l, _l, _i, _i, _vp, _l],
    'ipa_nan_max_dev': [_vp, _vp, _i, _i, _i, _l, _i, _vp, _l],
    'ipa_closest_distance_dev': [_vp, _vp, _i, _i, _l, _i, _vp, _i, _l],
    'ipa_pos_intensity_unc_dev': [_vp, _vp, _i, _i, _i, _l, _vp, _vp, _l, _d, _d, _i, _vp, _l],
    'ipa_median_threshold_dev': [_vp, _vp, _i, _i, _i, _l, _d, _i, _vp, _l, _vp, _l],
    'ipa_median_threshold_size_dev': [_vp, _vp, _i, _i, _i, _l, _i, _d, _i, _vp, _l, _vp, _l],
    'ipa_stencil_path': [_i, _i, _i, _i],
    'ipa_conv_path': [_i, _i, _i, _i, _i],
    'ipa_interp_path': [_i, _d, _d, _d, _d],
    'ipa_calib_prefilter_dev': [_vp, _vp, _i, _vp, _vp, _i, _i, _l, _l, _l, _d, _vp, _l],
    'ipa_remap_conv2d_dev': [_vp, _vp, _i, _i, _i, _l, _vp, _vp, _l, _dp, _i, _i, _vp, _i, _i,
                             _i, _l, _i, _l, _l, _i, _i, _d, _i, _i],
    'ipa_undistort_conv2d_dev': [_vp, _vp, _i, _i, _i, _l, _dp, _dp, _dp, _dp, _i, _i, _vp, _i,
                                 _i, _i, _l, _i, _l, _l, _i, _i, _d, _i, _i],
    'ipa_warp_perspective_conv2d_dev': [_vp, _vp, _i, _i, _i, _l, _dp, _dp, _i, _i, _vp, _i, _i,
                                        _i, _l, _i, _l, _l, _i, _i, _d, _i, _i],
    'ipa_remap_sepconv2d_dev': [_vp, _vp, _i, _i, _i, _l, _vp, _vp, _l, _dp, _i, _dp, _i, _vp, _i,
                                _i, _i, _l, _i, _l, _l, _i, _i, _d, _i, _i],
    'ipa_undistort_sepconv2d_dev': [_vp, _vp, _i, _i, _i, _l, _dp, _dp, _dp, _dp, _i, _dp, _i, _vp,
                                    _i, _i, _i, _l, _i, _l, _l, _i, _i, _d, _i, _i],
    'ipa_warp_perspective_sepconv2d_dev': [_vp, _vp, _i, _i, _i, _l, _dp, _dp, _i, _dp, _i, _vp, _i,
                                           _i, _i, _l, _i, _l, _l, _i, _i, _d, _i, _i],
    'ipa_idw_fill_dev': [_vp, _vp, _i, _vp, _i, _i, _l, _i, _dp],
    'ipa_idw_fill': [_vp, _vp, _i, _vp, _i, _i, _i, _dp],
    'ipa_fast_idw_fill_dev': [_vp, _vp, _i, _vp, _i, _i, _l, _vp, _dp, _i, _i],
    'ipa_fast_idw_fill': [_vp, _vp, _i, _vp, _i, _i, _vp, _dp, _i, _i],
    'ipa_unstructured_idw_dev': [_vp, _vp, _i, _i, _i, _l, _dp, _dp, _dp, _i, _d],
    'ipa_unstructured_idw': [_vp, _vp, _i, _i, _i, _dp, _dp, _dp, _i, _d],
    'ipa_circular_idw_fill_dev': [_vp, _vp, _i, _vp, _i, _i, _l, _i, _d, _d, _d, _d, _d],
    'ipa_circular_idw_fill': [_vp, _vp, _i, _vp, _i, _i, _i, _d, _d, _d, _d, _d],
    'ipa_cross_avg_fill_dev': [_vp, _vp, _i, _vp, _i, _i, _l, _i, _d],
    'ipa_cross_avg_fill': [_vp, _vp, _i, _vp, _i, _i, _i, _d],
    'ipa_point_spread_idw_dev': [_vp, _vp, _i, _vp, _i, _i, _l, _i, _d, _l],
    'ipa_point_spread_idw': [_vp, _vp, _i, _vp, _i, _i, _i, _d, _l],
    'ipa_resize_dev': [_vp, _vp, _i, _i, _i, _l, _vp, _i, _i, _l, _i],
    'ipa_resize': [_vp, _vp, _i, _i, _i, _vp, _i, _i, _i],
    'ipa_fast_filter_stat_dev': [_vp, _vp, _i, _i, _i, _l, _i, _i, _i, _vp],
    'ipa_fast_filter_stat': [_vp, _vp, _i, _i, _i, _i, _i, _i, _vp],
    'ipa_ste_dev': [_vp, _vp, _i, _i, _i, _i, _l, _l, _i, _dp, _d, _vp, _vp, _vp, _l, _vp, _vp, _vp,
                    _l],
    'ipa_remove_single_pixels_dev': [_vp, _vp, _i, _i, _l, _vp, _l],
    'ipa_nl_means_dev': [_vp, _vp, _i, _i, _i, _i, _l, _l, _i, _i, _d, _d, _vp, _l, _l],
    'ipa_nan_to_zero_dev': [_vp, _vp, _i, _i, _i, _i, _l, _l],
    'ipa_nlf_signal_dev': [_vp, _vp, _i, _vp, _i, _i, _l, _l, _vp, _l, _d, _vp, _l],
    'ipa_nlf_moments_dev': [_vp, _vp, _i, _i, _i, _l, _dp],
    'ipa_nlf_bins_dev': [_vp, _vp, _i, _vp, _i, _i, _l, _l, _vp, _l, _d, _vp, _l, _dp, _i, _d, _d,
                         _i, _vp, _dp],
    'ipa_snr_map_dev': [_vp, _vp, _i, _i, _l, _dp, _vp, _l, _d, _d, _d, _vp, _l],
    'ipa_snr_bg_median_dev': [_vp, _vp, _i, _i, _i, _l, _vp, _l],
    'ipa_pair_min_dev': [_vp, _vp, _vp, _i, _i, _i, _l, _l, _vp, _l],
    'ipa_nlf_threshold_dev': [_vp, _vp, _i, _i, _l, _i, _dp, _d, _vp, _l],
    'ipa_stack_linregress_dev': [_vp, _vp, _i, _i, _i, _i, _l, _l, _dp, _d, _d, _vp, _vp, _vp, _l],
    'ipa_dark_current_eval_dev': [_vp, _vp, _vp, _i, _i, _l, _d, _d, _vp, _i, _l],
    'ipa_cast_trunc_dev': [_vp, _vp, _i, _i, _l, _vp, _i, _l],
    'ipa_stack_mean_dev': [_vp, _vp, _i, _i, _i, _i, _l, _l, _vp, _l],
    'ipa_luma_dev': [_vp, _vp, _i, _i, _l, _dp, _d, _vp, _l],
    'ipa_strided_extremum_dev': [_vp, _vp, _i, _i, _i, _l, _i, _i, _i, _dp],
    'ipa_flat_scale_dev': [_vp, _vp, _i, _i, _l, _vp, _l, _d, _i, _d, _i, _vp, _l],
    'ipa_nlf_lower_mask_dev': [_vp, _vp, _i, _i, _i, _l, _vp, _l, _i, _dp, _d, _vp, _l],
    'ipa_sens_shrink_dev': [_vp, _vp, _i, _i, _i, _l, _vp, _l, _d, _i, _i, _vp, _l],
    'ipa_sens_accumulate_dev': [_vp, _vp, _i, _i, _i, _l, _vp, _l, _d, _vp, _i, _i, _l, _vp, _l, _i, _i],
    'ipa_tss_event_length_dev': [_vp, _vp, _i, _i, _i, _i, _l, _l, _dp, _vp, _vp, _vp, _l, _vp, _l, _vp, _l,
                                 _vp, _l, _l],
    'ipa_tss_finish_dev': [_vp, _vp, _vp, _i, _i, _l, _l, _vp, _l],
    'ipa_ovs_object_dev': [_vp, _vp, _i, _i, _l, _vp, _i, _i, _i, _i, _l, _l, _dp, _vp, _l, _vp, _l],
    'ipa_ovs_flatfield_dev': [_vp, _vp, _l, _vp, _i, _i, _i, _i, _l, _l, _vp, _l, _l, _dp, _vp, _i, _i, _l,
                              _vp, _l, _i, _vp, _i, _l],
    'ipa_masked_running_mean_dev': [_vp, _vp, _l, _vp, _l, _vp, _i, _l, _vp, _l, _i, _i],
    'ipa_poly2d_moments_dev': [_vp, _vp, _i, _i, _i, _l, _vp, _l, _i, _dp],
    'ipa_poly2d_eval_dev': [_vp, _dp, _i, _i, _vp, _i, _i, _i, _l, _vp, _l, _vp, _vp, _i, _i, _l, _vp, _l, _dp],
    'ipa_high_grad_dev': [_vp, _vp, _i, _i, _i, _l, _d, _i, _vp, _l, _dp],
    'ipa_clip01_dev': [_vp, _vp, _i, _i, _i, _l],
    'ipa_spot_range_dev': [_vp, _vp, _i, _i, _i, _l, _vp, _l, _d, _dp],
    'ipa_spot_histogram_dev': [_vp, _vp, _i, _i, _i, _l, _vp, _l, _d, _dp, _i, _vp],
    'ipa_spot_mask_dev': [_vp, _vp, _i, _i, _i, _l, _vp, _l, _d, _d, _vp, _l],
    'ipa_label_dev': [_vp, _vp, _i, _i, _l, _i, _vp, _l, _ip],
    'ipa_label_sizes_dev': [_vp, _vp, _i, _i, _l, _i, _vp],
    'ipa_label_largest_dev': [_vp, _vp, _i, _i, _l, _i, _vp],
    'ipa_spot_take_dev': [_vp, _vp, _i, _i, _i, _l, _vp, _l, _d, _vp, _l, _i, _i, _i, _vp, _l, _vp, _l, _dp],
    'ipa_cell_means_dev': [_vp, _vp, _i, _i, _i, _i, _l, _l, _vp, _i, _l, _d, _ip, _i, _ip, _i, _vp],
    'ipa_steps_separate_dev': [_vp, _vp, _i, _i, _i, _i, _i, _ip, _d, _i, _i, _d, _vp, _vp, _vp, _ip, _dp],
    'ipa_offset_meshgrid_dev': [_vp, _d, _d, _d, _d, _d, _d, _i, _i, _i, _vp, _vp, _l],
    'ipa_isnan_mask_dev': [_vp, _vp, _i, _i, _i, _l, _vp, _l],
    'ipa_fn2d_normal_dev': [_vp, _vp, _i, _i, _i, _l, _vp, _l, _i, _dp, _dp],
    'ipa_fn2d_eval_dev': [_vp, _i, _dp, _i, _vp, _i, _i, _i, _l, _vp, _l, _vp, _vp, _i, _i, _l, _vp, _l, _dp],
    'ipa_fn2d_divide_dev': [_vp, _vp, _i, _i, _i, _l, _d],
}
_CHARP = {'ipa_status_string': [_i], 'ipa_last_error': [_vp]}

_lib = None


class ImgProcHipError(RuntimeError):
    """a call into libimgproc_hip.so returned a non-zero status"""

    def __init__(self, status, message):
        RuntimeError.__init__(self, message)
        self.status = status


def lib():
    """load (once) and return the ctypes handle; raises if the extension is absent"""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                'imgprocessor_amd: %s is missing. Build it with '
                '`make -C imgprocessor_amd/csrc -j8` (or __graft_entry__.build()). '
                'There is no CPU fallback.' % LIB_PATH)
        l = C.CDLL(LIB_PATH)
        for name, args in PROTOTYPES.items():
            f = getattr(l, name)
            f.argtypes = args
            f.restype = _i
        for name, args in _CHARP.items():
            f = getattr(l, name)
            f.argtypes = args
            f.restype = C.c_char_p
        _lib = l
    return _lib


def check(status, ctx_handle=None, what=''):
    if status == OK:
        return
    l = lib()
    msg = l.ipa_last_error(ctx_handle) if ctx_handle else l.ipa_last_error(None)
    text = '%s: %s (%s)' % (what or 'libimgproc_hip', (msg or b'').decode() or '?',
                            l.ipa_status_string(status).decode())
    if status == ERR_BAD_ARG:
        raise ValueError(text)
    if status == ERR_UNSUPPORTED:
        raise NotImplementedError(text)
    if status == ERR_OOM:
        raise MemoryError(text)
    raise ImgProcHipError(status, text)


def dbl(values, n=None):
    """host double array for the small matrix / kernel arguments"""
    vals = [float(v) for v in values]
    if n is not None and len(vals) != n:
        raise ValueError('expected %d values, got %d' % (n, len(vals)))
    return (C.c_double * len(vals))(*vals)
