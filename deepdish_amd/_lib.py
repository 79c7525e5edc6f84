"""ctypes binding of libdeepdish_hip.so (the C ABI declared in include/deepdish_hip.h).

There is deliberately no fallback: if the library is missing or a call fails, this raises.
"""
import ctypes
import os
from ctypes import c_int, c_int64, c_double, c_float, c_void_p, c_char_p, POINTER

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('DD_LIB') or os.path.join(HERE, 'libdeepdish_hip.so')      # DD_LIB: another build of the same ABI (same-box A/B runs)

P = c_void_p


class DeepDishHipError(RuntimeError):
    pass


# name -> argtypes (every function returns int unless listed in _RESTYPE)
SIGNATURES = {
    'dd_last_error': [],
    'dd_version': [],
    'dd_ctx_create': [c_int, POINTER(P)],
    'dd_ctx_destroy': [P],
    'dd_ctx_stream': [P, POINTER(P)],
    'dd_ctx_sync': [P],
    'dd_kf_initiate': [P, P, P, P, P, c_int, P],
    'dd_kf_predict': [P, P, P, P, c_int, P],
    'dd_kf_project': [P, P, P, P, c_int, P, P, P],
    'dd_kf_update': [P, P, P, P, P, c_int, P],
    'dd_kf_gate': [P, P, P, P, c_int, P, c_int, c_int, P, P],
    'dd_iou_cost': [P, P, P, c_int, P, c_int, P, P],
    'dd_cosine_nn_cost': [P, P, P, c_int, P, c_int, P, P],
    'dd_euclidean_nn_cost': [P, P, P, c_int, P, c_int, P, P],
    'dd_nms': [P, P, P, c_int, c_double, P, P, P],
    'dd_nms_ssd': [P, P, P, c_int, c_double, P, P, P],
    'dd_lsap_host': [P, c_int, c_int, P, P],
    'dd_pyset_difference_order_host': [P, c_int, P, c_int, P, POINTER(c_int)],
    'dd_lsap_batch': [P, P, P, P, P, c_int, P, P],
    'dd_match_cascade': [P, c_int, P, P, c_int, c_int, P, P, c_double, c_double, c_int, P, POINTER(c_int), P, POINTER(c_int), P,
                         POINTER(c_int)],
    'dd_tracker_create': [P, c_double, c_double, c_int, c_int, c_int, c_int, c_int, POINTER(P)],
    'dd_tracker_create_metric': [P, c_int, c_double, c_double, c_int, c_int, c_int, c_int, c_int, POINTER(P)],
    'dd_tracker_destroy': [P],
    'dd_tracker_predict': [P],
    'dd_tracker_update': [P, P, P, c_int, c_int],
    'dd_tracker_count': [P, c_int, POINTER(c_int)],
    'dd_tracker_read': [P, c_int, P, P, P],
    'dd_tracker_track_update': [P, c_int64, P, P, c_int],
    'dd_tracker_track_predict': [P, c_int64],
    'dd_tracker_track_set': [P, c_int64, c_int, c_int],
    'dd_tracker_remove': [P, P, c_int],
    'dd_tracker_next_id': [P, POINTER(c_int64)],
    'dd_tracker_last_cost': [P, P, P, c_int, POINTER(c_int), POINTER(c_int)],
    'dd_tracker_last_matches': [P, P, c_int, POINTER(c_int)],
    'dd_tracker_set_association': [P, c_int],
    'dd_tracker_association_stats': [P, POINTER(ctypes.c_longlong), POINTER(ctypes.c_longlong), POINTER(ctypes.c_longlong),
                                     POINTER(ctypes.c_longlong)],
    'dd_crop_resize': [P, P, c_int, c_int, P, c_int, c_int, c_int, P, P, P],
    'dd_crop_resize_f64': [P, P, c_int, c_int, P, c_int, c_int, c_int, P, P, P],
    'dd_fake_encode': [P, P, c_int, c_int, P, P],
    'dd_resize_lanczos': [P, P, c_int, c_int, c_int, c_int, P, c_int, c_int, P],
    'dd_resize_lanczos_batch': [P, P, c_int, c_int, c_int, c_int, c_int, P, c_int, c_int, P],
    'dd_resize_lanczos_plan': [P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, P, P, P, POINTER(c_int), POINTER(c_int), POINTER(c_int),
                               POINTER(c_int)],
    'dd_letterbox_geometry': [c_int, c_int, c_int, c_int, POINTER(c_int), POINTER(c_int), POINTER(c_int), POINTER(c_int)],
    'dd_resize_lanczos_letterbox': [P, P, c_int, c_int, c_int, c_int, c_int, P, c_int, c_int, c_int, P],
    'dd_resize_lanczos_letterbox_plan': [P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, POINTER(c_int), POINTER(c_int)],
    'dd_resize_bilinear': [P, P, c_int, c_int, c_int, P, c_int, c_int, P],
    'dd_yuv420_to_bgr': [P, P, c_int, c_int, c_int, c_int, c_int, c_int64, c_int64, P, P],
    'dd_yuv422_to_bgr': [P, P, c_int, c_int, c_int, c_int, c_int, c_int64, P, P],
    'dd_raw8_to_bgr': [P, P, c_int, c_int, c_int, c_int, c_int, c_int64, P, P],
    'dd_ingest_create_raw8': [P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, P],
    'dd_ingest_create': [P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, P],
    'dd_ingest_create_format': [P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, P],
    'dd_ingest_create_jpeg': [P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int64, P],
    'dd_ingest_create_jpeg_scaled': [P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int64, P],
    'dd_ingest_jpeg_put': [P, c_int, c_int, P, c_int64],
    'dd_ingest_create_jpeg_ex': [P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int64, P],
    'dd_ingest_status': [P, c_int, P],
    'dd_ingest_destroy': [P],
    'dd_ingest_host_slot': [P, c_int, P, P],
    'dd_ingest_submit': [P, c_int],
    'dd_ingest_wait_uploaded': [P, c_int],
    'dd_ingest_acquire': [P, c_int, P, P],
    'dd_ingest_release': [P, c_int, P],
    'dd_mog2_create': [P, c_int, c_int, c_int, c_int, c_double, c_int, POINTER(P)],
    'dd_mog2_destroy': [P],
    'dd_mog2_state': [P, c_int, P, P, P, P],
    'dd_mog2_apply': [P, P, c_double, P, P, P],
    'dd_mog2_apply_streams': [P, P, P, c_double, P, P, P],
    'dd_mask_box_count': [P, P, c_int, c_int, c_int, P, P, c_int, P, P],
    'dd_mask_stream_count': [P, P, c_int, c_int, c_int, P, c_int, P],
    'dd_pipeline_motion_gate': [P, P],
    'dd_pipeline_gate_stats': [P, P, P, P],
    'dd_net_create': [P, P, c_int, P, c_int64, c_int, POINTER(P)],
    'dd_net_create_shared': [P, P, c_int, P, c_int64, c_int, POINTER(P)],
    'dd_net_activation_bytes': [P, POINTER(c_int64)],
    'dd_net_destroy': [P],
    'dd_net_forward': [P, P, c_int, P],
    'dd_net_output': [P, c_int, POINTER(P), POINTER(c_int), POINTER(c_int), POINTER(c_int), POINTER(c_int),
                      POINTER(c_int)],
    'dd_net_use_graph': [P, c_int],
    'dd_net_input_size': [P, POINTER(c_int), POINTER(c_int)],
    'dd_net_max_batch': [P, POINTER(c_int)],
    'dd_net_last_batch': [P, POINTER(c_int)],
    'dd_net_read': [P, c_int, c_int, P, c_int, P],
    'dd_net_profile': [P, c_int],
    'dd_net_profile_read': [P, P, c_int, POINTER(c_int)],
    'dd_net_op_launches': [P, P, c_int, POINTER(c_int)],
    'dd_net_op_variants': [P, P, c_int, POINTER(c_int)],
    'dd_netq_dwpw_fits': [c_int, c_int, c_int, c_int, c_int, c_int, POINTER(c_int)],
    'dd_ssd_postprocess': [P, P, P, c_int, c_int, c_int, c_float, c_float, P, P, P, P, P],
    'dd_ssd_decode': [P, P, P, c_int, c_int, c_float, P, P, P, P, c_int, P],
    'dd_ssd_postprocess_decoded': [P, P, P, P, P, c_int, c_int, c_float, c_float, P, P, P, P, c_int, P],
    'dd_ssd_regular_nms_decoded': [P, P, P, c_int, c_int, c_int, c_int, c_int, c_int, c_float, c_float, P, P, P, P, c_int, P],
    'dd_ssd_postprocess_regular': [P, P, P, c_int, c_int, c_int, c_int, c_float, c_float, P, P, P, P, c_int, P],
    'dd_ssd_postprocess_regular_u8': [P, P, P, c_int, P, P, P, c_int, c_int, c_int, c_int, c_float, c_float, P, P, P, P, c_int, P],
    'dd_net_ssd_heads_u8': [P, POINTER(P), POINTER(P), POINTER(c_int), POINTER(P), P, POINTER(c_int), POINTER(c_int)],
    'dd_net_ssd_decode': [P, P, c_int, c_float, c_int],
    'dd_net_ssd_decoded': [P, POINTER(P), POINTER(P), POINTER(P), POINTER(P)],
    'dd_net_ssd_decoded_read': [P, c_int, P, P, P, P],
    'dd_net_yolo_decode': [P, c_int],
    'dd_net_yolo_decoded': [P, P, P, P, P],
    'dd_net_yolo_decoded_read': [P, c_int, P, P, P],
    'dd_ssd_detections': [P, P, P, P, c_int, c_int, c_double, c_double, c_double, c_double, P, P, P, P, P],
    'dd_yolov5_decode': [P, P, c_int, c_int, c_float, c_float, c_float, P, P, P, c_int, P, P],
    'dd_yolov5_decode_letterbox': [P, P, c_int, c_int, c_float, c_int, c_int, c_int, c_int, P, P, P, c_int, P, P],
    'dd_yolov5_decode_batch': [P, P, c_int, c_int, c_float, c_float, c_float, c_int, c_int, P, P, P, c_int, P, c_int, P],
    'dd_yolov5_select_batch': [P, P, P, P, c_int, c_float, c_float, c_float, c_int, c_int, P, P, P, c_int, P, c_int, P],
    'dd_yolov5_pack': [P, P, P, P, P, c_int, c_int, P, P],
    'dd_pipeline_create': [P, c_int, c_int, c_int, P, P, c_int, c_int, P, c_char_p, c_char_p, c_double, c_double,
                           c_double, c_int, c_int, P, c_int, c_int, POINTER(P)],
    'dd_pipeline_destroy': [P],
    'dd_pipeline_detector_adaptor': [P, c_int],
    'dd_pipeline_ssd_options': [P, c_int, c_float, c_float],
    'dd_pipeline_ssd_regular_nms': [P, c_int],
    'dd_pipeline_detector_skip_frames': [P, c_int],
    'dd_pipeline_detector_letterbox': [P, c_int],
    'dd_pipeline_metric': [P, c_int],
    'dd_pipeline_association': [P, c_int],
    'dd_pipeline_step': [P, P, P, P, P, P],
    'dd_pipeline_step2': [P, P, P, P, P, P, P],
    'dd_pipeline_step3': [P, P, P, P, P, P, P, P, P],
    'dd_pipeline_frames_seen': [P, P],
    'dd_pipeline_present_stats': [P, P],
    'dd_pipeline_detector_skip_streams': [P, P, P],
    'dd_pipeline_skip_stats': [P, P, P],
    'dd_pipeline_stream_lines': [P, P],
    'dd_pipeline_lines': [P, P, c_int, P],
    'dd_pipeline_stream_wanted': [P, P],
    'dd_pipeline_stream_tracker_params': [P, P, P, P, P],
    'dd_pipeline_stream_nms_overlap': [P, P],
    'dd_pipeline_stream_motion_ratio': [P, P],
    'dd_pipeline_reset_streams': [P, P, c_int],
    'dd_pipeline_stream_param_stats': [P, P],
    'dd_pipeline_snapshot_bytes': [P, P, c_int, c_int, POINTER(c_int64)],
    'dd_pipeline_snapshot': [P, P, c_int, c_int, P, c_int64, POINTER(c_int64)],
    'dd_pipeline_restore': [P, P, c_int64, P, c_int],
    'dd_snapshot_info': [P, c_int64, POINTER(c_int), P, c_int],
    'dd_tracker_gallery_read': [P, c_int64, P, c_int, POINTER(c_int), POINTER(c_int)],
    'dd_chunk_rows_gather': [P, P, c_int, c_int64, P, c_int, P, c_int, P, c_int64, P],
    'dd_chunk_rows_scatter': [P, P, c_int, c_int64, P, c_int, P, c_int, P, c_int64, P],
    'dd_pipeline_mog2': [P, POINTER(P)],
    'dd_mog2_reset_streams': [P, P, c_int, P],
    'dd_feature_rows_carry': [P, P, c_int64, P, c_int64, P, c_int64, P, c_int64, P, c_int, P],
    'dd_gather_frames': [P, P, c_int, c_int64, P, c_int, P, P],
    'dd_pipeline_background_subtraction': [P, c_double, c_int],
    'dd_pipeline_motion_mask': [P, P, c_int, POINTER(ctypes.c_longlong)],
    'dd_pipeline_counts': [P, P],
    'dd_pipeline_tracker': [P, c_int, POINTER(P)],
    'dd_pipeline_stage_seconds': [P, P, POINTER(ctypes.c_longlong)],
    'dd_pipeline_stage_gpu_ms': [P, P, POINTER(ctypes.c_longlong)],
    'dd_pipeline_detector_stream': [P, POINTER(P)],
    'dd_pipeline_detections': [P, c_int, P, P, P, c_int, POINTER(c_int)],
    'dd_pipeline_overlay': [P, P, c_int, P, P, P, P, P, P, P, P, P],
    'dd_render_create': [P, c_int, c_int, POINTER(P)],
    'dd_render_destroy': [P],
    'dd_render_record_set': [P, c_int],
    'dd_render_put_mask': [P, P, c_int, c_int, POINTER(c_int)],
    'dd_render_draw': [P, P, c_int, P, c_int, P, P, P, P],
    'dd_ground_camera': [c_double, c_double, c_double, c_int, c_int, c_double, c_double, c_double, P],
    'dd_ground_from_image': [P, P, c_int, P, P, ctypes.c_longlong, P, c_int, P],
    'dd_jpeg_create': [P, c_int, c_int, c_int, c_int, POINTER(P)],
    'dd_jpeg_destroy': [P],
    'dd_jpeg_header': [P, P, c_int, POINTER(c_int)],
    'dd_jpeg_plan': [c_int, c_int, c_int, POINTER(c_int)],
    'dd_jpeg_encode': [P, P, c_int, P, c_int64, P, P],
    'dd_jpeg_parse': [P, c_int64, P],
    'dd_jpegdec_plan': [c_int, c_int, c_int, c_int, c_int, POINTER(c_int), POINTER(c_int), POINTER(c_int)],
    'dd_jpegdec_create': [P, c_int, c_int, c_int, c_int64, POINTER(P)],
    'dd_jpegdec_destroy': [P],
    'dd_jpegdec_decode': [P, P, P, P, c_int, P, P, P],
    'dd_jpegdec_profile': [P, c_int],
    'dd_jpegdec_profile_read': [P, P],
    'dd_jpegdec_create_scaled': [P, c_int, c_int, c_int, c_int, c_int64, POINTER(P)],
    'dd_jpegdec_plan_scaled': [c_int, c_int, c_int, c_int, c_int, c_int, POINTER(c_int), POINTER(c_int), POINTER(c_int)],
    'dd_jpegdec_output_size': [P, POINTER(c_int), POINTER(c_int)],
    'dd_jpeg_draft_scale': [c_int, c_int, c_int, c_int],
    'dd_jpeg_parse_scans': [P, c_int64, P, P],
    'dd_jpegdec_create_ex': [P, c_int, c_int, c_int, c_int, c_int, c_int64, POINTER(P)],
    'dd_jpegdec_profile_levels': [P, P, POINTER(c_int)],
    'dd_jpegdec_split_stats': [P, P],
    'dd_jpegdec_decode_scales': [P, P, P, P, P, c_int, P, P, P],
    'dd_ingest_source_sizes': [P, c_int, P],
    'dd_jpeg_parse_flags': [P, c_int64, c_int, P, P],
    'dd_counts_accumulate': [P, P, P, c_int, P],
}
_RESTYPE = {'dd_last_error': c_char_p}

_lib = None
MISSING = []


def lib():
    """Load the shared library once; raise (never fall back) when it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise DeepDishHipError(
            'libdeepdish_hip.so is missing (%s): build it with `python -m deepdish_amd.build`; '
            'there is no CPU fallback' % LIB_PATH)
    # torch first: its wheel carries its own libamdhip64, and a process that loads /opt/rocm's copy through this library BEFORE torch
    # ends up with two HIP runtimes (seen: build() then smoke() in one process -> "no ROCm-capable device is detected")
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    l = ctypes.CDLL(LIB_PATH)
    for name, args in SIGNATURES.items():
        try:
            fn = getattr(l, name)
        except AttributeError:         # header and library out of sync; tests/test_abi.py fails on this
            MISSING.append(name)
            continue
        fn.argtypes = args
        fn.restype = _RESTYPE.get(name, c_int)
    _lib = l
    return l


def check(rc, what=''):
    if rc != 0:
        msg = lib().dd_last_error()
        raise DeepDishHipError('%s failed (%d): %s' % (what or 'libdeepdish_hip call', rc,
                                                      msg.decode() if msg else '?'))
