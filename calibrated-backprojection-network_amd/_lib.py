"""ctypes binding of libkbnet_hip.so (the C ABI declared in include/kbnet_hip.h).

`import torch` happens before `ctypes.CDLL` on purpose: torch bundles its own
libamdhip64 with the same SONAME as /opt/rocm's, and the extension must bind to the
HIP runtime that is already loaded so streams and device pointers are shared.
There is NO fallback: a missing library is an error, never a silent CPU path.
"""

from __future__ import annotations

import ctypes as C
import os

import torch  # noqa: F401  (must precede CDLL, see module docstring)

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("KBN_LIB_PATH") or os.path.join(HERE, "libkbnet_hip.so")   # KBN_LIB_PATH: an alternative build (same-box A/B of compile-time variants, tools/ab_lib.sh)

KBN_OK = 0
KBN_ERR_INVALID_ARGUMENT, KBN_ERR_UNSUPPORTED, KBN_ERR_WORKSPACE, KBN_ERR_LAUNCH = -1, -2, -3, -4
KBN_SRC_TENSOR, KBN_SRC_COORDS, KBN_SRC_XYZ, KBN_SRC_PAIR = 0, 1, 2, 3
KBN_ACT_ELU, KBN_ACT_SIGMOID = 1, 2
KBN_RESIZE_NONE, KBN_RESIZE_NEAREST = 0, 1
KBN_MAX_SRC = 3
KBN_ADAM_TABLE_CAPACITY, KBN_ADAM_PASS_ELEMENTS = 48, 524288   # tensors a kbn_adam_step launch carries; elements one pass of its widest grid covers
KBN_MULTI_COPY_TABLE_CAPACITY, KBN_MULTI_COPY_PASS_ELEMENTS = 48, 524288   # the same two numbers of a kbn_multi_tensor_scale_copy launch
KBN_AUGMENT_ROLE_IMAGE, KBN_AUGMENT_ROLE_RANGE, KBN_AUGMENT_ROLE_VALIDITY = 0, 1, 2
KBN_AUGMENT_RANGE_0_255, KBN_AUGMENT_RANGE_0_1, KBN_AUGMENT_RANGE_M1_1 = 0, 1, 2
KBN_AUGMENT_NOISE_NONE, KBN_AUGMENT_NOISE_GAUSSIAN, KBN_AUGMENT_NOISE_UNIFORM = 0, 1, 2
KBN_AUGMENT_STAGE_SELECT, KBN_AUGMENT_STAGE_APPLY = 1, 2
KBN_AUGMENT_MAX_FRAMES, KBN_AUGMENT_WORKSPACE_RECORD_BYTES = 512, 16   # frames whose flags one launch carries; workspace bytes a frame and range map
KBN_UNPACK_TRAIN_MAX_FRAMES = 64   # frame records a kbn_unpack_train_frames_forward launch carries
KBN_UNPACK_PACKED_MAX_RAW_WIDTH = 16384   # widest packed triplet kbn_unpack_packed_frames_forward takes (its LDS budget)
KBN_UNPACK_SEQUENCE_MAX_FRAMES = 48   # sample records a launch of the two sequence entry points carries
KBN_PACK_FRAMES_MAX_WIDTH = 16384   # widest plane row kbn_pack_frames_forward takes (its LDS budget)
KBN_MAX_CHANNELS, KBN_MAX_WEIGHT_ELEMENTS = 1 << 20, 1 << 28   # the conv layers' common range: past it every size function answers 0
KBN_MAX_MAP_SIDE, KBN_MAX_SIZE_BYTES = 1 << 24, 1 << 62
KBN_SUMMARY_CELL_ZERO, KBN_SUMMARY_CELL_COPY, KBN_SUMMARY_CELL_PHOTO_ERR, KBN_SUMMARY_CELL_DEPTH, KBN_SUMMARY_CELL_REL_ERR = 0, 1, 2, 3, 4
KBN_SUMMARY_COLORMAP_VIRIDIS, KBN_SUMMARY_COLORMAP_INFERNO = 0, 1
KBN_SUMMARY_MAX_ROWS = 4   # rows of a kbn_summary_panel_forward panel
KBN_HISTOGRAM_POSITIVE_EDGES, KBN_HISTOGRAM_BINS, KBN_HISTOGRAM_WORKSPACE_BYTES = 774, 1548, 32768   # kbn_histogram_forward's table, counts, workspace
ABI_VERSION = 11


class KbnError(RuntimeError):
    pass


class ConvSrc(C.Structure):
    """Mirror of `kbn_conv_src` (include/kbnet_hip.h)."""
    _fields_ = [
        ("kind", C.c_int),
        ("channels", C.c_int),
        ("data", C.c_void_p),
        ("batch_stride", C.c_longlong),
        ("src_height", C.c_int),
        ("src_width", C.c_int),
        ("aux_channels", C.c_int),
        ("proj_weight", C.c_void_p),
        ("coordinates", C.c_void_p),
        ("coordinates_batch_stride", C.c_longlong),
        ("kinv", C.c_void_p),
        ("absmax", C.c_void_p),
        ("scale", C.c_void_p),
    ]


class AdamTensor(C.Structure):
    """Mirror of `kbn_adam_tensor` (include/kbnet_hip.h): one tensor of a kbn_adam_step call."""
    _fields_ = [
        ("param", C.c_void_p),
        ("grad", C.c_void_p),
        ("exp_avg", C.c_void_p),
        ("exp_avg_sq", C.c_void_p),
        ("numel", C.c_longlong),
        ("weight_decay", C.c_float),
        ("one_minus_beta1", C.c_float),
        ("beta2", C.c_float),
        ("one_minus_beta2", C.c_float),
        ("step_size", C.c_float),
        ("bc2_sqrt", C.c_float),
        ("eps", C.c_float),
    ]


class CopyTensor(C.Structure):
    """Mirror of `kbn_copy_tensor` (include/kbnet_hip.h): one tensor of a kbn_multi_tensor_scale_copy call."""
    _fields_ = [
        ("src", C.c_void_p),
        ("dst", C.c_void_p),
        ("numel", C.c_longlong),
    ]


class AugmentTensor(C.Structure):
    """Mirror of `kbn_augment_tensor` (include/kbnet_hip.h): one tensor of a kbn_augment_forward call."""
    _fields_ = [
        ("src", C.c_void_p),
        ("dst", C.c_void_p),
        ("stride_n", C.c_longlong),
        ("stride_c", C.c_longlong),
        ("stride_h", C.c_longlong),
        ("stride_w", C.c_longlong),
        ("channels", C.c_int),
        ("role", C.c_int),
        ("map_index", C.c_int),
        ("reserved", C.c_int),
    ]


class TrainFrame(C.Structure):
    """Mirror of `kbn_train_frame` (include/kbnet_hip.h): one frame of a kbn_unpack_train_frames_forward call."""
    _fields_ = [
        ("image_offset", C.c_longlong),
        ("depth_offset", C.c_longlong),
        ("height", C.c_int),
        ("raw_width", C.c_int),
        ("y_start", C.c_int),
        ("x_start", C.c_int),
    ]


class PackedFrame(C.Structure):
    """Mirror of `kbn_packed_frame` (include/kbnet_hip.h): one frame of a kbn_unpack_packed_frames_forward call."""
    _fields_ = [
        ("image_offset", C.c_longlong),
        ("depth_offset", C.c_longlong),
        ("image_bytes", C.c_uint),
        ("depth_bytes", C.c_uint),
        ("height", C.c_int),
        ("raw_width", C.c_int),
        ("y_start", C.c_int),
        ("x_start", C.c_int),
    ]


class SequenceFrame(C.Structure):
    """Mirror of `kbn_sequence_frame` (include/kbnet_hip.h): one sample of a kbn_unpack_sequence_frames_forward call."""
    _fields_ = [
        ("image_offset", C.c_longlong * 3),
        ("depth_offset", C.c_longlong),
        ("height", C.c_int),
        ("width", C.c_int),
        ("y_start", C.c_int),
        ("x_start", C.c_int),
    ]


class PackedSequenceFrame(C.Structure):
    """Mirror of `kbn_packed_sequence_frame` (include/kbnet_hip.h): one sample of a kbn_unpack_packed_sequence_frames_forward call."""
    _fields_ = [
        ("image_offset", C.c_longlong * 3),
        ("depth_offset", C.c_longlong),
        ("image_bytes", C.c_uint * 3),
        ("depth_bytes", C.c_uint),
        ("height", C.c_int),
        ("width", C.c_int),
        ("y_start", C.c_int),
        ("x_start", C.c_int),
    ]


class SummarySource(C.Structure):
    """Mirror of `kbn_summary_source` (include/kbnet_hip.h): one tensor a cell of a kbn_summary_panel_forward call reads."""
    _fields_ = [
        ("data", C.c_void_p),
        ("stride_n", C.c_longlong),
        ("stride_c", C.c_longlong),
        ("stride_h", C.c_longlong),
        ("stride_w", C.c_longlong),
        ("channels", C.c_int),
        ("reserved", C.c_int),
    ]


class SummaryCell(C.Structure):
    """Mirror of `kbn_summary_cell`: a kind (KBN_SUMMARY_CELL_*) and up to three sources."""
    _fields_ = [
        ("kind", C.c_int),
        ("reserved", C.c_int),
        ("src", SummarySource * 3),
    ]


class SummaryRow(C.Structure):
    """Mirror of `kbn_summary_row`: the left and the right cell of one row of a panel."""
    _fields_ = [
        ("left", SummaryCell),
        ("right", SummaryCell),
    ]


_P, _I, _L, _F = C.c_void_p, C.c_int, C.c_longlong, C.c_float

# name -> (restype, argtypes); must list every symbol include/kbnet_hip.h declares
SIGNATURES = {
    "kbn_version": (_I, []),
    "kbn_status_string": (C.c_char_p, [_I]),
    "kbn_reload_env": (None, []),
    "kbn_knob": (_I, [C.c_char_p]),
    "kbn_set_autotune": (_I, [_I]),
    "kbn_get_autotune": (_I, []),
    "kbn_s2d_forward": (_I, [_P, C.POINTER(_P), _P, _P, _I, _I, _I, _I, C.POINTER(_I), _I,
                             C.POINTER(_I), _I, _I, _I, _F, _P]),
    "kbn_s2d_pyramid": (_I, [_P, _L, _P, _I, _I, _I, C.POINTER(_I), _I, C.POINTER(_I), _I, _P]),
    "kbn_intrinsics_inverse": (_I, [_P, _P, _I, _F, _F, _P]),
    "kbn_camera_coordinates": (_I, [_P, _P, _I, _I, _I, _P]),
    "kbn_conv2d_packed_weight_bytes": (C.c_size_t, [_I, _I, _I, _I]),
    "kbn_conv2d_pack_weight": (_I, [_P, _P, _I, _I, _I, _I, _P]),
    "kbn_conv2d_forward": (_I, [C.POINTER(ConvSrc), _I, _P, _P, _L, _I, _I, _I, _I, _I, _I, _I, _I,
                                _F, _P, _P]),
    "kbn_upconv2x_packed_weight_bytes": (C.c_size_t, [_I, _I]),
    "kbn_upconv2x_pack_weight": (_I, [_P, _P, _I, _I, _P]),
    "kbn_upconv2x_forward": (_I, [_P, _L, _P, _P, _L, _I, _I, _I, _I, _I, _I, _F, _P, _P]),
    "kbn_activation_forward": (_I, [_P, _L, _I, _L, _I, _P, _P]),
    "kbn_scale_planes_forward": (_I, [_P, _L, _P, _L, _P, _L, _I, _I, _I, _I, _P]),
    "kbn_deconv2x_pack_weight": (_I, [_P, _P, _I, _I, _P]),
    "kbn_deconv2x_forward": (_I, [_P, _L, _P, _P, _L, _I, _I, _I, _I, _I, _I, _F, _P, _P]),
    "kbn_upconv2x_query": (_I, [_I, _I, _I, _I, _I, C.POINTER(_I)]),
    "kbn_conv2d_query": (_I, [_I, _I, _I, _I, _I, _I, _I, _I, C.POINTER(_I)]),
    "kbn_conv_last_route": (_I, [C.POINTER(_I)]),
    "kbn_kb_block_forward": (_I, [_P, _L, _P, _L, _P, _P, _P, _L, _P, _P, _P, _P, _P, _L, _P, _L, _P,
                                  _L, _I, _I, _I, _I, _I, _I, _I, _I, _I, _F, _P, _P, _P, _P]),
    "kbn_kb1_front_packed_weight_bytes": (C.c_size_t, [_I, _I, _I]),
    "kbn_kb1_front_pack_weight": (_I, [_P, _P, _P, _P, _I, _I, _I, _P]),
    "kbn_kb1_front_query": (_I, [_I, _I, _I, _I, _I, _F]),
    "kbn_kb1_depth_front_query": (_I, [_I, _I, _I, _I, _I, _F]),
    "kbn_kb1_front_forward": (_I, [_P, _L, _P, _P, _L, _P, _L, _P, _L, _I, _I, _I, _I, _I, _I, _F, _F, _P, _P, _P]),
    "kbn_kb1_front_next_packed_weight_bytes": (C.c_size_t, [_I, _I, _I]),
    "kbn_kb1_front_next_pack_weight": (_I, [_P, _P, _I, _I, _I, _P]),
    "kbn_kb1_front_next_query": (_I, [_I, _I, _I, _I, _I, _I, _F]),
    "kbn_kb1_front_next_forward": (_I, [_P, _L, _P, _P, _L, _P, _L, _P, _L, _I, _I, _I, _I, _I, _I, _F, _F, _P, _P,
                                        _P, _P, _L, _P, _L, _I, _F, _P, _P]),
    "kbn_kb1_depth_front_packed_weight_bytes": (C.c_size_t, [_I, _I, _I]),
    "kbn_kb1_depth_front_pack_weight": (_I, [_P, _P, _P, _P, _I, _I, _I, _P]),
    "kbn_kb1_depth_front_forward": (_I, [_P, _L, _P, _P, _P, _L, _P, _L, _I, _I, _I, _I, _I, _I, _F, _F, _I, _F, _P, _P]),
    "kbn_s2d_depth_front_packed_weight_bytes": (C.c_size_t, [_I]),
    "kbn_s2d_depth_front_pack_weight": (_I, [_P, _P, _P, _P, _P, _I, _P]),
    "kbn_s2d_depth_front_query": (_I, [_I, C.POINTER(_I), _I, C.POINTER(_I), _I, _I, _I, _I, _I, _I, _I, _F, _F]),
    "kbn_s2d_depth_front_forward": (_I, [_P, _L, _P, _P, _P, _P, _L, _P, _L, _I, _I, C.POINTER(_I), _I, C.POINTER(_I), _I, _I, _I, _I, _I,
                                        _I, _I, _F, _F, _F, _I, _F, _P, _P]),
    "kbn_preprocess_forward": (_I, [_P, _P, _P, _P, _P, _P, C.c_size_t, _I, _I, _I, _I, _I, _F, _I, _P]),
    "kbn_eval_accumulate": (_I, [_P, _P, _P, _P, _I, _I, _I, _F, _F, _P]),
    "kbn_photometric_loss_forward": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _P]),
    "kbn_photometric_loss_backward": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _P]),
    "kbn_conv2d_s2_affine_packed_weight_bytes": (C.c_size_t, [_I, _I, _I]),
    "kbn_conv2d_s2_affine_pack_weight": (_I, [_P, _P, _I, _I, _I, _P]),
    "kbn_conv2d_s2_affine_forward": (_I, [C.POINTER(ConvSrc), _I, _P, _P, _P, _P, _L, _I, _I, _I, _I, _I, _I, _F, _P]),
    "kbn_pose_head_forward": (_I, [_P, _L, _P, _P, _P, _I, _I, _I, _I, _P]),
    "kbn_conv2d_s2_backward_data_packed_weight_bytes": (C.c_size_t, [_I, _I, _I]),
    "kbn_conv2d_s2_backward_data_pack_weight": (_I, [_P, _P, _I, _I, _I, _P]),
    "kbn_conv2d_s2_backward_data": (_I, [_P, _L, _P, _P, _L, _I, _P, _L, _I, _I, _I, _I, _I, _I, _P]),
    "kbn_conv2d_s2_backward_weight_scratch_bytes": (C.c_size_t, [_I, _I, _I, _I, _I, _I, _I]),
    "kbn_conv2d_s2_backward_weight": (_I, [C.POINTER(ConvSrc), _I, _P, _L, _P, _I, _I, _I, _I, _I, _I, _P, C.c_size_t, _P]),
    "kbn_bn_stats_forward": (_I, [_P, _L, _P, _P, _I, _I, _I, _I, _P]),
    "kbn_bn_act_forward": (_I, [_P, _L, _P, _P, _P, _L, _I, _I, _I, _I, _I, _F, _P]),
    "kbn_bn_act_backward": (_I, [_P, _L, _P, _L, _P, _P, _P, _P, _P, _P, _L, _I, _I, _I, _I, _I, _F, _I, _P]),
    "kbn_bn_moments_forward": (_I, [_P, _L, _P, _I, _I, _I, _I, _P]),
    "kbn_bn_moments_merge": (_I, [_P, _I, _I, _P, _P, _P, _P]),
    "kbn_bn_act_backward_sums": (_I, [_P, _L, _P, _L, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _F, _P]),
    "kbn_bn_act_backward_sync_apply": (_I, [_P, _L, _P, _L, _P, _P, _P, _P, _P, _P, _I, _I, _P, _L, _I, _I, _I, _I, _I, _F, _P]),
    "kbn_conv2d_affine_packed_weight_bytes": (C.c_size_t, [_I, _I, _I]),
    "kbn_conv2d_affine_pack_weight": (_I, [_P, _P, _I, _I, _I, _P]),
    "kbn_conv2d_affine_forward": (_I, [C.POINTER(ConvSrc), _I, _P, _P, _P, _P, _L, _P, _L, _I, _I, _I, _I, _I, _I, _I, _F, _P]),
    "kbn_maxpool3x3s2_forward": (_I, [_P, _L, _P, _L, _I, _I, _I, _I, _P]),
    "kbn_conv2d_backward_weight_scratch_bytes": (C.c_size_t, [_I, _I, _I, _I, _I, _I, _I, _I]),
    "kbn_conv2d_backward_weight": (_I, [C.POINTER(ConvSrc), _I, _P, _L, _P, _I, _I, _I, _I, _I, _I, _I, _P, C.c_size_t, _P]),
    "kbn_conv2d_backward_data_packed_weight_bytes": (C.c_size_t, [_I, _I, _I, _I]),
    "kbn_conv2d_backward_data_pack_weight": (_I, [_P, _P, _I, _I, _I, _I, _P]),
    "kbn_conv2d_backward_data": (_I, [_P, _L, _P, _P, _L, _I, _I, _I, _I, _I, _I, _I, _P]),
    "kbn_maxpool3x3s2_backward": (_I, [_P, _L, _P, _L, _P, _L, _I, _I, _I, _I, _P]),
    "kbn_add_act_forward": (_I, [_P, _P, _P, _L, _I, _F, _P]),
    "kbn_add_act_backward": (_I, [_P, _P, _P, _L, _I, _F, _P]),
    "kbn_resize_nearest_forward": (_I, [_P, _L, _P, _L, _I, _I, _I, _I, _I, _I, _P]),
    "kbn_resize_nearest_backward": (_I, [_P, _L, _P, _L, _I, _I, _I, _I, _I, _I, _P]),
    "kbn_kb_xyz_backward": (_I, [_P, _L, _P, _L, _P, _L, _P, _L, _I, _I, _I, _I, _F, _P]),
    "kbn_depth_map_backward": (_I, [_P, _P, _P, _P, _L, _F, _P]),
    "kbn_depth_head_forward": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _F, _F, _P]),
    "kbn_conv_head_forward": (_I, [_P, _L, _P, _P, _P, _P, _I, _I, _I, _I, _I, _F, _F, _F, _P]),
    "kbn_conv_tail_packed_weight_bytes": (C.c_size_t, [_I]),
    "kbn_conv_tail_pack_weight": (_I, [_P, _P, _I, _P]),
    "kbn_conv_tail_forward": (_I, [_P, _L, _P, _P, _P, _P, _I, _I, _I, _I, _I, _F, _F, _F, _P]),
    "kbn_conv_tail_forward_pair": (_I, [_P, _L, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _F, _F, _F, _P]),
    "kbn_absmax_frames": (_I, [_P, _L, _I, _L, _P, _P]),
    "kbn_conv3x3_split_packed_weight_bytes": (C.c_size_t, [_I, _I, _I]),
    "kbn_conv3x3_split_pack_weight": (_I, [_P, _P, _I, _I, _I, _P]),
    "kbn_conv3x3_split_forward": (_I, [C.POINTER(ConvSrc), _I, _P, _P, _L, _I, _I, _I, _I, _I, _I, _I, _F, _P, _P, _L, _P, _P]),
    "kbn_conv3x3_split_forward_ksplit": (_I, [C.POINTER(ConvSrc), _I, _P, _P, _L, _I, _I, _I, _I, _I, _I, _I, _F, _P, _I, _P, _P]),
    "kbn_conv1x1s2_split_packed_weight_bytes": (C.c_size_t, [_I, _I, _I]),
    "kbn_conv1x1s2_split_pack_weight": (_I, [_P, _P, _I, _I, _I, _P]),
    "kbn_conv1x1s2_split_forward": (_I, [C.POINTER(ConvSrc), _I, _P, _P, _L, _P, _L, _I, _I, _I, _I, _I, _I, _F, _P, _P]),
    "kbn_kb_xyz_s2_forward": (_I, [_P, _L, _I, _I, _I, _P, _P, _I, _F, _P, _L, _I, _P]),
    "kbn_adam_step": (_I, [C.POINTER(AdamTensor), _I, _P]),
    "kbn_multi_tensor_scale_copy": (_I, [C.POINTER(CopyTensor), _I, _F, _P]),
    "kbn_augment_workspace_bytes": (C.c_size_t, [C.POINTER(AugmentTensor), _I, _I, _I, _I]),
    "kbn_augment_forward": (_I, [C.POINTER(AugmentTensor), _I, C.c_char_p, _I, _I, _I, _P, _P, C.c_size_t, _I, _I, _F, C.c_ulonglong, C.c_uint, _I, _P]),
    "kbn_augment_forward_at": (_I, [C.POINTER(AugmentTensor), _I, C.c_char_p, _I, _I, _I, _P, _P, C.c_size_t, _I, _I, _F, C.c_ulonglong, C.c_uint, C.c_uint, _I, _P]),
    "kbn_summary_panel_forward": (_I, [C.POINTER(SummaryRow), _I, _I, _I, _I, _F, _P, _P]),
    "kbn_summary_colorize_forward": (_I, [_P, _L, _L, _L, _I, _I, _I, _I, _P, _P]),
    "kbn_png_info": (_I, [_P, C.c_size_t, _P, _P, _P, _P]),
    "kbn_png_decode": (_I, [_P, C.c_size_t, _P, C.c_size_t]),
    "kbn_png_decode_batch": (_I, [_P, _P, _P, _P, _I, _I, _P]),
    "kbn_depth_to_u16_forward": (_I, [_P, _P, _L, _P]),
    "kbn_png_encode_gray16_bound": (C.c_size_t, [_I, _I]),
    "kbn_png_encode_gray16": (_I, [_P, _I, _I, _P, C.c_size_t, _P, _I]),
    "kbn_export_pack_forward": (_I, [_P, _F, _F, _P, _P, _P, _P, _P, _I, _I, _I, _P]),
    "kbn_png_encode_rgb8_bound": (C.c_size_t, [_I, _I]),
    "kbn_png_encode_rgb8": (_I, [_P, _I, _I, _P, C.c_size_t, _P, _I]),
    "kbn_png_encode_gray8_bound": (C.c_size_t, [_I, _I]),
    "kbn_png_encode_gray8": (_I, [_P, _I, _I, _P, C.c_size_t, _P, _I]),
    "kbn_unpack_frames_forward":(_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P]),
    "kbn_unpack_train_frames_forward": (_I, [_P, C.c_size_t, _P, C.c_size_t, C.POINTER(TrainFrame), _I, _I, _I, _I, _I, _P, _P, _P, _P, _P]),
    "kbn_frame_info": (_I, [_P, C.c_size_t, _P, _P, _P, _P]),
    "kbn_frame_encode_bound": (C.c_size_t, [_I, _I, _I, _I]),
    "kbn_frame_encode": (_I, [_P, _I, _I, _I, _I, _P, C.c_size_t, _P]),
    "kbn_frame_decode": (_I, [_P, C.c_size_t, _P, C.c_size_t]),
    "kbn_frame_check": (_I, [_P, C.c_size_t]),
    "kbn_unpack_packed_frames_forward": (_I, [_P, C.c_size_t, _P, C.c_size_t, C.POINTER(PackedFrame), _I, _I, _I, _I, _I, _P, _P, _P, _P, _P]),
    "kbn_unpack_sequence_frames_forward": (_I, [_P, C.c_size_t, _P, C.c_size_t, C.POINTER(SequenceFrame), _I, _I, _I, _I, _I, _P, _P, _P, _P, _P]),
    "kbn_unpack_packed_sequence_frames_forward": (_I, [_P, C.c_size_t, _P, C.c_size_t, C.POINTER(PackedSequenceFrame), _I, _I, _I, _I, _I, _P, _P, _P, _P, _P]),
    "kbn_pack_frames_stride": (C.c_size_t, [_I, _I, _I, _I]),
    "kbn_pack_frames_workspace_bytes": (C.c_size_t, [_I, _I, _I, _I, _I]),
    "kbn_pack_frames_forward": (_I, [_P, _I, _I, _I, _I, _I, _P, C.c_size_t, _P, _P, C.c_size_t, _P]),
    "kbn_point_cloud_workspace_bytes": (C.c_size_t, [_I, _I, _I]),
    "kbn_point_cloud_forward": (_I, [_P, _L, _P, _F, _F, _P, _F, _F, _I, _I, _I, _P, C.c_size_t, _P, _P, C.c_size_t, _P]),
    "kbn_histogram_forward": (_I, [_P, _L, _P, _P, _P, _P, C.c_size_t, _P]),
    "kbn_crc32c": (C.c_uint, [C.c_char_p, C.c_size_t, C.c_uint]),
}

_lib = None


def load():
    """Loads the shared library once; raises KbnError when it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise KbnError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'`"
            " (needs hipcc).  There is no CPU fallback for the product path.")
    lib = C.CDLL(LIB_PATH)
    rebuild = "rebuild it with `python -c 'import __graft_entry__ as g; g.build()'`"
    try:
        lib.kbn_version.restype = _I
        lib.kbn_version.argtypes = []
        have = lib.kbn_version()
    except AttributeError:
        raise KbnError(f"{LIB_PATH} exports no kbn_version: not a KBNet HIP library; {rebuild}") from None
    if have != ABI_VERSION:   # checked BEFORE the symbols are bound: a stale library names the mismatch, not a missing symbol
        raise KbnError(f"libkbnet_hip.so ABI {have} != binding ABI {ABI_VERSION}: stale library; {rebuild}")
    for name, (res, args) in SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError:
            raise KbnError(f"libkbnet_hip.so (ABI {have}) does not export {name}: header / library mismatch; {rebuild}") from None
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(status: int, what: str):
    if status != KBN_OK:
        msg = load().kbn_status_string(status).decode()
        raise KbnError(f"{what} failed: {msg} (status {status})")
