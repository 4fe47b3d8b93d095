"""ctypes binding of libaae_hip.so (include/aae_hip.h).

The product path has exactly one back end: the hand-written HIP library built
in-tree by ``__graft_entry__.build()``.  There is no CPU fallback -- if the
library or a GPU is missing, loading fails loudly.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, Structure, c_char_p, c_double, c_float, c_int, c_int32, c_int64, c_size_t, c_void_p

AAE_OK = 0
AAE_DTYPE_U8 = 0
AAE_DTYPE_F32 = 1
AAE_DTYPE_BF16 = 2
AAE_MAX_LAYERS = 8
AAE_SCAN_AUTO, AAE_SCAN_GEMV, AAE_SCAN_MFMA, AAE_SCAN_STREAM, AAE_SCAN_STREAM_2L, AAE_SCAN_AUTO_NO_PRUNE, AAE_SCAN_STREAM_WALK = 0, 1, 2, 3, 4, 5, 6
AAE_SCAN_AUTO_PACKED, AAE_SCAN_AUTO_RH2, AAE_SCAN_AUTO_FIN, AAE_SCAN_AUTO_TOPK_ROWS = 7, 8, 9, 10
AAE_ABI_VERSION = 3
AAE_MODEL_RECONST, AAE_MODEL_CAD = 0, 1
AAE_SCENE_MAX_DRAWS = 256
AAE_ICP_MAX_PROBLEMS, AAE_ICP_MAX_POINTS = 16, 4096
AAE_ICP_DEPTH_ONLY, AAE_ICP_NO_DEPTH, AAE_ICP_NO_DEPTH_ZERO_T = 1, 2, 4
AAE_AUGMENT_MAX_OPS, AAE_AUGMENT_MAX_BLUR_K = 16, 15
AAE_AUGMENT_AFFINE, AAE_AUGMENT_DROPOUT, AAE_AUGMENT_BLUR, AAE_AUGMENT_ADD = 1, 2, 3, 4
AAE_AUGMENT_INVERT, AAE_AUGMENT_MULTIPLY, AAE_AUGMENT_CONTRAST = 5, 6, 7
AAE_LOSS_L2, AAE_LOSS_L1 = 0, 1
AAE_LOSS_MAX_BATCH, AAE_LOSS_MAX_N, AAE_LOSS_MAX_LATENT = 65536, 4194304, 1048576

LIB_NAME = 'libaae_hip.so'
# the same sources with -DAAE_EXPERIMENTS: every kernel variant that measured slower than the defaults + the profiling / ablation
# aids (tools/, the A/B tests).  Chosen for the whole process by AAE_EXPERIMENTS=1 in the environment; never the default.
EXPERIMENTS_LIB_NAME = 'libaae_hip_experiments.so'


def experiments_requested():
    return os.environ.get('AAE_EXPERIMENTS', '0') not in ('', '0')

# every symbol include/aae_hip.h declares (tests check the .so exports all of them)
EXPORTED_SYMBOLS = (
    'aae_abi_version', 'aae_has_experiments', 'aae_last_error',
    'aae_encoder_create', 'aae_encoder_destroy', 'aae_encoder_set_option', 'aae_encoder_workspace_bytes', 'aae_encoder_forward',
    'aae_encoder_forward_timed', 'aae_encoder_kernel_label', 'aae_encoder_kernel_flops',
    'aae_encoder_activation_info', 'aae_encoder_debug_timeline', 'aae_encoder_x3h_saturated', 'aae_encoder_x3h_last_slot', 'aae_encoder_x3h_poll',
    'aae_encoder_x3h_release_slot',
    'aae_encoder_split_precision_for_batch',
    'aae_codebook_create', 'aae_codebook_update', 'aae_codebook_destroy', 'aae_codebook_set_scan_mode',
    'aae_codebook_prepare_upright',
    'aae_codebook_workspace_bytes', 'aae_codebook_nn', 'aae_codebook_nn_timed', 'aae_codebook_last_launches', 'aae_encode_nn', 'aae_encode_nn_topk', 'aae_detect_nn', 'aae_codebook_similarity', 'aae_l2_normalize',
    'aae_crop_resize_u8', 'aae_pack_pairs', 'aae_unpack_pairs',
    'aae_multi_workspace_bytes', 'aae_multi_rows', 'aae_encode_nn_multi', 'aae_codebook_nn_multi', 'aae_detect_nn_multi', 'aae_multi_last_launches',
    'aae_decoder_create', 'aae_decoder_destroy', 'aae_decoder_workspace_bytes', 'aae_decoder_forward',
    'aae_decoder_forward_timed', 'aae_decoder_kernel_label', 'aae_decoder_kernel_flops', 'aae_decoder_activation_info',
    'aae_mesh_create', 'aae_mesh_destroy', 'aae_render_workspace_bytes', 'aae_render_embedding_views', 'aae_render_embedding_views_timed',
    'aae_render_frames', 'aae_render_training_workspace_bytes', 'aae_render_training_views', 'aae_render_training_views_timed',
    'aae_mesh_set_create', 'aae_mesh_set_destroy', 'aae_render_scenes_workspace_bytes', 'aae_render_scenes', 'aae_render_scenes_timed',
    'aae_overlay_blend',
    'aae_icp_workspace_bytes', 'aae_icp_workspace_info', 'aae_icp_prepare', 'aae_icp_refine', 'aae_icp_refine_timed',
    'aae_augment_max_image_bytes', 'aae_augment_batch',
    'aae_recon_loss_workspace_bytes', 'aae_recon_loss', 'aae_latent_reg_loss',
    'aae_upconv_backward_workspace_bytes', 'aae_upconv_backward', 'aae_dense_backward_workspace_bytes', 'aae_dense_backward',
    'aae_decoder_get_desc', 'aae_decoder_backward_workspace_bytes', 'aae_decoder_backward', 'aae_decoder_backward_timed',
    'aae_decoder_bwd_label_count', 'aae_decoder_bwd_label',
    'aae_conv_backward_workspace_bytes', 'aae_conv_backward', 'aae_linear_backward_workspace_bytes', 'aae_linear_backward',
    'aae_encoder_get_desc', 'aae_encoder_backward_workspace_bytes', 'aae_encoder_backward', 'aae_encoder_backward_timed',
    'aae_encoder_bwd_label_count', 'aae_encoder_bwd_label',
)


class EncoderDesc(Structure):
    _fields_ = [
        ('in_h', c_int32), ('in_w', c_int32), ('in_c', c_int32),
        ('num_layers', c_int32),
        ('num_filters', c_int32 * AAE_MAX_LAYERS),
        ('strides', c_int32 * AAE_MAX_LAYERS),
        ('kernel_size', c_int32),
        ('latent_size', c_int32),
        ('batch_norm', c_int32),
        ('bn_eps', c_float),
    ]


class DecoderDesc(Structure):
    _fields_ = [
        ('out_h', c_int32), ('out_w', c_int32), ('out_c', c_int32),
        ('num_layers', c_int32),
        ('num_filters', c_int32 * AAE_MAX_LAYERS),
        ('strides', c_int32 * AAE_MAX_LAYERS),
        ('kernel_size', c_int32),
        ('latent_size', c_int32),
        ('batch_norm', c_int32),
        ('bn_eps', c_float),
    ]


class RenderParams(Structure):
    """aae_render_params"""
    _fields_ = [('K', c_double * 9), ('t', c_double * 3), ('W', c_int32), ('H', c_int32), ('clip_near', c_double), ('clip_far', c_double),
                ('pad_factor', c_double), ('light', c_float * 3), ('ambient', c_float), ('diffuse', c_float), ('specular', c_float)]


class IcpShape(Structure):
    """aae_icp_shape"""
    _fields_ = [('n_problems', c_int32), ('max_points', c_int32), ('W', c_int32), ('H', c_int32), ('crop_w', c_int32), ('crop_h', c_int32)]


class AugmentOp(Structure):
    """aae_augment_op"""
    _fields_ = [('code', c_int32), ('i', c_int32 * 4), ('f', c_float * 3)]


class AugmentShape(Structure):
    """aae_augment_shape"""
    _fields_ = [('N', c_int32), ('M', c_int32), ('H', c_int32), ('W', c_int32), ('C', c_int32), ('B', c_int32), ('aux_words', c_int32)]


class ReconLossDesc(Structure):
    """aae_recon_loss_desc"""
    _fields_ = [('B', c_int32), ('n', c_int32), ('kind', c_int32), ('bootstrap_ratio', c_int32)]


class UpconvBackwardDesc(Structure):
    """aae_upconv_backward_desc"""
    _fields_ = [('B', c_int32), ('H', c_int32), ('W', c_int32), ('Cin', c_int32), ('UH', c_int32), ('UW', c_int32), ('Cout', c_int32), ('KS', c_int32),
                ('act', c_int32)]


class DenseBackwardDesc(Structure):
    """aae_dense_backward_desc"""
    _fields_ = [('B', c_int32), ('J', c_int32), ('U', c_int32)]


class ConvBackwardDesc(Structure):
    """aae_conv_backward_desc"""
    _fields_ = [('B', c_int32), ('H', c_int32), ('W', c_int32), ('Cin', c_int32), ('Cout', c_int32), ('KS', c_int32), ('S', c_int32), ('x_dtype', c_int32)]


class MultiItem(Structure):
    """aae_multi_item: (encoder handle, codebook handle, detections of that object in the frame, col_stride)"""
    _fields_ = [('enc', c_void_p), ('cb', c_void_p), ('n', c_int32), ('col_stride', c_int32)]


def declare(lib):
    """Attach argtypes/restypes for every entry point of include/aae_hip.h."""
    lib.aae_abi_version.restype = c_int
    lib.aae_abi_version.argtypes = []
    lib.aae_has_experiments.restype = c_int
    lib.aae_has_experiments.argtypes = []
    lib.aae_last_error.restype = c_char_p
    lib.aae_last_error.argtypes = []

    lib.aae_encoder_create.restype = c_int
    lib.aae_encoder_create.argtypes = [POINTER(EncoderDesc), POINTER(c_void_p), c_int, POINTER(c_void_p)]
    lib.aae_encoder_destroy.restype = None
    lib.aae_encoder_destroy.argtypes = [c_void_p]
    lib.aae_encoder_set_option.restype = c_int
    lib.aae_encoder_set_option.argtypes = [c_void_p, c_char_p, c_int]
    lib.aae_encoder_workspace_bytes.restype = c_size_t
    lib.aae_encoder_workspace_bytes.argtypes = [c_void_p, c_int]
    lib.aae_encoder_forward.restype = c_int
    lib.aae_encoder_forward.argtypes = [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_size_t, c_void_p]
    lib.aae_encoder_forward_timed.restype = c_int
    lib.aae_encoder_forward_timed.argtypes = [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_size_t, c_void_p,
                                              POINTER(c_float), c_int, POINTER(c_int)]
    lib.aae_encoder_kernel_label.restype = c_char_p
    lib.aae_encoder_kernel_label.argtypes = [c_void_p, c_int]
    lib.aae_encoder_kernel_flops.restype = c_double
    lib.aae_encoder_kernel_flops.argtypes = [c_void_p, c_int]
    lib.aae_encoder_split_precision_for_batch.restype = c_int
    lib.aae_encoder_split_precision_for_batch.argtypes = [c_void_p, c_int]
    lib.aae_encoder_x3h_saturated.restype = c_int
    lib.aae_encoder_x3h_saturated.argtypes = [c_void_p, POINTER(c_int), c_void_p]
    lib.aae_encoder_x3h_last_slot.restype = c_int
    lib.aae_encoder_x3h_last_slot.argtypes = []
    lib.aae_encoder_x3h_poll.restype = c_int
    lib.aae_encoder_x3h_poll.argtypes = [c_void_p, POINTER(c_int), c_int, POINTER(c_int), c_void_p]
    lib.aae_encoder_x3h_release_slot.restype = c_int
    lib.aae_encoder_x3h_release_slot.argtypes = [c_void_p, c_int, c_void_p]
    lib.aae_encoder_debug_timeline.restype = c_int
    lib.aae_encoder_debug_timeline.argtypes = [c_void_p, POINTER(c_int64)]
    lib.aae_encoder_activation_info.restype = c_int
    lib.aae_encoder_activation_info.argtypes = [c_void_p, c_int, c_int, POINTER(c_size_t), POINTER(c_size_t)]

    lib.aae_codebook_create.restype = c_int
    lib.aae_codebook_create.argtypes = [c_void_p, c_int, c_int, c_int, c_int, POINTER(c_void_p)]
    lib.aae_codebook_update.restype = c_int
    lib.aae_codebook_update.argtypes = [c_void_p, c_void_p, c_int, c_void_p]
    lib.aae_codebook_destroy.restype = None
    lib.aae_codebook_destroy.argtypes = [c_void_p]
    lib.aae_codebook_set_scan_mode.restype = c_int
    lib.aae_codebook_set_scan_mode.argtypes = [c_void_p, c_int]
    lib.aae_codebook_prepare_upright.restype = c_int
    lib.aae_codebook_prepare_upright.argtypes = [c_void_p, c_int, c_void_p]
    lib.aae_codebook_workspace_bytes.restype = c_size_t
    lib.aae_codebook_workspace_bytes.argtypes = [c_void_p, c_int, c_int]
    lib.aae_pack_pairs.restype = c_int
    lib.aae_pack_pairs.argtypes = [c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p]
    lib.aae_unpack_pairs.restype = c_int
    lib.aae_unpack_pairs.argtypes = [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p]
    lib.aae_encode_nn.restype = c_int
    lib.aae_encode_nn.argtypes = [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t,
                                  c_void_p, c_size_t, c_void_p]
    lib.aae_encode_nn_topk.restype = c_int
    lib.aae_encode_nn_topk.argtypes = [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t,
                                       c_void_p, c_size_t, c_void_p]
    lib.aae_codebook_last_launches.restype = c_int
    lib.aae_codebook_last_launches.argtypes = []
    lib.aae_codebook_nn.restype = c_int
    lib.aae_codebook_nn.argtypes = [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]
    lib.aae_codebook_nn_timed.restype = c_int
    lib.aae_codebook_nn_timed.argtypes = [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p, c_int, POINTER(c_float)]
    lib.aae_detect_nn.restype = c_int
    lib.aae_detect_nn.argtypes = [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                  c_void_p, c_size_t, c_void_p, c_size_t, c_void_p]
    lib.aae_codebook_similarity.restype = c_int
    lib.aae_codebook_similarity.argtypes = [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_size_t, c_void_p]
    lib.aae_l2_normalize.restype = c_int
    lib.aae_l2_normalize.argtypes = [c_void_p, c_int, c_int, c_void_p, c_void_p]
    lib.aae_crop_resize_u8.restype = c_int
    lib.aae_crop_resize_u8.argtypes = [c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]
    lib.aae_multi_workspace_bytes.restype = c_size_t
    lib.aae_multi_workspace_bytes.argtypes = [POINTER(MultiItem), c_int, c_int]
    lib.aae_multi_rows.restype = c_int
    lib.aae_multi_rows.argtypes = [POINTER(MultiItem), c_int]
    lib.aae_encode_nn_multi.restype = c_int
    lib.aae_encode_nn_multi.argtypes = [POINTER(MultiItem), c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]
    lib.aae_codebook_nn_multi.restype = c_int
    lib.aae_codebook_nn_multi.argtypes = [POINTER(MultiItem), c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]
    lib.aae_detect_nn_multi.restype = c_int
    lib.aae_detect_nn_multi.argtypes = [POINTER(MultiItem), c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                        c_void_p, c_size_t, c_void_p]
    lib.aae_multi_last_launches.restype = c_int
    lib.aae_multi_last_launches.argtypes = []

    lib.aae_decoder_create.restype = c_int
    lib.aae_decoder_create.argtypes = [POINTER(DecoderDesc), POINTER(c_void_p), c_int, POINTER(c_void_p)]
    lib.aae_decoder_destroy.restype = None
    lib.aae_decoder_destroy.argtypes = [c_void_p]
    lib.aae_decoder_workspace_bytes.restype = c_size_t
    lib.aae_decoder_workspace_bytes.argtypes = [c_void_p, c_int]
    lib.aae_decoder_forward.restype = c_int
    lib.aae_decoder_forward.argtypes = [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_size_t, c_void_p]
    lib.aae_decoder_forward_timed.restype = c_int
    lib.aae_decoder_forward_timed.argtypes = [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_size_t, c_void_p,
                                              POINTER(c_float), c_int, POINTER(c_int)]
    lib.aae_decoder_kernel_label.restype = c_char_p
    lib.aae_decoder_kernel_label.argtypes = [c_void_p, c_int]
    lib.aae_decoder_kernel_flops.restype = c_double
    lib.aae_decoder_kernel_flops.argtypes = [c_void_p, c_int]
    lib.aae_decoder_activation_info.restype = c_int
    lib.aae_decoder_activation_info.argtypes = [c_void_p, c_int, c_int, POINTER(c_size_t), POINTER(c_size_t)]
    return lib


def declare_render(lib):
    """The mesh rasteriser's entry points (aae_render.hip: part of the GPU library only, the CPU-emulated build of the host
    sources that the tests load through declare() has no rasteriser)."""
    lib.aae_mesh_create.restype = c_int
    lib.aae_mesh_create.argtypes = [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_int, c_float, POINTER(c_void_p)]
    lib.aae_mesh_destroy.restype = None
    lib.aae_mesh_destroy.argtypes = [c_void_p]
    lib.aae_render_workspace_bytes.restype = c_size_t
    lib.aae_render_workspace_bytes.argtypes = [c_void_p, c_int, c_int, c_int]
    lib.aae_render_embedding_views.restype = c_int
    lib.aae_render_embedding_views.argtypes = [c_void_p, c_void_p, c_int, POINTER(RenderParams), c_int, c_void_p, c_void_p, c_void_p,
                                               c_void_p, c_size_t, c_void_p]
    lib.aae_render_embedding_views_timed.restype = c_int
    lib.aae_render_embedding_views_timed.argtypes = [c_void_p, c_void_p, c_int, POINTER(RenderParams), c_int, c_void_p, c_void_p, c_void_p,
                                                     c_void_p, c_size_t, c_void_p, POINTER(c_float)]
    lib.aae_render_frames.restype = c_int
    lib.aae_render_frames.argtypes = [c_void_p, c_void_p, c_void_p, c_int, POINTER(RenderParams), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                      c_void_p, c_size_t, c_void_p]
    lib.aae_render_training_workspace_bytes.restype = c_size_t
    lib.aae_render_training_workspace_bytes.argtypes = [c_void_p, c_int, c_int, c_int]
    training = [c_void_p, c_void_p, c_void_p, c_void_p, c_int, POINTER(RenderParams), c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                c_void_p, c_size_t, c_void_p]
    lib.aae_render_training_views.restype = c_int
    lib.aae_render_training_views.argtypes = training
    lib.aae_render_training_views_timed.restype = c_int
    lib.aae_render_training_views_timed.argtypes = training + [POINTER(c_float)]
    lib.aae_mesh_set_create.restype = c_int
    lib.aae_mesh_set_create.argtypes = [POINTER(c_void_p), c_int, POINTER(c_void_p)]
    lib.aae_mesh_set_destroy.restype = None
    lib.aae_mesh_set_destroy.argtypes = [c_void_p]
    lib.aae_render_scenes_workspace_bytes.restype = c_size_t
    lib.aae_render_scenes_workspace_bytes.argtypes = [c_void_p, c_int, c_int, c_int, c_int]
    scenes = [c_void_p, POINTER(c_int32), POINTER(c_int32), c_void_p, c_void_p, c_int, c_int, POINTER(RenderParams), c_void_p, c_void_p, c_void_p,
              c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]
    lib.aae_render_scenes.restype = c_int
    lib.aae_render_scenes.argtypes = scenes
    lib.aae_render_scenes_timed.restype = c_int
    lib.aae_render_scenes_timed.argtypes = scenes + [POINTER(c_float)]
    lib.aae_overlay_blend.restype = c_int
    lib.aae_overlay_blend.argtypes = [c_void_p, c_void_p, c_size_t, c_int, c_void_p, c_void_p]
    return lib


def declare_icp(lib):
    """The depth refinement's entry points (aae_icp.hip: like the rasteriser, part of the GPU library only)."""
    lib.aae_icp_workspace_bytes.restype = c_size_t
    lib.aae_icp_workspace_bytes.argtypes = [c_int, c_int, c_int, c_int, c_int, c_int]
    lib.aae_icp_workspace_info.restype = c_int
    lib.aae_icp_workspace_info.argtypes = [POINTER(IcpShape), c_int, c_int, POINTER(c_size_t), POINTER(c_size_t)]
    lib.aae_icp_prepare.restype = c_int
    lib.aae_icp_prepare.argtypes = [POINTER(IcpShape), c_void_p, c_void_p, c_void_p, c_void_p, c_double, c_void_p, c_void_p, c_size_t, c_void_p]
    refine = [POINTER(IcpShape), c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_double, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
              c_void_p, c_size_t, c_void_p]
    lib.aae_icp_refine.restype = c_int
    lib.aae_icp_refine.argtypes = refine
    lib.aae_icp_refine_timed.restype = c_int
    lib.aae_icp_refine_timed.argtypes = refine + [POINTER(c_float)]
    return lib


def declare_augment(lib):
    """The training-batch kernel's entry points (aae_augment.hip: like the rasteriser, part of the GPU library only)."""
    lib.aae_augment_max_image_bytes.restype = c_size_t
    lib.aae_augment_max_image_bytes.argtypes = []
    lib.aae_augment_batch.restype = c_int
    lib.aae_augment_batch.argtypes = [POINTER(AugmentShape)] + [c_void_p] * 13
    return lib


def declare_loss(lib):
    """The loss kernels' entry points (aae_loss.hip: like the rasteriser, part of the GPU library only)."""
    lib.aae_recon_loss_workspace_bytes.restype = c_size_t
    lib.aae_recon_loss_workspace_bytes.argtypes = [c_int, c_int]
    lib.aae_recon_loss.restype = c_int
    lib.aae_recon_loss.argtypes = [POINTER(ReconLossDesc), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]
    lib.aae_latent_reg_loss.restype = c_int
    lib.aae_latent_reg_loss.argtypes = [c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p]
    return lib


def declare_decoder_bwd(lib):
    """The decoder's backward pass (aae_decoder_bwd.hip: part of the GPU library only)."""
    lib.aae_upconv_backward_workspace_bytes.restype = c_size_t
    lib.aae_upconv_backward_workspace_bytes.argtypes = [POINTER(UpconvBackwardDesc), c_int]
    lib.aae_upconv_backward.restype = c_int
    lib.aae_upconv_backward.argtypes = [POINTER(UpconvBackwardDesc)] + [c_void_p] * 8 + [c_size_t, c_void_p]
    lib.aae_dense_backward_workspace_bytes.restype = c_size_t
    lib.aae_dense_backward_workspace_bytes.argtypes = [POINTER(DenseBackwardDesc), c_int]
    lib.aae_dense_backward.restype = c_int
    lib.aae_dense_backward.argtypes = [POINTER(DenseBackwardDesc)] + [c_void_p] * 8 + [c_size_t, c_void_p]
    lib.aae_decoder_get_desc.restype = c_int
    lib.aae_decoder_get_desc.argtypes = [c_void_p, POINTER(DecoderDesc)]
    lib.aae_decoder_backward_workspace_bytes.restype = c_size_t
    lib.aae_decoder_backward_workspace_bytes.argtypes = [c_void_p, c_int]
    chain = [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, POINTER(c_void_p), POINTER(c_void_p), c_void_p, c_void_p, c_size_t, c_void_p]
    lib.aae_decoder_backward.restype = c_int
    lib.aae_decoder_backward.argtypes = chain
    lib.aae_decoder_backward_timed.restype = c_int
    lib.aae_decoder_backward_timed.argtypes = chain + [POINTER(c_float), c_int, POINTER(c_int)]
    lib.aae_decoder_bwd_label_count.restype = c_int
    lib.aae_decoder_bwd_label_count.argtypes = []
    lib.aae_decoder_bwd_label.restype = c_char_p
    lib.aae_decoder_bwd_label.argtypes = [c_int]
    return lib


def declare_encoder_bwd(lib):
    """The encoder's backward pass (aae_encoder_bwd.hip: part of the GPU library only)."""
    lib.aae_conv_backward_workspace_bytes.restype = c_size_t
    lib.aae_conv_backward_workspace_bytes.argtypes = [POINTER(ConvBackwardDesc)]
    lib.aae_conv_backward.restype = c_int
    lib.aae_conv_backward.argtypes = [POINTER(ConvBackwardDesc)] + [c_void_p] * 8 + [c_size_t, c_void_p]
    lib.aae_linear_backward_workspace_bytes.restype = c_size_t
    lib.aae_linear_backward_workspace_bytes.argtypes = [POINTER(DenseBackwardDesc), c_int]
    lib.aae_linear_backward.restype = c_int
    lib.aae_linear_backward.argtypes = [POINTER(DenseBackwardDesc)] + [c_void_p] * 7 + [c_size_t, c_void_p]
    lib.aae_encoder_get_desc.restype = c_int
    lib.aae_encoder_get_desc.argtypes = [c_void_p, POINTER(EncoderDesc)]
    lib.aae_encoder_backward_workspace_bytes.restype = c_size_t
    lib.aae_encoder_backward_workspace_bytes.argtypes = [c_void_p, c_int]
    chain = [c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, POINTER(c_void_p), POINTER(c_void_p), c_void_p, c_void_p, c_size_t, c_void_p]
    lib.aae_encoder_backward.restype = c_int
    lib.aae_encoder_backward.argtypes = chain
    lib.aae_encoder_backward_timed.restype = c_int
    lib.aae_encoder_backward_timed.argtypes = chain + [POINTER(c_float), c_int, POINTER(c_int)]
    lib.aae_encoder_bwd_label_count.restype = c_int
    lib.aae_encoder_bwd_label_count.argtypes = []
    lib.aae_encoder_bwd_label.restype = c_char_p
    lib.aae_encoder_bwd_label.argtypes = [c_int]
    return lib


def library_path():
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), EXPERIMENTS_LIB_NAME if experiments_requested() else LIB_NAME)


_LIB = None


def load():
    """Load libaae_hip.so.  torch is imported first so that the library binds to the
    HIP runtime torch already loaded (one runtime per process: device pointers,
    streams and events are shared between torch tensors and our kernels)."""
    global _LIB
    if _LIB is not None:
        return _LIB
    import torch  # noqa: F401  (must precede the dlopen below)
    path = library_path()
    if not os.path.exists(path):
        raise RuntimeError(
            '%s not built: run `python -c "import __graft_entry__ as g; g.build(%s)"` at the repo root '
            '(hipcc --offload-arch=gfx950).  There is no CPU fallback.' % (path, 'experiments=True' if experiments_requested() else ''))
    lib = declare_encoder_bwd(declare_decoder_bwd(declare_loss(declare_augment(declare_icp(declare_render(declare(ctypes.CDLL(path))))))))
    if lib.aae_abi_version() != AAE_ABI_VERSION:
        raise RuntimeError('libaae_hip.so ABI version %d != expected %d' % (lib.aae_abi_version(), AAE_ABI_VERSION))
    _LIB = lib
    return lib


def check(lib, rc, what):
    if rc != AAE_OK:
        msg = lib.aae_last_error()
        msg = msg.decode('utf-8', 'replace') if msg else ''
        if rc in (-1, -2, -4):
            raise ValueError('%s failed (%d): %s' % (what, rc, msg))
        raise RuntimeError('%s failed (%d): %s' % (what, rc, msg))
