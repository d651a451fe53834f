"""ctypes binding of libfr_hip.so (the C ABI of include/fr_rasterizer.h).

The library is the product: if it is missing or cannot be loaded this module raises —
there is no CPU or PyTorch fallback anywhere in the package.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.environ.get("FR_HIP_LIB", os.path.join(_HERE, "libfr_hip.so"))  # FR_HIP_LIB: experiments only

FR_OK = 0
FR_ERR_INVALID_ARGUMENT = 1
FR_ERR_BINNING_CAPACITY = 2
FR_ERR_HIP = 3
FR_ERR_UNSUPPORTED = 4
FR_FLAG_NO_WAIT = 1
FR_FLAG_RAW_ACTIVATIONS = 2
FR_FLAG_FORWARD_ONLY = 4       # fr_forward: a frame no backward follows (no backward hand-off is written)
FR_FLAG_DEPTH_ALPHA = 8        # depth and alpha planes next to the image (fr_aux::out_depth / out_alpha, their gradients)
FR_FLAG_CAMERA_GRAD = 16       # fr_backward: also dL/d(viewmatrix, projmatrix, campos) (fr_aux_camera::d_viewmatrix / d_projmatrix / d_campos)
FR_FLAG_ACCUMULATE_SHIFT = 8   # fr_backward: bit (8 + k) = add into the k-th array of fr_grads
FR_BIND_SHELL = 0              # fr_binding::mode: FateAvatar's barycentric point + shell offset (a zeroed descriptor)
FR_BIND_FACE_LOCAL = 1         # GaussianAvatars': a free position in the face's local frame (fr_binding::local_xyz)
FR_BIND_PHONG = 2              # SplattingAvatar's: a point of the posed mesh's Phong surface (uvd travels in local_xyz)
FR_BIND_DEFORM = 4             # FlashAvatar's: barycentric point + the MLP's ten outputs (deform [N,10] travels in local_xyz); 3 is unassigned

_fp = C.c_void_p  # device pointers travel as integers


class fr_binding(C.Structure):
    _fields_ = [("N", C.c_int32), ("V", C.c_int32), ("F", C.c_int32), ("verts", C.c_void_p), ("faces", C.c_void_p),
                ("face_index", C.c_void_p), ("bary", C.c_void_p), ("face_scale_canonical", C.c_void_p),
                ("shell_len", C.c_float), ("resize_scale", C.c_int32), ("offset", C.c_void_p), ("rotation", C.c_void_p),
                ("scaling", C.c_void_p), ("mode", C.c_int32), ("local_xyz", C.c_void_p)]


class fr_binding_phong(C.Structure):
    """A FR_BIND_PHONG descriptor: fr_binding with the mode's three arrays behind it.  `as_binding()` is the `base` member as
    an fr_binding that SHARES this object's memory (and keeps it alive): what the entry points and fr_aux::binding take."""
    _fields_ = [("base", fr_binding), ("vert_normals", C.c_void_p), ("vert_quats", C.c_void_p), ("face_ratio", C.c_void_p)]

    def as_binding(self) -> fr_binding:
        return fr_binding.from_buffer(self)


class fr_aux(C.Structure):
    _fields_ = [("visible", C.c_void_p), ("grad_accum", C.c_void_p), ("denom", C.c_void_p),
                ("binding", C.POINTER(fr_binding)), ("d_verts", C.c_void_p), ("d_offset", C.c_void_p),
                ("d_rotation", C.c_void_p), ("d_scaling", C.c_void_p), ("overflow_out", C.c_void_p),
                ("d_local_xyz", C.c_void_p),
                ("out_depth", C.c_void_p), ("out_alpha", C.c_void_p), ("dL_ddepth", C.c_void_p), ("dL_dalpha", C.c_void_p),
                ("planes", C.c_void_p)]


class fr_aux_camera(C.Structure):
    """The side block of a backward with FR_FLAG_CAMERA_GRAD: fr_aux with the camera's members behind it.  `as_aux()` is the
    `base` member as an fr_aux that SHARES this object's memory (and keeps it alive): what fr_params::aux points at."""
    _fields_ = [("base", fr_aux), ("d_viewmatrix", C.c_void_p), ("d_projmatrix", C.c_void_p), ("d_campos", C.c_void_p),
                ("camera_workspace", C.c_void_p)]

    def as_aux(self) -> fr_aux:
        return fr_aux.from_buffer(self)


class fr_params(C.Structure):
    _fields_ = [("P", C.c_int32), ("D", C.c_int32), ("M", C.c_int32), ("W", C.c_int32), ("H", C.c_int32),
                ("tan_fovx", C.c_float), ("tan_fovy", C.c_float), ("scale_modifier", C.c_float),
                ("prefiltered", C.c_int32), ("debug", C.c_int32), ("flags", C.c_int32),
                ("aux", C.POINTER(fr_aux))]


FR_ADAM_MAX_SEGMENTS = 16
FR_ADAM_STATE_FLOATS = 576
FR_ADAM_MAX_GRADS = 4
FR_MAX_BATCH = 4


class fr_adam_config(C.Structure):
    _fields_ = [("n_segments", C.c_int32), ("segment_end", C.c_uint64 * FR_ADAM_MAX_SEGMENTS),
                ("segment_lr", C.c_float * FR_ADAM_MAX_SEGMENTS), ("segment_period", C.c_uint32 * FR_ADAM_MAX_SEGMENTS),
                ("segment_split", C.c_uint32 * FR_ADAM_MAX_SEGMENTS), ("segment_lr2", C.c_float * FR_ADAM_MAX_SEGMENTS),
                ("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_double), ("grad_scale", C.c_float),
                ("skip", C.c_void_p * FR_ADAM_MAX_GRADS), ("n_skip", C.c_int32)]


FR_TEX_MAX_LAYERS = 8
FR_TEX_ACT_IDENTITY, FR_TEX_ACT_TANH_SCALE, FR_TEX_ACT_SOFTPLUS_CAP = 0, 1, 2


class fr_tex_layer(C.Structure):
    _fields_ = [("texture", C.c_void_p), ("out", C.c_void_p), ("d_out", C.c_void_p), ("d_texture", C.c_void_p),
                ("channels", C.c_int32), ("activation", C.c_int32), ("a0", C.c_float), ("a1", C.c_float)]


class fr_regularise_config(C.Structure):
    _fields_ = [("scale_weight", C.c_float), ("xyz_weight", C.c_float), ("threshold_scale", C.c_float),
                ("threshold_xyz", C.c_float)]


class fr_mesh_terms_config(C.Structure):
    _fields_ = [("laplacian_weight", C.c_float), ("flame_weight", C.c_float)]


class fr_lbs_terms_config(C.Structure):
    _fields_ = [("weights_weight", C.c_float), ("posedirs_weight", C.c_float), ("shapedirs_weight", C.c_float)]


FR_LBS_MAX_E = 64
FR_LBS_MAX_J = 8
FR_LBS_POSE_FEATURES = 36
FR_NEAREST_MAX_V = 8192


class fr_pose_state(C.Structure):
    _fields_ = [("betas", C.c_void_p), ("pose_feature", C.c_void_p), ("transforms", C.c_void_p)]


class fr_point_lbs(C.Structure):
    _fields_ = [("N", C.c_int32), ("E", C.c_int32), ("J", C.c_int32), ("points", C.c_void_p), ("shapedirs", C.c_void_p),
                ("posedirs", C.c_void_p), ("weights", C.c_void_p), ("canonical", fr_pose_state), ("frame", fr_pose_state)]


FR_MLP_WIDTH = 256
FR_MLP_MAX_LAYERS = 8
FR_MLP_MAX_OUT = 16
FR_MLP_POINT_TILE = 128        # points per workgroup of the MLP's forward and backward-data products
FR_MLP_CHUNK = 256             # points per split-N partial of the MLP's weight gradients


class fr_mlp(C.Structure):
    _fields_ = [("N", C.c_int32), ("L", C.c_int32), ("De", C.c_int32), ("Dc", C.c_int32), ("D_out", C.c_int32),
                ("E", C.c_void_p), ("cond", C.c_void_p), ("weights", C.c_void_p)]


FR_FLAME_MAX_E = 128
FR_FLAME_JOINTS = 5
FR_FLAME_POSE_FEATURES = 36


class fr_flame(C.Structure):
    _fields_ = [("V", C.c_int32), ("NS", C.c_int32), ("NE", C.c_int32), ("parents", C.c_void_p), ("v_template", C.c_void_p),
                ("shapedirs", C.c_void_p), ("posedirs", C.c_void_p), ("J_regressor", C.c_void_p), ("lbs_weights", C.c_void_p),
                ("delta_exp", C.c_void_p), ("delta_posedirs", C.c_void_p), ("delta_vertex", C.c_void_p), ("expression", C.c_void_p),
                ("pose", C.c_void_p)]


FR_VGG_MAX_LAYERS = 16
FR_VGG_LOSS_BLOCKS = 1024
FR_VGG_REDUCE_BYTES = (16 + 1) * 32 * 4 + FR_VGG_LOSS_BLOCKS * 4
FR_VGG_TILE_AUTO, FR_VGG_TILE_64, FR_VGG_TILE_128 = 0, 1, 2
FR_VGG_NO_SPLIT = 4


class fr_vgg_layer(C.Structure):
    _fields_ = [("c_in", C.c_int32), ("c_out", C.c_int32), ("pool_before", C.c_int32), ("tap_after", C.c_int32)]


class fr_vgg(C.Structure):
    _fields_ = [("n_layers", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("size_h", C.c_int32), ("size_w", C.c_int32),
                ("tile", C.c_int32), ("mean", C.c_float * 3), ("std", C.c_float * 3), ("layers", fr_vgg_layer * FR_VGG_MAX_LAYERS),
                ("weights_fwd", C.c_void_p), ("weights_bwd", C.c_void_p), ("image", C.c_void_p), ("target", C.c_void_p)]


class fr_image_loss_config(C.Structure):
    _fields_ = [("rgb_weight", C.c_float), ("dssim_weight", C.c_float)]


class fr_huber_config(C.Structure):
    _fields_ = [("alpha", C.c_float), ("mask_weight", C.c_float)]


class fr_pixel_loss_config(C.Structure):
    _fields_ = [("rgb_weight", C.c_float), ("mse_weight", C.c_float)]


class fr_scale_term_config(C.Structure):
    _fields_ = [("weight", C.c_float), ("scale_threshold", C.c_float), ("max_scaling", C.c_float)]


class fr_scale_ratio_config(C.Structure):
    _fields_ = [("weight", C.c_float), ("scale_threshold", C.c_float)]


class fr_inputs(C.Structure):
    _fields_ = [(n, _fp) for n in ("background", "means3D", "shs", "colors_precomp", "opacities", "scales",
                                   "rotations", "cov3D_precomp", "viewmatrix", "projmatrix", "campos")]


class fr_grads(C.Structure):
    _fields_ = [(n, _fp) for n in ("dL_dmeans2D", "dL_dcolors", "dL_dopacity", "dL_dmeans3D", "dL_dcov3D", "dL_dsh",
                                   "dL_dscales", "dL_drotations")]


class fr_counts(C.Structure):
    _fields_ = [("num_rendered", C.c_uint32), ("num_instances", C.c_uint32), ("max_tile_list", C.c_uint32),
                ("overflow", C.c_uint32)]


EXPORTS = ["fr_create", "fr_destroy", "fr_last_error", "fr_version", "fr_profile_enable", "fr_profile_read", "fr_geometry_bytes", "fr_image_bytes",
           "fr_binning_bytes", "fr_planes_bytes", "fr_camera_grad_workspace_bytes", "fr_forward", "fr_forward_batch", "fr_read_counts", "fr_backward", "fr_backward_batch", "fr_mark_visible", "fr_image_final_T",
           "fr_image_n_contrib", "fr_debug_geometry_field", "fr_debug_binning_region", "fr_debug_selftest_reduce", "fr_knn_workspace_bytes", "fr_knn_mean_dist2", "fr_knn_nearest_dist2", "fr_adam_step", "fr_adam_step_multi", "fr_l1_workspace_bytes", "fr_l1_loss_grad", "fr_l1_loss_grad_batch", "fr_huber_workspace_bytes", "fr_huber_loss_grad", "fr_pixel_loss_workspace_bytes", "fr_pixel_loss_grad", "fr_scale_term_workspace_bytes", "fr_scale_term", "fr_scale_ratio_workspace_bytes", "fr_scale_ratio_term", "fr_regularise_workspace_bytes", "fr_gaussian_regularise", "fr_mesh_terms_workspace_bytes", "fr_mesh_terms", "fr_ssim_window", "fr_image_loss_workspace_bytes", "fr_image_loss_grad", "fr_multi_copy", "fr_scaled_sum", "fr_face_scale",
           "fr_bind_forward", "fr_bind_backward", "fr_bind_backward_local", "fr_bind_backward_phong", "fr_bind_backward_deform", "fr_phong_frame", "fr_bind_backward_phong_frame", "fr_phong_frame_backward_workspace_bytes", "fr_phong_frame_backward", "fr_triwalk", "fr_phong_fit", "fr_texture_corners", "fr_texture_lookup", "fr_texture_lookup_backward",
           "fr_bake_decode", "fr_bake_decode_backward", "fr_rot_term_workspace_bytes", "fr_rot_term",
           "fr_point_lbs_forward", "fr_point_lbs_backward", "fr_point_lbs_pose_workspace_bytes", "fr_point_lbs_backward_pose", "fr_nearest_vertex", "fr_lbs_terms_workspace_bytes", "fr_lbs_terms",
           "fr_mlp_workspace_bytes", "fr_mlp_forward", "fr_mlp_backward",
           "fr_flame_workspace_bytes", "fr_flame_workspace_zeroed_bytes", "fr_flame_forward", "fr_flame_backward",
           "fr_vgg_workspace_bytes", "fr_vgg_loss_grad", "fr_lpips_workspace_bytes", "fr_lpips_loss_grad"]


def build(force: bool = False) -> str:
    """Compile the HIP library for gfx950 (hipcc cross-compiles without a GPU)."""
    cmd = ["make", "-C", os.path.join(_HERE, "csrc"), "-s", "-j8"]
    if force:
        cmd.append("-B")
    subprocess.check_call(cmd)
    return SO_PATH


_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(SO_PATH):
        raise RuntimeError(
            f"{SO_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C fateavatar_amd/csrc`). There is no fallback path.")
    # PyTorch-ROCm ships its own libamdhip64: import it FIRST so that this library binds to the same
    # HIP runtime instance (two runtimes in one process cannot share streams or device pointers).
    import torch  # noqa: F401

    # RTLD_GLOBAL: the compiled `_C` extension (fateavatar_amd/torch_ext.py) links against this library by name
    L = C.CDLL(SO_PATH, mode=C.RTLD_GLOBAL)
    L.fr_create.argtypes = [C.POINTER(C.c_void_p)]
    L.fr_create.restype = C.c_int
    L.fr_destroy.argtypes = [C.c_void_p]
    L.fr_last_error.restype = C.c_char_p
    L.fr_version.restype = C.c_char_p
    L.fr_profile_enable.argtypes = [C.c_void_p, C.c_int32]
    L.fr_profile_enable.restype = C.c_int
    L.fr_profile_read.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_uint32)]
    L.fr_profile_read.restype = C.c_int
    L.fr_geometry_bytes.argtypes = [C.c_int32]
    L.fr_geometry_bytes.restype = C.c_size_t
    L.fr_image_bytes.argtypes = [C.c_int32, C.c_int32]
    L.fr_image_bytes.restype = C.c_size_t
    L.fr_binning_bytes.argtypes = [C.c_uint64, C.c_int32, C.c_int32]
    L.fr_binning_bytes.restype = C.c_size_t
    L.fr_planes_bytes.argtypes = [C.c_uint64, C.c_int32, C.c_int32]
    L.fr_planes_bytes.restype = C.c_size_t
    L.fr_camera_grad_workspace_bytes.argtypes = []
    L.fr_camera_grad_workspace_bytes.restype = C.c_size_t
    L.fr_forward.argtypes = [C.c_void_p, C.POINTER(fr_params), C.POINTER(fr_inputs), _fp, _fp, _fp, _fp, _fp,
                             C.c_uint64, C.POINTER(fr_counts), C.c_void_p]
    L.fr_forward.restype = C.c_int
    # batched frames: arrays (one entry per view) of what fr_forward / fr_backward take
    _pp = C.POINTER(C.c_void_p)
    L.fr_forward_batch.argtypes = [C.c_int32, _pp, C.POINTER(C.POINTER(fr_params)), C.POINTER(C.POINTER(fr_inputs)), _pp, _pp,
                                   _pp, _pp, _pp, C.POINTER(C.c_uint64), C.POINTER(fr_counts), C.c_void_p]
    L.fr_forward_batch.restype = C.c_int
    L.fr_backward_batch.argtypes = [C.c_int32, _pp, C.POINTER(C.POINTER(fr_params)), C.POINTER(C.POINTER(fr_inputs)), _pp, _pp,
                                    _pp, _pp, _pp, C.POINTER(C.POINTER(fr_grads)), C.c_void_p]
    L.fr_backward_batch.restype = C.c_int
    L.fr_read_counts.argtypes = [C.c_void_p, C.POINTER(fr_counts)]
    L.fr_read_counts.restype = C.c_int
    L.fr_backward.argtypes = [C.c_void_p, C.POINTER(fr_params), C.POINTER(fr_inputs), _fp, _fp, _fp, _fp, _fp,
                              C.POINTER(fr_grads), C.c_void_p]
    L.fr_backward.restype = C.c_int
    L.fr_mark_visible.argtypes = [C.c_int32, _fp, _fp, _fp, _fp, C.c_void_p]
    L.fr_mark_visible.restype = C.c_int
    L.fr_image_final_T.argtypes = [_fp, C.c_int32, C.c_int32]
    L.fr_image_final_T.restype = C.c_void_p
    L.fr_image_n_contrib.argtypes = [_fp, C.c_int32, C.c_int32]
    L.fr_image_n_contrib.restype = C.c_void_p
    L.fr_debug_geometry_field.argtypes = [_fp, C.c_int32, C.c_int32]
    L.fr_debug_geometry_field.restype = C.c_void_p
    L.fr_debug_binning_region.argtypes = [_fp, C.c_uint64, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_size_t)]
    L.fr_debug_binning_region.restype = C.c_void_p
    L.fr_debug_selftest_reduce.argtypes = [_fp, _fp, C.c_void_p]
    L.fr_debug_selftest_reduce.restype = C.c_int
    L.fr_knn_workspace_bytes.argtypes = [C.c_int32]
    L.fr_knn_workspace_bytes.restype = C.c_size_t
    L.fr_knn_mean_dist2.argtypes = [C.c_int32, _fp, _fp, _fp, C.c_size_t, C.c_void_p]
    L.fr_knn_mean_dist2.restype = C.c_int
    L.fr_knn_nearest_dist2.argtypes = [C.c_int32, _fp, _fp, _fp, C.c_size_t, C.c_void_p]
    L.fr_knn_nearest_dist2.restype = C.c_int
    L.fr_face_scale.argtypes = [C.c_int32, C.c_int32, _fp, _fp, _fp, C.c_void_p]
    L.fr_face_scale.restype = C.c_int
    L.fr_bind_forward.argtypes = [C.POINTER(fr_binding), _fp, _fp, _fp, C.c_void_p]
    L.fr_bind_forward.restype = C.c_int
    L.fr_bind_backward.argtypes = [C.POINTER(fr_binding), _fp, _fp, _fp, _fp, _fp, _fp, _fp, C.c_void_p]
    L.fr_bind_backward.restype = C.c_int
    L.fr_bind_backward_local.argtypes = [C.POINTER(fr_binding), _fp, _fp, _fp, _fp, _fp, _fp, _fp, C.c_void_p]
    L.fr_bind_backward_local.restype = C.c_int
    L.fr_bind_backward_phong.argtypes = [C.POINTER(fr_binding), _fp, _fp, _fp, _fp, _fp, _fp, _fp, C.c_void_p]
    L.fr_bind_backward_phong.restype = C.c_int
    L.fr_bind_backward_deform.argtypes = [C.POINTER(fr_binding), _fp, _fp, _fp, _fp, _fp, _fp, _fp, C.c_void_p]
    L.fr_bind_backward_deform.restype = C.c_int
    L.fr_phong_frame.argtypes = [C.c_int32, C.c_int32, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp, C.c_void_p]
    L.fr_phong_frame.restype = C.c_int
    L.fr_bind_backward_phong_frame.argtypes = [C.POINTER(fr_binding), _fp, _fp, _fp, _fp, _fp, _fp, _fp, C.c_void_p]
    L.fr_bind_backward_phong_frame.restype = C.c_int
    L.fr_phong_frame_backward_workspace_bytes.argtypes = [C.c_int32, C.c_int32]
    L.fr_phong_frame_backward_workspace_bytes.restype = C.c_size_t
    L.fr_phong_frame_backward.argtypes = [C.c_int32, C.c_int32] + [_fp] * 11 + [C.c_void_p]
    L.fr_phong_frame_backward.restype = C.c_int
    # (the stream is the FIRST argument of these two: `launch_first`)
    L.fr_triwalk.argtypes = [C.c_void_p, _fp, C.c_int32, C.c_int32, _fp, _fp, _fp, C.c_int32, C.c_float, _fp]
    L.fr_triwalk.restype = C.c_int
    L.fr_phong_fit.argtypes = [C.c_void_p, _fp, _fp, _fp, _fp, C.c_int32, C.c_int32, C.c_int32, _fp, _fp, _fp, C.c_int32, C.c_int32,
                               C.c_float, _fp, _fp, _fp]
    L.fr_phong_fit.restype = C.c_int
    L.fr_texture_corners.argtypes = [C.c_int32, _fp, C.c_int32, C.c_int32, _fp, C.c_void_p]
    L.fr_texture_corners.restype = C.c_int
    L.fr_texture_lookup.argtypes = [C.c_int32, _fp, C.c_int32, C.c_int32, C.c_int32, C.POINTER(fr_tex_layer), C.c_void_p]
    L.fr_texture_lookup.restype = C.c_int
    L.fr_texture_lookup_backward.argtypes = [C.c_int32, _fp, C.c_int32, C.c_int32, _fp, _fp, C.c_int32, C.POINTER(fr_tex_layer),
                                             C.c_void_p]
    L.fr_texture_lookup_backward.restype = C.c_int
    L.fr_bake_decode.argtypes = [C.c_int32, _fp, C.c_int32, C.c_int32, _fp, C.c_float, C.c_float, _fp, _fp, _fp, _fp, _fp, C.c_void_p]
    L.fr_bake_decode.restype = C.c_int
    L.fr_bake_decode_backward.argtypes = [C.c_int32, _fp, C.c_int32, C.c_int32, _fp, _fp, _fp, C.c_float, C.c_float, _fp, _fp, _fp, _fp,
                                          _fp, _fp, C.c_void_p]
    L.fr_bake_decode_backward.restype = C.c_int
    L.fr_rot_term_workspace_bytes.argtypes = []
    L.fr_rot_term_workspace_bytes.restype = C.c_size_t
    L.fr_rot_term.argtypes = [C.c_float, C.c_int32, _fp, _fp, _fp, C.c_void_p, C.c_void_p]
    L.fr_rot_term.restype = C.c_int
    L.fr_adam_step.argtypes = [C.POINTER(fr_adam_config), _fp, _fp, _fp, _fp, C.c_uint64, _fp, C.c_void_p]
    L.fr_adam_step.restype = C.c_int
    L.fr_adam_step_multi.argtypes = [C.POINTER(fr_adam_config), _fp, C.POINTER(C.c_void_p), C.c_int32, _fp, _fp, C.c_uint64, _fp,
                                     C.c_void_p]
    L.fr_adam_step_multi.restype = C.c_int
    L.fr_l1_workspace_bytes.argtypes = []
    L.fr_l1_workspace_bytes.restype = C.c_size_t
    L.fr_l1_loss_grad.argtypes = [C.c_uint64, _fp, _fp, _fp, _fp, C.c_void_p, C.c_void_p]
    L.fr_l1_loss_grad.restype = C.c_int
    L.fr_l1_loss_grad_batch.argtypes = [C.c_int32, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.fr_l1_loss_grad_batch.restype = C.c_int
    L.fr_huber_workspace_bytes.argtypes = []
    L.fr_huber_workspace_bytes.restype = C.c_size_t
    L.fr_huber_loss_grad.argtypes = [C.POINTER(fr_huber_config), C.c_int32, C.c_int32, C.c_int32, _fp, _fp, _fp, _fp, _fp, C.c_void_p,
                                     C.c_void_p]
    L.fr_huber_loss_grad.restype = C.c_int
    L.fr_pixel_loss_workspace_bytes.argtypes = []
    L.fr_pixel_loss_workspace_bytes.restype = C.c_size_t
    L.fr_pixel_loss_grad.argtypes = [C.POINTER(fr_pixel_loss_config), C.c_int32, C.c_int32, C.c_int32, _fp, _fp, _fp, _fp, C.c_void_p,
                                     C.c_void_p]
    L.fr_pixel_loss_grad.restype = C.c_int
    L.fr_scale_term_workspace_bytes.argtypes = []
    L.fr_scale_term_workspace_bytes.restype = C.c_size_t
    L.fr_scale_term.argtypes = [C.POINTER(fr_scale_term_config), C.c_int32, _fp, _fp, _fp, C.c_void_p, C.c_void_p]
    L.fr_scale_term.restype = C.c_int
    L.fr_scale_ratio_workspace_bytes.argtypes = []
    L.fr_scale_ratio_workspace_bytes.restype = C.c_size_t
    L.fr_scale_ratio_term.argtypes = [C.POINTER(fr_scale_ratio_config), C.c_int32, _fp, _fp, _fp, C.c_void_p, C.c_void_p]
    L.fr_scale_ratio_term.restype = C.c_int
    L.fr_regularise_workspace_bytes.argtypes = []
    L.fr_regularise_workspace_bytes.restype = C.c_size_t
    L.fr_gaussian_regularise.argtypes = [C.POINTER(fr_regularise_config), C.c_int32, _fp, _fp, _fp, _fp, _fp, C.c_void_p, C.c_void_p]
    L.fr_gaussian_regularise.restype = C.c_int
    L.fr_mesh_terms_workspace_bytes.argtypes = []
    L.fr_mesh_terms_workspace_bytes.restype = C.c_size_t
    L.fr_mesh_terms.argtypes = [C.POINTER(fr_mesh_terms_config), C.c_int32, _fp, _fp, _fp, _fp, _fp, _fp, C.c_void_p, C.c_void_p]
    L.fr_mesh_terms.restype = C.c_int
    L.fr_point_lbs_forward.argtypes = [C.POINTER(fr_point_lbs), _fp, C.c_void_p]
    L.fr_point_lbs_forward.restype = C.c_int
    L.fr_point_lbs_backward.argtypes = [C.POINTER(fr_point_lbs), _fp, _fp, _fp, _fp, _fp, C.c_void_p]
    L.fr_point_lbs_backward.restype = C.c_int
    L.fr_point_lbs_pose_workspace_bytes.argtypes = []
    L.fr_point_lbs_pose_workspace_bytes.restype = C.c_size_t
    L.fr_point_lbs_backward_pose.argtypes = [C.POINTER(fr_point_lbs), _fp, _fp, _fp, _fp, C.c_void_p, C.c_void_p]
    L.fr_point_lbs_backward_pose.restype = C.c_int
    L.fr_nearest_vertex.argtypes = [C.c_int32, _fp, C.c_int32, _fp, _fp, _fp, C.c_void_p]
    L.fr_nearest_vertex.restype = C.c_int
    L.fr_lbs_terms_workspace_bytes.argtypes = []
    L.fr_lbs_terms_workspace_bytes.restype = C.c_size_t
    L.fr_lbs_terms.argtypes = [C.POINTER(fr_lbs_terms_config), C.c_int32, C.c_int32, C.c_int32, C.c_int32] + [_fp] * 11 + \
        [C.c_void_p, C.c_void_p]
    L.fr_lbs_terms.restype = C.c_int
    L.fr_mlp_workspace_bytes.argtypes = [C.c_int32, C.c_int32]
    L.fr_mlp_workspace_bytes.restype = C.c_size_t
    L.fr_mlp_forward.argtypes = [C.POINTER(fr_mlp), _fp, _fp, C.c_void_p]
    L.fr_mlp_forward.restype = C.c_int
    L.fr_mlp_backward.argtypes = [C.POINTER(fr_mlp), _fp, _fp, _fp, _fp, C.c_void_p]
    L.fr_mlp_backward.restype = C.c_int
    L.fr_flame_workspace_bytes.argtypes = [C.c_int32, C.c_int32]
    L.fr_flame_workspace_bytes.restype = C.c_size_t
    L.fr_flame_workspace_zeroed_bytes.argtypes = []
    L.fr_flame_workspace_zeroed_bytes.restype = C.c_size_t
    L.fr_flame_forward.argtypes = [C.POINTER(fr_flame), _fp, _fp, _fp, _fp, _fp, C.c_void_p]
    L.fr_flame_forward.restype = C.c_int
    L.fr_flame_backward.argtypes = [C.POINTER(fr_flame), _fp, _fp, _fp, _fp, _fp, _fp, _fp, C.c_void_p]
    L.fr_flame_backward.restype = C.c_int
    L.fr_vgg_workspace_bytes.argtypes = [C.POINTER(fr_vgg)]
    L.fr_vgg_workspace_bytes.restype = C.c_size_t
    L.fr_vgg_loss_grad.argtypes = [C.POINTER(fr_vgg), C.c_float, C.c_int, _fp, _fp, C.c_void_p, C.c_void_p]
    L.fr_vgg_loss_grad.restype = C.c_int
    L.fr_lpips_workspace_bytes.argtypes = [C.POINTER(fr_vgg)]
    L.fr_lpips_workspace_bytes.restype = C.c_size_t
    L.fr_lpips_loss_grad.argtypes = [C.POINTER(fr_vgg), _fp, C.c_float, C.c_int, _fp, _fp, C.c_void_p, C.c_void_p]
    L.fr_lpips_loss_grad.restype = C.c_int
    L.fr_ssim_window.argtypes = [C.POINTER(C.c_float)]
    L.fr_ssim_window.restype = None
    L.fr_image_loss_workspace_bytes.argtypes = [C.c_int32, C.c_int32, C.c_int32]
    L.fr_image_loss_workspace_bytes.restype = C.c_size_t
    L.fr_image_loss_grad.argtypes = [C.POINTER(fr_image_loss_config), C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.fr_image_loss_grad.restype = C.c_int
    L.fr_multi_copy.argtypes = [C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_uint64), C.c_void_p]
    L.fr_multi_copy.restype = C.c_int
    L.fr_scaled_sum.argtypes = [C.c_int32, C.POINTER(C.c_void_p), _fp, C.c_uint64, C.c_float, C.c_void_p]
    L.fr_scaled_sum.restype = C.c_int
    _lib = L
    return L


STAGES = ("preprocess_fwd", "scan", "emit", "tile_sort", "blend_fwd", "blend_bwd", "preprocess_bwd")


def profile_enable(device_index: int, on: bool) -> None:
    rc = lib().fr_profile_enable(handle(device_index), int(on))
    if rc != FR_OK:
        raise RuntimeError(last_error())


def profile_read(device_index: int) -> dict:
    """{stage: (total_ms, launches)} since profile_enable(True); synchronise the device first."""
    out = {}
    for i, name in enumerate(STAGES):
        ms, n = C.c_double(), C.c_uint32()
        rc = lib().fr_profile_read(handle(device_index), i, C.byref(ms), C.byref(n))
        if rc != FR_OK:
            raise RuntimeError(last_error())
        out[name] = (ms.value, n.value)
    return out


def last_error() -> str:
    return lib().fr_last_error().decode("utf-8", "replace")


def check(rc: int, name: str) -> None:
    if rc != FR_OK:
        raise RuntimeError(f"{name} failed (code {rc}): {last_error()}")


def launch(name: str, device, *args) -> None:
    """The entry point `name` on `device`'s current stream (its last argument), checked: how every stream-ordered call of
    the package reaches the library."""
    import torch

    with torch.cuda.device(device):
        rc = getattr(lib(), name)(*args, torch.cuda.current_stream(device).cuda_stream)
    check(rc, name)


def launch_first(name: str, device, *args) -> None:
    """`launch` for an entry point whose stream is its FIRST argument (fr_triwalk, fr_phong_fit)."""
    import torch

    with torch.cuda.device(device):
        rc = getattr(lib(), name)(torch.cuda.current_stream(device).cuda_stream, *args)
    check(rc, name)


_handles: dict = {}


def handle(device_index: int, slot: int = 0):
    """One fr_handle per (device, slot), created with that device current.  Frames of ONE handle are ordered (the handle
    owns per-frame state); frames that are to overlap on the device — several views in flight on several streams — use
    different slots (rasterizer.handle_slot)."""
    key = device_index if slot == 0 else (device_index, slot)
    h = _handles.get(key)
    if h is None:
        import torch

        if torch.cuda.is_current_stream_capturing():
            # fr_create allocates (device + pinned memory, a stream, events): not allowed under capture, and trying
            # would invalidate the caller's capture
            raise RuntimeError(f"rasterizer handle (device {device_index}, slot {slot}) does not exist yet and cannot be "
                               "created while a stream is being captured: run one eager frame through it first")
        with torch.cuda.device(device_index):
            out = C.c_void_p()
            rc = lib().fr_create(C.byref(out))
            if rc != FR_OK:
                raise RuntimeError(f"fr_create failed: {last_error()}")
        h = out
        _handles[key] = h
    return h
