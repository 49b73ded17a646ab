"""ctypes binding of libegotap_hip.so (include/egotap.h).  No CPU fallback: if the HIP library is
missing or fails to load, everything here raises."""
from __future__ import annotations

import ctypes as C
import os

from . import build as _build

ERR_NAMES = {1: "EGOTAP_ERR_INVALID", 2: "EGOTAP_ERR_HIP", 3: "EGOTAP_ERR_UNBOUND", 4: "EGOTAP_ERR_WORKSPACE"}
NET_LIFT, NET_HM_POS, NET_HM_ROT = 0, 1, 2
F32, I64, BF16 = 0, 1, 2                               # egotap.h EGOTAP_F32 / _I64 / _BF16
PRECISIONS = {"f32": 0, "bf16x3": 1, "bf16": 2}      # egotap.h EGOTAP_PREC_*
ABI_VERSION = 2                                       # egotap.h EGOTAP_ABI_VERSION: what egotap_abi_version() of a matching library returns
RGB_FORMS = {0: "none", 1: "heatmaps", 2: "scratch", 3: "handoff"}      # egotap_debug.h EGOTAP_RGB_FORM_*


class EgotapConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "struct_bytes", "n_joints_hm", "estimate_head", "hm_size", "hidden", "vit_dim", "vit_heads", "vit_layers",
        "patch", "pu_hidden")] + [("hm_blocks", C.c_int32 * 4)]      # zeros = resnet18's (2, 2, 2, 2)


class EgotapOcam(C.Structure):                        # egotap.h egotap_ocam: doubles and two lengths
    _fields_ = [("pol", C.c_double * 8), ("invpol", C.c_double * 24)] + [(n, C.c_double) for n in ("xc", "yc", "c", "d", "e", "ue_flip")] + [
        ("n_pol", C.c_int32), ("n_invpol", C.c_int32)]


class EgotapStereoRig(C.Structure):                   # egotap.h egotap_stereo_rig: two models and 21 doubles, 792 bytes
    _fields_ = [("left", EgotapOcam), ("right", EgotapOcam), ("R", C.c_double * 9), ("t", C.c_double * 3), ("affine", (C.c_double * 4) * 2),
                ("min_score", C.c_double)]


class EgotapTrackParams(C.Structure):                 # egotap.h egotap_track_params: twelve doubles and two ints
    _fields_ = [(f"{c}_{n}", C.c_double) for c in ("pose", "root", "joints") for n in ("min_cutoff", "beta", "d_cutoff")] + [
        (n, C.c_double) for n in ("max_disagree", "max_gap", "max_joint_gap")] + [("min_joints", C.c_int32), ("max_hold", C.c_int32)]


class EgotapFuseParams(C.Structure):                  # egotap.h egotap_fuse_params: three doubles and an int
    _fields_ = [(n, C.c_double) for n in ("sigma_ray", "sigma_prior", "max_sigma")] + [("min_joints", C.c_int32)]


class EgotapSkeletonRig(C.Structure):                 # egotap.h egotap_skeleton_rig: 2584 bytes
    _fields_ = [("P", C.c_int32), ("has_mirror", C.c_int32), ("has_fixed_length", C.c_int32), ("frame_rows", C.c_int32 * 3), ("parent", C.c_int32 * 64),
                ("mirror", C.c_int32 * 64), ("rest_pos", (C.c_double * 3) * 64), ("fixed_length", C.c_double * 64)]


class EgotapSkeletonParams(C.Structure):              # egotap.h egotap_skeleton_params: a double and four ints
    _fields_ = [("max_dev", C.c_double), ("window", C.c_int32), ("min_samples", C.c_int32), ("freeze", C.c_int32), ("track_rows", C.c_int32)]


class EgotapSkeletonTwist(C.Structure):               # egotap.h egotap_skeleton_twist: 1808 bytes
    _fields_ = [("pole", C.c_int32 * 64), ("hinge", (C.c_double * 3) * 64), ("bend_lo", C.c_double), ("bend_hi", C.c_double)]


class EgotapOverlayStyle(C.Structure):                # egotap.h egotap_overlay_style: 664 bytes
    _fields_ = [(n, C.c_int32) for n in ("n_marks", "n_bones", "r16", "w16")] + [("min_score", C.c_float), ("heat_rgba", C.c_uint8 * 4),
                ("bones", (C.c_uint8 * 2) * 64), ("mark_rgba", (C.c_uint8 * 4) * 64), ("bone_rgba", (C.c_uint8 * 4) * 64)]


class EgotapYuvSource(C.Structure):                   # egotap.h egotap_yuv_source: seven int32 (then padding) and two int64
    _fields_ = [(n, C.c_int32) for n in ("struct_size", "format", "matrix", "range", "H", "W", "pitch")] + [("uv_offset", C.c_int64), ("frame_stride", C.c_int64)]


class EgotapLensSource(C.Structure):                  # egotap.h egotap_lens_source: eight int32, two device pointers, six fill bytes (then padding), the yuv source
    _fields_ = [(n, C.c_int32) for n in ("struct_size", "format", "H", "W", "model_h", "model_w")] + [("mirror", C.c_int32 * 2), ("map_left", C.c_void_p),
                ("map_right", C.c_void_p), ("fill", (C.c_uint8 * 3) * 2), ("yuv", EgotapYuvSource)]


LENS_FORMATS = {"rgb8": 0, "nv12": 1, "yuyv": 2}     # egotap.h EGOTAP_LENS_RGB8 / _NV12 / _YUYV


class EgotapError(RuntimeError):
    pass


_lib = None

_PROTOS = {
    "egotap_abi_version": (C.c_int, []),
    "egotap_last_error": (C.c_char_p, []),
    "egotap_create": (C.c_int, [C.POINTER(EgotapConfig), C.POINTER(C.c_void_p)]),
    "egotap_destroy": (None, [C.c_void_p]),
    "egotap_bind_param": (C.c_int, [C.c_void_p, C.c_int, C.c_char_p, C.c_void_p, C.c_int64, C.c_int]),
    "egotap_unbound_count": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int)]),
    "egotap_lift_workspace_bytes": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_size_t)]),
    "egotap_lift_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "egotap_lift_predict_pose": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    # ---- stereo RGB -> pose in one call
    "egotap_predict_pose_rgb_workspace_bytes": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    "egotap_predict_pose_rgb": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    # ---- camera bytes: uint8 [B, S0, S0, 3] frames + the fp32 [3][256] value table
    "egotap_rgb_u8_to_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "egotap_hm_forward_u8_workspace_bytes": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_size_t)]),
    "egotap_hm_forward_u8": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                       C.c_size_t, C.c_void_p]),
    "egotap_predict_pose_rgb_u8_workspace_bytes": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    "egotap_predict_pose_rgb_u8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                             C.c_size_t, C.c_void_p]),
    # ---- the sensor's own frames: uint8 [B, H, W, 3] + a source rectangle and a mirror flag per eye
    "egotap_rgb_u8_resize": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int,
                                       C.c_void_p, C.c_void_p, C.c_void_p]),
    "egotap_predict_pose_sensor_u8_workspace_bytes": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    "egotap_predict_pose_sensor_u8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_void_p,
                                                C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    # ---- 2D joints and confidences from the position heatmaps: the operator, and the one-call entries with a keypoints output last
    "egotap_heatmap_peaks": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float), C.c_void_p, C.c_void_p]),
    "egotap_predict_pose_rgb_kp": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p,
                                             C.c_void_p]),
    "egotap_predict_pose_rgb_u8_kp": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                                C.c_size_t, C.c_void_p, C.c_void_p]),
    "egotap_predict_pose_sensor_u8_kp": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_void_p,
                                                   C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    # ---- limb elevation angles and 2D segments from the sin/cos limb heatmaps: the operator, and the _kp entries with a limbs output last
    "egotap_limb_decode": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float), C.c_void_p, C.c_void_p]),
    "egotap_predict_pose_rgb_kpl": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p,
                                              C.c_void_p, C.c_void_p]),
    "egotap_predict_pose_rgb_u8_kpl": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                                 C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]),
    "egotap_predict_pose_sensor_u8_kpl": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_void_p,
                                                    C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]),
    # ---- NV12 / YUYV sensor frames: the descriptor in place of H, W
    "egotap_yuv_u8_resize": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(EgotapYuvSource), C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int,
                                       C.c_void_p, C.c_void_p, C.c_void_p]),
    "egotap_predict_pose_sensor_yuv": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(EgotapYuvSource), C.POINTER(C.c_int), C.POINTER(C.c_int),
                                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "egotap_predict_pose_sensor_yuv_kp": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(EgotapYuvSource), C.POINTER(C.c_int), C.POINTER(C.c_int),
                                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "egotap_predict_pose_sensor_yuv_kpl": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(EgotapYuvSource), C.POINTER(C.c_int), C.POINTER(C.c_int),
                                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]),
    # ---- frames from another lens: the descriptor (format, H, W, the two device maps, fills) in place of H, W, rectangles and mirrors
    "egotap_lens_remap": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(EgotapLensSource), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "egotap_predict_pose_lens_workspace_bytes": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    "egotap_predict_pose_lens": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(EgotapLensSource), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                           C.c_void_p, C.c_size_t, C.c_void_p]),
    "egotap_predict_pose_lens_kp": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(EgotapLensSource), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                              C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "egotap_predict_pose_lens_kpl": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(EgotapLensSource), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                               C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]),
    # ---- the fisheye camera model and the stereo triangulation of the keypoints: three operators, no handle
    "egotap_ocam_project": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(EgotapOcam), C.c_void_p, C.c_void_p]),
    "egotap_ocam_unproject": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(EgotapOcam), C.c_void_p, C.c_void_p]),
    "egotap_stereo_triangulate": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(EgotapOcam), C.POINTER(EgotapOcam), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                            C.POINTER(C.c_double), C.c_double, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    # (keypoints, B, J, left, right, R, t, affine, min_score, pose, P, pose_row0, frame, params, fused, pose_fused, stats, stream)
    "egotap_stereo_fuse": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(EgotapOcam), C.POINTER(EgotapOcam), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                     C.POINTER(C.c_double), C.c_double, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.POINTER(EgotapFuseParams), C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p]),
    # ---- a camera rig per stream: a table of S rigs, or S lens maps per eye, in device memory
    "egotap_stereo_rigs_check": (C.c_int, [C.POINTER(EgotapStereoRig), C.c_int]),
    # (keypoints, B, J, rigs_dev, S, pose, P, pose_row0, joints3d, frame, stream)
    "egotap_stereo_triangulate_streams": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                                    C.c_void_p]),
    # (keypoints, B, J, rigs_dev, S, pose, P, pose_row0, frame, params, fused, pose_fused, stats, stream)
    "egotap_stereo_fuse_streams": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                             C.POINTER(EgotapFuseParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "egotap_lens_remap_streams": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(EgotapLensSource), C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "egotap_predict_pose_lens_streams": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(EgotapLensSource), C.c_int, C.c_void_p, C.c_void_p,
                                                   C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "egotap_predict_pose_lens_streams_kp": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(EgotapLensSource), C.c_int, C.c_void_p, C.c_void_p,
                                                      C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "egotap_predict_pose_lens_streams_kpl": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(EgotapLensSource), C.c_int, C.c_void_p, C.c_void_p,
                                                       C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]),
    # ---- heatmaps, keypoints and bones drawn onto the frames: two operators, no handle
    # (hm, dtype, B, C, S, image_stride, c0, n, groups, heat8, stream)
    "egotap_heat_u8": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    # (left8, right8, B, Hc, Wc, heat8, S, tx_left, ty_left, tx_right, ty_right, marks, style, out_left8, out_right8, stream)
    "egotap_overlay_u8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.POINTER(EgotapOverlayStyle), C.c_void_p, C.c_void_p, C.c_void_p]),
    # ---- the pose, the root and the stereo joints filtered over time: one operator, no handle
    "egotap_pose_track": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_double, C.POINTER(EgotapTrackParams),
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    # (pose, frame, joints3d, rig_pose, T, S, P, J, dts, dt, params, ortho_tol, state_in, state_out, tracks, placed_world, placed_cam, stream)
    "egotap_pose_track_world": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_double,
                                          C.POINTER(EgotapTrackParams), C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    # ---- a rigid skeleton and bone rotations from the tracked pose: one operator, no handle
    # (points, tracks, T, S, rig, params, state_in, state_out, rigid, rotations, lengths, stream)
    "egotap_skeleton_fit": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(EgotapSkeletonRig), C.POINTER(EgotapSkeletonParams), C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    # (points, tracks, T, S, rig, twist, params, state_in, state_out, rigid, rotations, lengths, stream)
    "egotap_skeleton_fit_twist": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(EgotapSkeletonRig), C.POINTER(EgotapSkeletonTwist),
                                            C.POINTER(EgotapSkeletonParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "egotap_debug_predict_pose_rgb_form": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    "egotap_debug_predict_pose_rgb_intermediate": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_char_p, C.POINTER(C.c_size_t), C.POINTER(C.c_int64)]),
    "egotap_lift_intermediate": (C.c_int, [C.c_void_p, C.c_int, C.c_char_p, C.POINTER(C.c_size_t), C.POINTER(C.c_int64)]),
    "egotap_lift_debug_stop": (C.c_int, [C.c_void_p, C.c_int]),
    "egotap_set_precision": (C.c_int, [C.c_void_p, C.c_int]),
    "egotap_set_pu_chain": (C.c_int, [C.c_void_p, C.c_int]),
    "egotap_pu_chain_status": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "egotap_debug_pu_drop_workgroups": (C.c_int, [C.c_void_p, C.c_int]),
    "egotap_debug_pu_train_routes": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.c_int]),
    "egotap_debug_pu_train_routes_for": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int]),
    "egotap_debug_gemm_bk": (C.c_int, [C.c_int]),
    "egotap_debug_conv_addressing": (C.c_int, [C.c_int]),
    "egotap_set_weight_scratch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "egotap_set_act_scratch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    # ---- frozen-weight serving: prepared weights kept in a caller-owned arena
    "egotap_lift_frozen_bytes": (C.c_int, [C.c_void_p, C.POINTER(C.c_size_t)]),
    "egotap_lift_freeze": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "egotap_lift_unfreeze": (C.c_int, [C.c_void_p]),
    "egotap_hm_frozen_bytes": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    "egotap_hm_freeze": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "egotap_hm_unfreeze": (C.c_int, [C.c_void_p, C.c_int]),
    "egotap_hm_workspace_bytes": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_size_t)]),
    "egotap_hm_forward": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p,
                                    C.c_size_t, C.c_void_p]),
    "egotap_hm_intermediate": (C.c_int, [C.c_void_p, C.c_int, C.c_char_p, C.POINTER(C.c_size_t), C.POINTER(C.c_int64)]),
    "egotap_hm_forward_bnbatch_workspace_bytes": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    "egotap_hm_forward_bnbatch_intermediate": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_char_p, C.POINTER(C.c_size_t), C.POINTER(C.c_int64)]),
    "egotap_hm_forward_bnbatch": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_int, C.c_void_p,
                                            C.c_size_t, C.c_void_p]),
    "egotap_linear_f32": (C.c_int, [C.c_void_p] * 4 + [C.c_int] * 4 + [C.c_void_p] * 5 + [C.c_int, C.c_void_p]),
    "egotap_gemm_tile_name": (C.c_char_p, [C.c_int]),
    "egotap_linear_bf16_dma": (C.c_int, [C.c_void_p] * 4 + [C.c_int] * 3 + [C.c_void_p]),
    "egotap_layernorm_f32": (C.c_int, [C.c_void_p] * 4 + [C.c_int, C.c_int, C.c_float, C.c_void_p]),
    "egotap_attention_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "egotap_debug_attention_f32_shared": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "egotap_debug_attention_f32_split": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]),
    "egotap_debug_attention_f32_live": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "egotap_debug_attention_f32_ksplit": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_int]),
    "egotap_pose_metrics": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "egotap_pose_metrics_batch_axes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "egotap_attention": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "egotap_synth_heatmaps": (C.c_int, [C.c_void_p] * 4 + [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "egotap_timing_enable": (C.c_int, [C.c_void_p, C.c_int]),
    "egotap_timing_read": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "egotap_timing_detail": (C.c_char_p, [C.c_void_p]),
    # ---- training-step operators
    "egotap_train_gemm_nt": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "egotap_debug_wgrad_splits": (C.c_int, [C.c_int, C.c_int64, C.c_int64, C.c_size_t, C.c_int, C.c_int, C.c_double, C.c_double, C.POINTER(C.c_int)]),
    "egotap_train_gemm_tn_bias": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                           C.c_void_p, C.c_size_t, C.c_void_p]),
    "egotap_train_gemm_tn": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                       C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "egotap_train_colsum": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "egotap_train_transpose": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int64, C.c_void_p]),
    "egotap_train_add_inplace": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "egotap_train_patch_fwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 6),
    "egotap_train_patch_split": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "egotap_train_tokens_scatter": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "egotap_train_layernorm_fwd": (C.c_int, [C.c_void_p] * 6 + [C.c_int, C.c_float, C.c_void_p]),
    "egotap_train_layernorm_bwd": (C.c_int, [C.c_void_p] * 9 + [C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "egotap_train_bn_lrelu_fwd": (C.c_int, [C.c_void_p] * 8 + [C.c_int, C.c_int, C.c_float, C.c_float, C.c_void_p, C.c_size_t, C.c_void_p]),
    "egotap_train_bn_lrelu_bwd": (C.c_int, [C.c_void_p] * 9 + [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "egotap_train_qkv_fwd": (C.c_int, [C.c_void_p] * 9 + [C.c_int, C.c_int, C.c_void_p]),
    "egotap_train_attention_fwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "egotap_train_attention_bwd": (C.c_int, [C.c_void_p] * 6 + [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "egotap_train_pu_saved_bytes": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "egotap_train_pu_fwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "egotap_train_pu_bwd_ws_bytes": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_size_t)]),
    "egotap_train_pu_bwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.POINTER(C.c_void_p), C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "egotap_train_pose_head_fwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "egotap_train_pose_head_bwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 6 + [C.c_int, C.c_void_p]),
    "egotap_train_pose_loss": (C.c_int, [C.c_void_p] * 6 + [C.c_int, C.c_float, C.c_float, C.c_void_p]),
    "egotap_train_adamw": (C.c_int, [C.c_void_p] * 4 + [C.c_int64] + [C.c_double] * 5 + [C.c_int, C.c_void_p]),
    # ---- bf16-storage operators
    "egotap_bf16_gemm_nt": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "egotap_bf16_gemm_tn": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                      C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "egotap_bf16_layernorm_fwd": (C.c_int, [C.c_void_p] * 6 + [C.c_int, C.c_float, C.c_void_p]),
    "egotap_bf16_layernorm_bwd": (C.c_int, [C.c_void_p] * 11 + [C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "egotap_bf16_colsum": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "egotap_bf16_prep_weight": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int64, C.c_void_p]),
    "egotap_bf16_from_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "egotap_bf16_attention_fwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "egotap_bf16_attention_bwd": (C.c_int, [C.c_void_p] * 6 + [C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "egotap_bf16_attention_bwd_bias": (C.c_int, [C.c_void_p] * 9 + [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "egotap_bf16_fc1_fwd": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "egotap_bf16_patch_fwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "egotap_bf16_fc1_wgrad": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "egotap_bf16_fc1_dgrad_tokens": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "egotap_bf16_fc1_dgrad_rot": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "egotap_bf16_patch_dgrad": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "egotap_train_adamw_multi": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64] + [C.c_double] * 5 + [C.c_int, C.c_void_p]),
    "egotap_bind_grad": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_int64]),
    "egotap_lift_train_bytes": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "egotap_lift_forward_train": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]),
    "egotap_lift_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                      C.c_void_p, C.c_int, C.c_void_p]),
    "egotap_lift_backward_dhm": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                          C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    # ---- heatmap-estimator training operators
    "egotap_hmtrain_conv_fwd": (C.c_int, [C.c_void_p] * 6 + [C.c_int] * 7 + [C.c_int64] * 3 + [C.c_void_p]),
    "egotap_hm_conv_bn_fwd": (C.c_int, [C.c_void_p] * 9 + [C.c_int] * 7 + [C.c_int64] * 3 + [C.c_void_p]),
    "egotap_hm_stem_bn_fwd": (C.c_int, [C.c_void_p] * 8 + [C.c_int, C.c_int, C.c_void_p]),
    "egotap_hmtrain_set_pack_buffer": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "egotap_hmtrain_pack_bytes": (C.c_size_t, []),
    "egotap_hmtrain_stem_fwd": (C.c_int, [C.c_void_p] * 4 + [C.c_int, C.c_int, C.c_void_p]),
    "egotap_hmtrain_bn2d_fwd": (C.c_int, [C.c_void_p] * 9 + [C.c_int] * 3 + [C.c_int64] * 3 + [C.c_int, C.c_float, C.c_float, C.c_void_p, C.c_size_t, C.c_void_p]),
    "egotap_hmtrain_bn2d_bwd": (C.c_int, [C.c_void_p] * 10 + [C.c_int] * 3 + [C.c_int64] * 2 + [C.c_int] * 3 + [C.c_void_p, C.c_size_t, C.c_void_p]),
    "egotap_hmtrain_chansum": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "egotap_hmtrain_conv_wt": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "egotap_hmtrain_zero_upsample": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64, C.c_void_p]),
    "egotap_hmtrain_conv_wgrad": (C.c_int, [C.c_void_p] * 3 + [C.c_int] * 6 + [C.c_int64] * 2 + [C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "egotap_hmtrain_relu_bwd": (C.c_int, [C.c_void_p] * 3 + [C.c_int] * 3 + [C.c_int64] * 3 + [C.c_void_p]),
    "egotap_hmtrain_maxpool_bwd": (C.c_int, [C.c_void_p] * 3 + [C.c_int64, C.c_int, C.c_void_p]),
    "egotap_hmtrain_upsample_bwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64, C.c_void_p]),
    "egotap_hmtrain_maxpool_fwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p]),
    "egotap_hmtrain_upsample_fwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64, C.c_void_p]),
    "egotap_hmtrain_mse": (C.c_int, [C.c_void_p] * 5 + [C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_size_t, C.c_void_p]),
}


def exported_symbols():
    """names declared in include/egotap.h that the library must export"""
    return sorted(_PROTOS)


def load(build_if_missing: bool = True):
    global _lib
    if _lib is not None:
        return _lib
    # torch ships its own HIP runtime: import it first so this process has exactly one libamdhip64
    # (loading ours before torch's gives two runtimes and "no ROCm-capable device" at the first launch)
    import torch  # noqa: F401
    path = _build.LIB
    if build_if_missing and not os.path.exists(path):
        # several ranks of one node may get here together (torch.distributed.run): one builds, the others wait on the lock
        import fcntl
        with open(path + ".lock", "w") as lk:
            fcntl.flock(lk, fcntl.LOCK_EX)
            try:
                if not os.path.exists(path):
                    path = _build.build()
            finally:
                fcntl.flock(lk, fcntl.LOCK_UN)
    if not os.path.exists(path):
        raise EgotapError(f"{path} is missing: build it with `python -m egotap_amd.build` (hipcc, gfx950)")
    lib = C.CDLL(path)
    for name, (res, args) in _PROTOS.items():
        fn = getattr(lib, name)      # AttributeError if a declared symbol is not exported
        fn.restype = res
        fn.argtypes = args
    if lib.egotap_abi_version() != ABI_VERSION:
        raise EgotapError("libegotap_hip.so ABI version mismatch")
    _lib = lib
    return lib


def check(rc: int):
    if rc != 0:
        msg = load().egotap_last_error().decode("utf-8", "replace")
        raise EgotapError(f"{ERR_NAMES.get(rc, rc)}: {msg}")


def ptr(t, byte_offset: int = 0):
    """a tensor's device address (plus `byte_offset`) as the ABI takes it; None -> null pointer"""
    return C.c_void_p(t.data_ptr() + byte_offset) if t is not None else C.c_void_p(0)


def stream(dev=None):
    """the current HIP stream of `dev` (None: of the current device) as the ABI takes it"""
    import torch
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


_ptr, _stream = ptr, stream


# ----------------------------------------------------------------------------------------- single operators
def _need_cuda_f32(*ts):
    import torch
    for t in ts:
        if t is None:
            continue
        if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
            raise EgotapError("egotap_amd ops need contiguous float32 tensors on the GPU (no CPU fallback)")


def linear(x, w, b, epi: str = "bias", residual=None, bn=None, tile: int = 0):
    """y = epi(x @ w.T + b) on the fp32 MFMA GEMM.  epi: bias | residual | gelu | bn_lrelu."""
    import torch
    code = {"bias": 0, "residual": 1, "gelu": 2, "bn_lrelu": 3}[epi]
    M, K = x.shape
    N = w.shape[0]
    g = beta = mean = var = None
    if bn is not None:
        g, beta, mean, var = bn
    _need_cuda_f32(x, w, b, residual, g, beta, mean, var)
    y = torch.empty((M, N), device=x.device, dtype=torch.float32)
    check(load().egotap_linear_f32(_ptr(x), _ptr(w), _ptr(b), _ptr(y), M, N, K, code, _ptr(residual), _ptr(g), _ptr(beta),
                                   _ptr(mean), _ptr(var), tile, _stream()))
    return y


def linear_bf16_dma(x_bf16, w_bf16, b):
    """y = x @ w.T + b on the LDS-DMA bf16 kernel; x [M,K], w [N,K] torch.bfloat16 (caller-owned copies), b fp32 -> fp32"""
    import torch
    if not (x_bf16.is_cuda and w_bf16.is_cuda and x_bf16.dtype == torch.bfloat16 and w_bf16.dtype == torch.bfloat16
            and x_bf16.is_contiguous() and w_bf16.is_contiguous()):
        raise EgotapError("linear_bf16_dma needs contiguous bfloat16 operands on the GPU")
    _need_cuda_f32(b)
    (M, K), N = x_bf16.shape, w_bf16.shape[0]
    y = torch.empty((M, N), device=x_bf16.device, dtype=torch.float32)
    check(load().egotap_linear_bf16_dma(_ptr(x_bf16), _ptr(w_bf16), _ptr(b), _ptr(y), M, N, K, _stream()))
    return y


def pose_metrics(pred, gt, want_aligned: bool = False, reference_batch_axes: bool = False):
    """per-sample (mpjpe [B], pa_mpjpe [B][, aligned [B,J,3]]) of poses [B,J,3] in the input units (egotap_pose_metrics).
    reference_batch_axes: for a batch of 2 or 3 frames return what utils/util.py:328-379 returns there -- line 337 skips its transpose
    and aligns the wrong axes (egotap_pose_metrics_batch_axes); other batch sizes are unaffected, as in the reference."""
    import torch
    pred, gt = pred.detach().float().contiguous(), gt.detach().float().contiguous()
    _need_cuda_f32(pred, gt)
    if pred.shape != gt.shape or pred.dim() != 3 or pred.shape[2] != 3:
        raise ValueError(f"expected pred, gt [B, J, 3]; got {tuple(pred.shape)}, {tuple(gt.shape)}")
    B, J = pred.shape[0], pred.shape[1]
    e, pa = torch.empty(B, device=pred.device), torch.empty(B, device=pred.device)
    al = torch.empty_like(pred) if want_aligned else None
    fn = load().egotap_pose_metrics_batch_axes if reference_batch_axes and B in (2, 3) else load().egotap_pose_metrics
    check(fn(_ptr(pred), _ptr(gt), B, J, _ptr(e), _ptr(pa), _ptr(al), _stream()))
    return (e, pa, al) if want_aligned else (e, pa)


def _check_u8_frames(who, whose, left8, right8, expected):
    """what every byte entry refuses alike, in this order: frames off the GPU, another dtype than uint8, a shape that is not the entry's
    (``expected()`` names the one it wants, or returns None), frames that are not contiguous or sit on two devices"""
    import torch
    for t in (left8, right8):
        if not (torch.is_tensor(t) and t.is_cuda):
            raise EgotapError(f"{who} runs on the GPU only (no CPU fallback); move the frames to cuda")
    for t in (left8, right8):
        if t.dtype != torch.uint8:
            raise EgotapError(f"{who} takes the {whose}'s bytes: dtype uint8, got {t.dtype} (normalised float frames go to the float entry)")
    want = expected()
    if want:
        raise ValueError(f"{who}: expected left8 / right8 {want}, got {tuple(left8.shape)} / {tuple(right8.shape)}")
    if not (left8.is_contiguous() and right8.is_contiguous()) or left8.device != right8.device:
        raise EgotapError(f"{who}: the frames must be contiguous and on one device (the bytes are read in place, nothing is copied)")


def check_camera_frames(who, left8, right8, S0):
    """the one wording of what the byte entries take: two uint8 [B, S0, S0, 3] contiguous tensors on one GPU; returns B"""
    def shape():
        B = left8.shape[0] if left8.dim() else 0
        if tuple(left8.shape) != (B, S0, S0, 3) or tuple(right8.shape) != (B, S0, S0, 3):
            return f"[B, {S0}, {S0}, 3] (HWC, RGB)"
    _check_u8_frames(who, "camera", left8, right8, shape)
    return left8.shape[0]


def rgb_u8_to_f32(left8, right8, table):
    """camera bytes uint8 [B, S0, S0, 3] x 2 -> the planar normalised frames fp32 [B, 3, S0, S0] x 2 (egotap_rgb_u8_to_f32): out[b, c, y, x] =
    table[c, in[b, y, x, c]]; `table` fp32 [3, 256] on the same device (spec.rgb_u8_table)"""
    import torch
    S0 = left8.shape[1] if left8.dim() == 4 else -1
    B = check_camera_frames("rgb_u8_to_f32", left8, right8, S0)
    _need_cuda_f32(table)
    if tuple(table.shape) != (3, 256) or table.device != left8.device:
        raise ValueError("rgb_u8_to_f32: the table is fp32 [3, 256] on the frames' device")
    left = torch.empty((B, 3, S0, S0), dtype=torch.float32, device=left8.device)
    right = torch.empty_like(left)
    with torch.cuda.device(left8.device):
        check(load().egotap_rgb_u8_to_f32(_ptr(left8), _ptr(right8), B, S0, _ptr(table), _ptr(left), _ptr(right), _stream(left8.device)))
    return left, right


def check_sensor_frames(who, left8, right8):
    """the one wording of what the sensor entries take: two uint8 [B, H, W, 3] contiguous tensors on one GPU, the same H and W for both eyes;
    returns (B, H, W)"""
    def shape():
        if left8.dim() != 4 or left8.shape[3] != 3 or left8.shape[1] < 1 or left8.shape[2] < 1 or tuple(right8.shape) != tuple(left8.shape):
            return "[B, H, W, 3] (HWC, RGB) with one H and W for both eyes"
    _check_u8_frames(who, "sensor", left8, right8, shape)
    return tuple(int(v) for v in left8.shape[:3])


def rgb_u8_resize(left8, right8, S0, rect_left=None, rect_right=None, mirror_left=False, mirror_right=False):
    """sensor frames uint8 [B, H, W, 3] x 2 -> camera bytes uint8 [B, S0, S0, 3] x 2 (egotap_rgb_u8_resize): per eye the source rectangle
    (x0, y0, w, h) (None: the full frame), mirrored or not, resampled bilinearly with align_corners=False in the integer arithmetic of
    spec.resize_u8 -- equal to it bit for bit.  One launch for both eyes."""
    import torch
    from . import spec as _spec
    B, H, W = check_sensor_frames("rgb_u8_resize", left8, right8)
    rl = (C.c_int * 4)(*_spec.check_resize_rect("rgb_u8_resize", rect_left, H, W))
    rr = (C.c_int * 4)(*_spec.check_resize_rect("rgb_u8_resize", rect_right, H, W))
    out_l = torch.empty((B, S0, S0, 3), dtype=torch.uint8, device=left8.device)
    out_r = torch.empty_like(out_l)
    if B == 0:
        return out_l, out_r
    with torch.cuda.device(left8.device):
        check(load().egotap_rgb_u8_resize(_ptr(left8), _ptr(right8), B, H, W, rl, rr, int(bool(mirror_left)), int(bool(mirror_right)), int(S0), _ptr(out_l),
                                          _ptr(out_r), _stream(left8.device)))
    return out_l, out_r


def yuv_source(layout, colour):
    """the egotap_yuv_source of a ``spec.YuvLayout`` and a ``spec.YuvColour``"""
    from . import spec as _spec
    return EgotapYuvSource(C.sizeof(EgotapYuvSource), _spec.YUV_FORMATS[layout.format], _spec.YUV_MATRICES[colour.matrix][0], _spec.YUV_RANGES[colour.range],
                           layout.H, layout.W, layout.pitch, layout.uv_offset, layout.frame_stride)


def check_yuv_frames(who, left8, right8, layout):
    """the one wording of what the YUV entries take: two contiguous uint8 tensors on one GPU, B frames of ``layout.frame_stride`` bytes each (any shape
    whose first axis is B), frame 0 at a multiple of the format's load width (2 bytes for nv12, 4 for yuyv); returns B"""
    fs = layout.frame_stride

    def shape():
        B = int(left8.shape[0]) if left8.dim() else -1
        if B < 0 or left8.numel() != B * fs or tuple(right8.shape) != tuple(left8.shape):
            return f"of one shape, B {layout.format} frames of frame_stride = {fs} bytes each ([B, {fs}])"
    _check_u8_frames(who, "sensor", left8, right8, shape)
    B, a = int(left8.shape[0]), layout.base_alignment
    if B > 0 and (left8.data_ptr() % a or right8.data_ptr() % a):
        raise EgotapError(f"{who}: {layout.format} frames must start at a multiple of {a} bytes (the widest load of the format)")
    return B


def yuv_u8_resize(left8, right8, layout, colour, S0, rect_left=None, rect_right=None, mirror_left=False, mirror_right=False):
    """NV12 / YUYV sensor frames (``check_yuv_frames``) x 2 -> camera bytes uint8 [B, S0, S0, 3] x 2 (egotap_yuv_u8_resize): per eye the source
    rectangle (x0, y0, w, h) in pixels (None: the full frame), mirrored or not, each tap converted to RGB bytes with ``colour`` and resampled
    bilinearly -- equal to spec.yuv_resize_u8 bit for bit.  One launch for both eyes."""
    import torch
    from . import spec as _spec
    B = check_yuv_frames("yuv_u8_resize", left8, right8, layout)
    rl = (C.c_int * 4)(*_spec.check_resize_rect("yuv_u8_resize", rect_left, layout.H, layout.W))
    rr = (C.c_int * 4)(*_spec.check_resize_rect("yuv_u8_resize", rect_right, layout.H, layout.W))
    out_l = torch.empty((B, S0, S0, 3), dtype=torch.uint8, device=left8.device)
    out_r = torch.empty_like(out_l)
    if B == 0:
        return out_l, out_r
    with torch.cuda.device(left8.device):
        check(load().egotap_yuv_u8_resize(_ptr(left8), _ptr(right8), B, C.byref(yuv_source(layout, colour)), rl, rr, int(bool(mirror_left)),
                                          int(bool(mirror_right)), int(S0), _ptr(out_l), _ptr(out_r), _stream(left8.device)))
    return out_l, out_r


class LensMaps:
    """A rig's two lens maps on the device (``lens_maps``): ``left`` / ``right`` the ``spec.LensMap`` of each eye, ``map_left`` / ``map_right`` their
    taps as int32 [S0 * S0, 2] device tensors (uploaded once, kept alive here), ``fill`` the (R, G, B) of an invalid pixel per eye.  With a rig per
    stream (``lens_maps`` of a list of pairs) ``S`` is the number of streams, ``streams`` the per-stream (left, right) ``spec.LensMap`` pairs,
    ``map_left`` / ``map_right`` int32 [S, S0 * S0, 2], and ``left`` / ``right`` stream 0's."""

    def __init__(self, left, right, map_left, map_right, fill, streams=None):
        self.left, self.right, self.map_left, self.map_right, self.fill = left, right, map_left, map_right, fill
        self.S0, self.H, self.W, self.model_size = left.S0, left.H, left.W, left.model_size
        self.mirrors = (int(left.mirror), int(right.mirror))
        self.streams = ((left, right),) if streams is None else tuple(streams)
        self.S = len(self.streams)

    @property
    def key(self):
        """what tells two uploads apart in a capture key: both map addresses and the fill"""
        return (self.map_left.data_ptr(), self.map_right.data_ptr(), self.fill)


def lens_maps(left, right=None, fill=(0, 0, 0), device=None):
    """``LensMaps`` of two ``spec.LensMap`` (left eye, right eye) on ``device`` (None: the current GPU): one upload per rig.  Both maps must share S0,
    the sensor frame's (H, W) and the model camera's calibration size -- one descriptor serves both eyes; the mirror flags may differ.  ``fill``: three
    bytes (R, G, B) for both eyes, or a pair of them (left, right).  A rig per stream: ``left`` a list of (left, right) pairs, stream 0 first, and
    ``right`` None -- every pair must share all of the above and each eye's mirror flag (the descriptor is one); the result has ``S`` = the number of
    pairs and frame b of a time-major batch is gathered through pair b % S (``lens_remap_streams``)."""
    import numpy as np
    import torch
    from . import spec as _spec
    streams = None
    if right is None:
        streams = [tuple(pair) if hasattr(pair, "__len__") else (pair,) for pair in (left if isinstance(left, (list, tuple)) else ())]
        if not 1 <= len(streams) <= _spec.STEREO_MAX_STREAMS or any(len(pair) != 2 for pair in streams):
            raise ValueError(f"lens_maps: without right, left is a list of 1 .. {_spec.STEREO_MAX_STREAMS} (left, right) pairs of spec.LensMap, one per stream")
        left, right = streams[0]
    for m in (left, right) if streams is None else tuple(m for pair in streams for m in pair):
        if not isinstance(m, _spec.LensMap):
            raise ValueError(f"lens_maps: left and right are spec.LensMap (spec.lens_map builds one per eye), got {type(m).__name__}")
    for s, (ml, mr) in enumerate(streams or ()):
        for m, first in ((ml, left), (mr, right)):
            if (m.S0, m.H, m.W, m.model_size, m.mirror) != (first.S0, first.H, first.W, first.model_size, first.mirror):
                raise ValueError(f"lens_maps: stream {s}'s maps differ from stream 0's in S0, frame size, model size or mirror flag (one descriptor serves all streams)")
    if left.S0 != right.S0:
        raise ValueError(f"lens_maps: both eyes' maps must have one output side, got S0 = {left.S0} / {right.S0}")
    if (left.H, left.W) != (right.H, right.W):
        raise ValueError(f"lens_maps: both eyes' maps must be built for one frame size, got {left.H} x {left.W} / {right.H} x {right.W}")
    if left.model_size != right.model_size:
        raise ValueError(f"lens_maps: both eyes' maps must share the model camera's calibration size, got {left.model_size} / {right.model_size}")
    if left.S0 % 4 or left.S0 > 4096:
        raise ValueError(f"lens_maps: the output side must be a multiple of 4, at most 4096, got S0 = {left.S0}")
    def triple(f):
        return hasattr(f, "__len__") and len(f) == 3 and all(isinstance(v, (int, np.integer)) and 0 <= v <= 255 for v in f)
    both = (fill, fill) if triple(fill) else fill
    if not (hasattr(both, "__len__") and len(both) == 2 and all(triple(f) for f in both)):
        raise ValueError(f"lens_maps: fill is three bytes (R, G, B), or one such triple per eye, got {fill}")
    fill = tuple(tuple(int(v) for v in f) for f in both)
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if dev.type != "cuda":
        raise EgotapError("lens_maps: the maps live on the GPU (no CPU fallback); pass a cuda device")
    if streams is None:
        up = [torch.from_numpy(np.array(m.taps).reshape(m.S0 * m.S0, 2)).to(dev) for m in (left, right)]
    else:
        up = [torch.from_numpy(np.stack([pair[e].taps.reshape(left.S0 * left.S0, 2) for pair in streams])).to(dev) for e in range(2)]
    if any(t.data_ptr() % 16 for t in up):
        raise EgotapError("lens_maps: a device map is not 16-byte aligned")
    return LensMaps(left, right, up[0], up[1], fill, streams)


def lens_source(maps, layout=None, colour=None):
    """the egotap_lens_source of a ``LensMaps`` and the frames' kind: ``layout`` None for uint8 [B, H, W, 3], or a ``spec.YuvLayout`` with its
    ``spec.YuvColour``"""
    d = EgotapLensSource()
    d.struct_size, d.H, d.W = C.sizeof(EgotapLensSource), maps.H, maps.W
    d.format = LENS_FORMATS["rgb8" if layout is None else layout.format]
    d.model_h, d.model_w = maps.model_size
    d.mirror[0], d.mirror[1] = maps.mirrors
    d.map_left, d.map_right = maps.map_left.data_ptr(), maps.map_right.data_ptr()
    for e in range(2):
        for c in range(3):
            d.fill[e][c] = maps.fill[e][c]
    if layout is not None:
        d.yuv = yuv_source(layout, colour)
    return d


def check_lens_frames(who, left8, right8, maps, layout=None, colour=None):
    """the one wording of what the lens entries take: a ``LensMaps`` on the frames' device, and frames of the size the maps were built for --
    ``check_sensor_frames``' (``layout`` None) or ``check_yuv_frames``' (a ``spec.YuvLayout`` with a ``spec.YuvColour``); returns B"""
    from . import spec as _spec
    if not isinstance(maps, LensMaps):
        raise ValueError(f"{who}: maps is what lens_maps returns (the rig's two uploaded spec.LensMap), got {type(maps).__name__}")
    if layout is None:
        B, H, W = check_sensor_frames(who, left8, right8)
    else:
        if not isinstance(layout, _spec.YuvLayout) or not isinstance(colour, _spec.YuvColour):
            raise ValueError(f"{who}: layout is a spec.YuvLayout (or None for uint8 [B, H, W, 3]) and colour a spec.YuvColour, got "
                             f"{type(layout).__name__} / {type(colour).__name__}")
        B, H, W = check_yuv_frames(who, left8, right8, layout), layout.H, layout.W
    if (H, W) != (maps.H, maps.W):
        raise ValueError(f"{who}: the maps were built for {maps.H} x {maps.W} frames, got {H} x {W} (spec.lens_map(..., frame_size=(H, W)))")
    if maps.map_left.device != left8.device:
        raise EgotapError(f"{who}: the maps are on {maps.map_left.device}, the frames on {left8.device}")
    return B


def lens_remap_streams(left8, right8, maps, S0, layout=None, colour=None):
    """``lens_remap`` with a rig per stream (egotap_lens_remap_streams): ``maps`` a ``LensMaps`` of S streams (``lens_maps`` of a list of pairs; S = 1
    too), frames time-major (frame b = t * S + s), frame b gathered through stream b % S's maps -- equal to spec.lens_remap_streams_u8 bit for bit, and
    on frames s, s + S, .. to ``lens_remap`` with stream s's maps.  B must be a multiple of S.  One launch for both eyes and all streams."""
    import torch
    from . import spec as _spec
    colour = _spec.YuvColour() if colour is None else colour
    B = check_lens_frames("lens_remap_streams", left8, right8, maps, layout, colour)
    if int(S0) != maps.S0:
        raise ValueError(f"lens_remap_streams: the maps were built for S0 = {maps.S0}, got S0 = {S0}")
    if B % maps.S:
        raise ValueError(f"lens_remap_streams: the batch must be a multiple of the number of streams (frame b uses map b % S), got B = {B}, S = {maps.S}")
    out_l = torch.empty((B, maps.S0, maps.S0, 3), dtype=torch.uint8, device=left8.device)
    out_r = torch.empty_like(out_l)
    if B == 0:
        return out_l, out_r
    with torch.cuda.device(left8.device):
        check(load().egotap_lens_remap_streams(_ptr(left8), _ptr(right8), B, C.byref(lens_source(maps, layout, colour)), maps.S, maps.S0, _ptr(out_l),
                                               _ptr(out_r), _stream(left8.device)))
    return out_l, out_r


def lens_remap(left8, right8, maps, S0, layout=None, colour=None):
    """frames from another lens x 2 -> camera bytes uint8 [B, S0, S0, 3] x 2 (egotap_lens_remap): each eye gathered bilinearly through its lens map
    (``lens_maps``), the fill bytes where the sensor does not see the model camera's pixel -- equal to spec.lens_remap_u8 bit for bit.  ``layout``
    None: uint8 [B, H, W, 3]; a ``spec.YuvLayout``: NV12 / YUYV frames (``check_yuv_frames``), each tap converted with ``colour`` (default bt601
    limited) first -- equal to spec.lens_remap_u8(spec.yuv_to_rgb_u8(frames, layout, colour), map).  One launch for both eyes."""
    import torch
    from . import spec as _spec
    colour = _spec.YuvColour() if colour is None else colour
    B = check_lens_frames("lens_remap", left8, right8, maps, layout, colour)
    if maps.S != 1:
        raise ValueError(f"lens_remap: the maps hold {maps.S} streams; lens_remap_streams gathers frame b through stream b % S's maps")
    if int(S0) != maps.S0:
        raise ValueError(f"lens_remap: the maps were built for S0 = {maps.S0}, got S0 = {S0}")
    out_l = torch.empty((B, maps.S0, maps.S0, 3), dtype=torch.uint8, device=left8.device)
    out_r = torch.empty_like(out_l)
    if B == 0:
        return out_l, out_r
    with torch.cuda.device(left8.device):
        check(load().egotap_lens_remap(_ptr(left8), _ptr(right8), B, C.byref(lens_source(maps, layout, colour)), maps.S0, _ptr(out_l), _ptr(out_r),
                                       _stream(left8.device)))
    return out_l, out_r


def heatmap_peaks(hm, c0: int = 0, n=None, groups: int = 1, affine=None):
    """2D joints and confidences of heatmaps (egotap_heatmap_peaks): hm [B, C, S, S], float32 or bfloat16 on the GPU -- estimator outputs or
    ground-truth maps, also a dim-1 slice of a larger contiguous tensor (read in place) -> float32 [B, n, 4], per map c0 .. c0 + n - 1 (None: all
    from c0 on) the record (x, y, score, index) of ``spec.heatmap_peaks_ref``, bit for bit.  ``affine``: [groups, 4] = (ax, bx, ay, by) for each
    group of n / groups consecutive maps (None: heatmap pixels, centres at i + 0.5).  One launch."""
    import torch
    if not (torch.is_tensor(hm) and hm.is_cuda):
        raise EgotapError("heatmap_peaks runs on the GPU only (no CPU fallback); move the maps to cuda")
    if hm.dtype not in (torch.float32, torch.bfloat16):
        raise EgotapError(f"heatmap_peaks takes float32 or bfloat16 maps, got {hm.dtype}")
    if hm.dim() != 4 or hm.shape[2] != hm.shape[3]:
        raise ValueError(f"heatmap_peaks: maps are [B, C, S, S], got {tuple(hm.shape)}")
    B, Cn, S, _ = (int(v) for v in hm.shape)
    n = Cn - c0 if n is None else int(n)
    if c0 < 0 or n < 1 or c0 + n > Cn:
        raise ValueError(f"heatmap_peaks: maps {c0} .. {c0 + n - 1} are not inside the {Cn} channels")
    # what the kernel addresses: element (b, c, y, x) at b * image_stride + c * S*S + y * S + x, an image stride of any size (a channel slice)
    if B > 0 and (hm.stride(3) != 1 or hm.stride(2) != S or hm.stride(1) != S * S or (B > 1 and hm.stride(0) < Cn * S * S)):
        raise EgotapError("heatmap_peaks: the maps must be contiguous per image (a dim-1 slice of a contiguous tensor is; nothing is copied)")
    aff = None
    if affine is not None:
        flat = [float(v) for row in affine for v in row]
        if len(flat) != 4 * groups:
            raise ValueError(f"heatmap_peaks: affine is [groups, 4] = (ax, bx, ay, by) per group, got {len(flat)} values for {groups} groups")
        aff = (C.c_float * len(flat))(*flat)
    out = torch.empty((B, n, 4), dtype=torch.float32, device=hm.device)
    if B == 0:
        return out
    with torch.cuda.device(hm.device):
        check(load().egotap_heatmap_peaks(_ptr(hm), F32 if hm.dtype == torch.float32 else BF16, B, S, hm.stride(0) if B > 1 else Cn * S * S, int(c0), n,
                                          int(groups), aff, _ptr(out), _stream(hm.device)))
    return out


def limb_decode(hm, c0: int, n_limbs: int, eyes: int = 2, affine=None):
    """Limb elevation angles and 2D segments of sin/cos limb heatmaps (egotap_limb_decode): hm [B, C, S, S], float32 or bfloat16 on the GPU --
    estimator outputs or ground-truth maps, also a dim-1 slice of a larger contiguous tensor (read in place) -> float32 [B, eyes, n_limbs, 8], per
    (cos, sin) pair the record (theta, coherence, x, y, phi, length, peak, mass) of ``spec.limb_decode_ref``.  For eye e and limb l the cos map is
    channel c0 + e * 2 n_limbs + l, the sin map channel c0 + e * 2 n_limbs + n_limbs + l.  ``affine``: [eyes, 4] = (ax, bx, ay, by) per eye
    (None: heatmap pixels, centres at i + 0.5).  One launch."""
    import torch
    if not torch.is_tensor(hm):
        raise EgotapError("limb_decode takes a torch tensor on the GPU")
    if hm.dtype not in (torch.float32, torch.bfloat16):
        raise EgotapError(f"limb_decode takes float32 or bfloat16 maps, got {hm.dtype}")
    if hm.dim() != 4 or hm.shape[2] != hm.shape[3]:
        raise ValueError(f"limb_decode: maps are [B, C, S, S], got {tuple(hm.shape)}")
    B, Cn, S, _ = (int(v) for v in hm.shape)
    c0, n_limbs, eyes = int(c0), int(n_limbs), int(eyes)
    if c0 < 0 or n_limbs < 1 or eyes < 1 or c0 + 2 * eyes * n_limbs > Cn:
        raise ValueError(f"limb_decode: channels {c0} .. {c0 + 2 * eyes * n_limbs - 1} (eyes x (cos, sin) x n_limbs) are not inside the {Cn} channels")
    if B > 0 and (hm.stride(3) != 1 or hm.stride(2) != S or hm.stride(1) != S * S or (B > 1 and hm.stride(0) < Cn * S * S)):
        raise EgotapError("limb_decode: the maps must be contiguous per image (a dim-1 slice of a contiguous tensor is; nothing is copied)")
    aff = None
    if affine is not None:
        flat = [float(v) for row in affine for v in row]
        if len(flat) != 4 * eyes:
            raise ValueError(f"limb_decode: affine is [eyes, 4] = (ax, bx, ay, by) per eye, got {len(flat)} values for {eyes} eyes")
        aff = (C.c_float * len(flat))(*flat)
    if not hm.is_cuda:                                   # (after the argument checks, so those can be exercised without a GPU)
        raise EgotapError("limb_decode runs on the GPU only (no CPU fallback); move the maps to cuda")
    out = torch.empty((B, eyes, n_limbs, 8), dtype=torch.float32, device=hm.device)
    if B == 0:
        return out
    with torch.cuda.device(hm.device):
        check(load().egotap_limb_decode(_ptr(hm), F32 if hm.dtype == torch.float32 else BF16, B, S, hm.stride(0) if B > 1 else Cn * S * S, c0, n_limbs, eyes,
                                        aff, _ptr(out), _stream(hm.device)))
    return out


def ocam_struct(model) -> EgotapOcam:
    """a ``spec.OcamModel`` as the ABI takes it (egotap_ocam, by pointer to host memory)"""
    o = EgotapOcam()
    for k, v in enumerate(model.pol):
        o.pol[k] = v
    for k, v in enumerate(model.invpol):
        o.invpol[k] = v
    o.xc, o.yc, o.c, o.d, o.e, o.ue_flip = model.xc, model.yc, model.c, model.d, model.e, 1.0 if model.ue_flip else 0.0
    o.n_pol, o.n_invpol = len(model.pol), len(model.invpol)
    return o


def _ocam_points(who, fn, pts, model, n_in, n_out):
    import torch
    if not torch.is_tensor(pts):
        raise EgotapError(f"{who} takes a torch tensor on the GPU")
    if pts.dim() < 1 or pts.shape[-1] != n_in:
        raise ValueError(f"{who}: points are [..., {n_in}], got {tuple(pts.shape)}")
    cam = ocam_struct(model)
    if not pts.is_cuda:                                  # (after the argument checks, so those can be exercised without a GPU)
        raise EgotapError(f"{who} runs on the GPU only (no CPU fallback); move the points to cuda")
    x = pts.detach().float().contiguous()
    out = torch.empty(tuple(x.shape[:-1]) + (n_out,), dtype=torch.float32, device=x.device)
    N = x.numel() // n_in
    if N == 0:
        return out
    with torch.cuda.device(x.device):
        check(fn(_ptr(x), N, C.byref(cam), _ptr(out), _stream(x.device)))
    return out


def ocam_project(points3d, model):
    """3D points [..., 3] in a camera's frame -> that camera's pixels [..., 2] through its fisheye model (egotap_ocam_project; the reference's
    world2cam, ``spec.ocam_world2cam_ref``): float32 in and out, float64 inside, one launch.  ``model``: a ``spec.OcamModel``.  The first step
    of ground-truth maps from 3D poses alone: ``synth_heatmaps(ocam_project(pts3d_left, left), ocam_project(pts3d_right, right), pose)``."""
    return _ocam_points("ocam_project", load().egotap_ocam_project, points3d, model, 3, 2)


def ocam_unproject(points2d, model):
    """pixels [..., 2] -> unit rays [..., 3] in the frame ``ocam_project`` takes its points in (egotap_ocam_unproject; the reference's cam2world
    as the inverse convention of world2cam, ``spec.ocam_cam2world_ref``): float32 in and out, float64 inside, one launch."""
    return _ocam_points("ocam_unproject", load().egotap_ocam_unproject, points2d, model, 2, 3)


def stereo_triangulate_args(left, right, t, R=None, affine=None, min_score=0.5):
    """the host-side arguments of egotap_stereo_triangulate as ctypes values, built once per rig: (left, right, R, t, affine, min_score)"""
    tt = [float(v) for v in t]
    if len(tt) != 3:
        raise ValueError(f"stereo_triangulate: t is the right camera's origin in the left frame, 3 values, got {len(tt)}")
    Rp = None
    if R is not None:
        rr = [float(v) for row in R for v in row]
        if len(rr) != 9:
            raise ValueError(f"stereo_triangulate: R is 3 x 3, got {len(rr)} values")
        Rp = (C.c_double * 9)(*rr)
    ap = None
    if affine is not None:
        aa = [float(v) for row in affine for v in row]
        if len(aa) != 8:
            raise ValueError(f"stereo_triangulate: affine is [2, 4] = (ax, bx, ay, by) per eye, got {len(aa)} values")
        ap = (C.c_double * 8)(*aa)
    return ocam_struct(left), ocam_struct(right), Rp, (C.c_double * 3)(*tt), ap, C.c_double(float(min_score))


def stereo_triangulate_into(args, keypoints, pose, pose_row0, joints3d, frame, dev):
    """the launch itself on ``dev``'s current stream: ``args`` from ``stereo_triangulate_args``, tensors as the ABI takes them"""
    cl, cr, Rp, tp, ap, ms = args
    B, _, J, _ = keypoints.shape
    check(load().egotap_stereo_triangulate(_ptr(keypoints), B, J, C.byref(cl), C.byref(cr), Rp, tp, ap, ms, _ptr(pose), pose.shape[1] if pose is not None else 0,
                                           int(pose_row0), _ptr(joints3d), _ptr(frame), _stream(dev)))


def stereo_triangulate(keypoints, left, right, t, R=None, affine=None, min_score=0.5, pose=None, pose_row0=0):
    """The stereo keypoints triangulated through the two cameras' fisheye models (egotap_stereo_triangulate, ``spec.stereo_triangulate_ref``):
    keypoints float32 [B, 2, J, 4] on the GPU, exactly what the serving entries return -> (joints3d float32 [B, J, 8] = (X, Y, Z, gap, den, s,
    disagree, valid), frame float32 [B, 8] = (t_hat xyz, n, rms / max disagree, rms / max gap)) in the left camera's frame.  ``left`` / ``right``:
    ``spec.OcamModel``; ``t`` (3) and ``R`` (3 x 3, None: identity): the right camera's origin and axes in the left frame, in the pose's units;
    ``affine``: [2, 4] = (ax, bx, ay, by) per eye from keypoint units to the calibration's pixels (None: identity); ``pose``: the lifted pose
    float32 [B, P, 3] whose rows pose_row0 .. pose_row0 + J - 1 pair with the joints (None: no translation, no disagreement).  One launch."""
    import torch
    args = stereo_triangulate_args(left, right, t, R, affine, min_score)
    if not torch.is_tensor(keypoints) or keypoints.dim() != 4 or keypoints.shape[1] != 2 or keypoints.shape[3] != 4:
        raise ValueError(f"stereo_triangulate: keypoints are a tensor [B, 2, J, 4], got {tuple(getattr(keypoints, 'shape', ()))}")
    B, _, J, _ = (int(v) for v in keypoints.shape)
    if not 1 <= J <= 64:
        raise ValueError(f"stereo_triangulate: 1 .. 64 joints, got {J}")
    if pose is not None and (not torch.is_tensor(pose) or pose.dim() != 3 or pose.shape[0] != B or pose.shape[2] != 3 or pose_row0 < 0
                             or pose_row0 + J > pose.shape[1]):
        raise ValueError(f"stereo_triangulate: pose is a tensor [B, P, 3] with pose_row0 + J <= P, got {tuple(getattr(pose, 'shape', ()))}, "
                         f"pose_row0 = {pose_row0}, J = {J}")
    if not keypoints.is_cuda or (pose is not None and pose.device != keypoints.device):
        raise EgotapError("stereo_triangulate runs on the GPU only (no CPU fallback); keypoints and pose on one cuda device")
    kp = keypoints.detach().float().contiguous()
    ps = pose.detach().float().contiguous() if pose is not None else None
    joints3d = torch.empty((B, J, 8), dtype=torch.float32, device=kp.device)
    frame = torch.empty((B, 8), dtype=torch.float32, device=kp.device)
    if B == 0:
        return joints3d, frame
    with torch.cuda.device(kp.device):
        stereo_triangulate_into(args, kp, ps, pose_row0, joints3d, frame, kp.device)
    return joints3d, frame


def fuse_params_struct(params) -> EgotapFuseParams:
    """a ``spec.FuseParams`` as the ABI takes it (egotap_fuse_params, by pointer to host memory); there is no default: sigma_prior carries a unit"""
    from . import spec
    if not isinstance(params, spec.FuseParams):
        raise ValueError(f"stereo_fuse: params is a spec.FuseParams(sigma_prior=...) -- sigma_prior has no default -- got {type(params).__name__}")
    o = EgotapFuseParams()
    o.sigma_ray, o.sigma_prior, o.max_sigma, o.min_joints = params.sigma_ray, params.sigma_prior, params.max_sigma, params.min_joints
    return o


def stereo_fuse_into(args, prm, keypoints, pose, pose_row0, frame, fused, pose_fused, stats, dev):
    """the launch itself on ``dev``'s current stream: ``args`` from ``stereo_triangulate_args``, ``prm`` from ``fuse_params_struct``, tensors as the ABI
    takes them (pose_fused may be pose)"""
    cl, cr, Rp, tp, ap, ms = args
    B, _, J, _ = keypoints.shape
    check(load().egotap_stereo_fuse(_ptr(keypoints), B, J, C.byref(cl), C.byref(cr), Rp, tp, ap, ms, _ptr(pose), pose.shape[1], int(pose_row0), _ptr(frame),
                                    C.byref(prm), _ptr(fused), _ptr(pose_fused), _ptr(stats), _stream(dev)))


def _stereo_fuse_shapes(who, keypoints, pose, frame, pose_row0):
    """the shape checks of ``stereo_fuse`` and ``StereoFusion.update`` under the face's name -> (B, J, P)"""
    import torch
    if not torch.is_tensor(keypoints) or keypoints.dim() != 4 or keypoints.shape[1] != 2 or keypoints.shape[3] != 4:
        raise ValueError(f"{who}: keypoints are a tensor [B, 2, J, 4], got {tuple(getattr(keypoints, 'shape', ()))}")
    B, _, J, _ = (int(v) for v in keypoints.shape)
    if not 1 <= J <= 64:
        raise ValueError(f"{who}: 1 .. 64 joints, got {J}")
    if not torch.is_tensor(pose) or pose.dim() != 3 or pose.shape[0] != B or pose.shape[2] != 3 or pose_row0 < 0 or pose_row0 + J > pose.shape[1]:
        raise ValueError(f"{who}: pose is a tensor [B, P, 3] with pose_row0 + J <= P, got {tuple(getattr(pose, 'shape', ()))}, pose_row0 = {pose_row0}, J = {J}")
    if not torch.is_tensor(frame) or tuple(frame.shape) != (B, 8):
        raise ValueError(f"{who}: frame is a tensor [B, 8] = {(B, 8)}, the triangulation's frame record, got {tuple(getattr(frame, 'shape', ()))}")
    return B, J, int(pose.shape[1])


def _stereo_fuse_run(who, args, prm, keypoints, pose, frame, pose_row0):
    import torch
    B, J, P = _stereo_fuse_shapes(who, keypoints, pose, frame, pose_row0)
    if not _on_one_gpu(keypoints, pose, frame):
        raise EgotapError(f"{who} runs on the GPU only (no CPU fallback); keypoints, pose and frame on one cuda device")
    kp, ps, fr = _f32c(keypoints), _f32c(pose), _f32c(frame)
    pose_fused = torch.empty((B, P, 3), dtype=torch.float32, device=kp.device)
    fused = torch.empty((B, J, 8), dtype=torch.float32, device=kp.device)
    stats = torch.empty((B, 8), dtype=torch.float32, device=kp.device)
    if B == 0:
        return pose_fused, fused, stats
    with torch.cuda.device(kp.device):
        stereo_fuse_into(args, prm, kp, ps, pose_row0, fr, fused, pose_fused, stats, kp.device)
    return pose_fused, fused, stats


def stereo_fuse(keypoints, pose, frame, left, right, t, params, R=None, affine=None, min_score=0.5, pose_row0=0):
    """The lifted joints fused with the keypoint rays of whichever eyes see them (egotap_stereo_fuse, ``spec.stereo_fuse_ref``): keypoints float32
    [B, 2, J, 4], pose float32 [B, P, 3] and frame float32 [B, 8] on the GPU -- what a ``return_keypoints=True, return_triangulation=True`` serving call
    returns -> (pose_fused float32 [B, P, 3], fused float32 [B, J, 8] = (x, y, z, move, res left, res right, share, mode), stats float32 [B, 8]).
    pose_fused goes into ``pose_track`` / ``PoseTracker.update`` in place of pose.  The rig arguments are ``stereo_triangulate``'s; ``params`` a
    ``spec.FuseParams(sigma_prior=...)``: sigma_prior is in the pose's units and has no default.  One launch."""
    args = stereo_triangulate_args(left, right, t, R, affine, min_score)
    prm = fuse_params_struct(params)
    return _stereo_fuse_run("stereo_fuse", args, prm, keypoints, pose, frame, pose_row0)


# ---- a camera rig per stream: the rig table and the two operators that read it
STEREO_RIG_BYTES = C.sizeof(EgotapStereoRig)          # 792


def stereo_rig_struct(rig) -> EgotapStereoRig:
    """a ``spec.StereoRig`` as one row of a rig table (egotap_stereo_rig): every value spelled out, the identity where R or affine is None"""
    from . import spec as _spec
    if not isinstance(rig, _spec.StereoRig):
        raise ValueError(f"stereo rig table: a rig is a spec.StereoRig, got {type(rig).__name__}")
    o = EgotapStereoRig()
    o.left, o.right = ocam_struct(rig.left), ocam_struct(rig.right)
    R = rig.R if rig.R is not None else ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0))
    aff = rig.affine if rig.affine is not None else _spec.STEREO_IDENTITY_AFFINE
    for k in range(9):
        o.R[k] = R[k // 3][k % 3]
    for k in range(3):
        o.t[k] = rig.t[k]
    for e in range(2):
        for k in range(4):
            o.affine[e][k] = aff[e][k]
    o.min_score = rig.min_score
    return o


def stereo_rigs_host(rigs):
    """a list of ``spec.StereoRig`` as a checked host table (egotap_stereo_rigs_check: every refusal names the field and the stream): a ctypes array of
    S egotap_stereo_rig.  Needs no GPU."""
    rigs = list(rigs)
    host = (EgotapStereoRig * max(1, len(rigs)))(*[stereo_rig_struct(r) for r in rigs])
    check(load().egotap_stereo_rigs_check(host, len(rigs)))
    return host


def stereo_rigs_table(rigs, device=None):
    """The rig table of S streams on ``device`` (None: the current GPU): (table, host) -- ``table`` a uint8 device tensor of S * 792 bytes, uploaded
    once, that ``stereo_triangulate_streams`` / ``stereo_fuse_streams`` read rig b % S of for frame b; ``host`` the checked ctypes array it was
    uploaded from.  The library cannot inspect device memory: write the tensor through ``stereo_rig_write`` only."""
    import torch
    host = stereo_rigs_host(rigs)
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if dev.type != "cuda":
        raise EgotapError("stereo_rigs_table: the table lives on the GPU (no CPU fallback); pass a cuda device")
    table = torch.frombuffer(bytearray(bytes(host)), dtype=torch.uint8).to(dev)
    if table.data_ptr() % 8:
        raise EgotapError("stereo_rigs_table: the device table is not 8-byte aligned")
    return table, host


def stereo_rig_check(rig, s):
    """one ``spec.StereoRig`` checked as stream ``s``'s (egotap_stereo_rigs_check; the refusal names the field and stream s) -> a ctypes array of one row"""
    one = (EgotapStereoRig * 1)(stereo_rig_struct(rig))
    try:
        check(load().egotap_stereo_rigs_check(one, 1))
    except EgotapError as e:
        raise EgotapError(str(e).replace("rig 0:", f"rig {int(s)}:")) from None
    return one


def stereo_rig_write(table, host, s, rig):
    """Row ``s`` of a rig table rewritten in place with ``rig`` (a ``spec.StereoRig``), checked first; the copy is ordered on the table's device's
    current stream, so launches and graph replays enqueued after it read the new rig and those before it the old one."""
    import torch
    S = len(host)
    if not 0 <= int(s) < S:
        raise ValueError(f"stereo_rig_write: stream {s} is not one of the table's {S}")
    one = stereo_rig_check(rig, s)
    host[int(s)] = one[0]
    with torch.cuda.device(table.device):
        table[int(s) * STEREO_RIG_BYTES:(int(s) + 1) * STEREO_RIG_BYTES].copy_(torch.frombuffer(bytearray(bytes(one)), dtype=torch.uint8))


def _check_rig_table(who, table, S, B, dev):
    import torch
    if not (torch.is_tensor(table) and table.dtype == torch.uint8 and table.dim() == 1 and table.is_contiguous()) or int(S) < 1 or \
            table.numel() != int(S) * STEREO_RIG_BYTES:
        raise ValueError(f"{who}: the rig table is what stereo_rigs_table returns, uint8 [S * {STEREO_RIG_BYTES}] with S >= 1, got "
                         f"{tuple(getattr(table, 'shape', ()))} for S = {S}")
    if B % int(S):
        raise ValueError(f"{who}: the batch must be a multiple of the number of streams (frame b uses rig b % S), got B = {B}, S = {S}")
    if dev is not None and table.device != dev:
        raise EgotapError(f"{who}: the rig table is on {table.device}, the keypoints on {dev}")


def stereo_triangulate_streams_into(table, S, keypoints, pose, pose_row0, joints3d, frame, dev):
    """the launch itself on ``dev``'s current stream: tensors as the ABI takes them"""
    B, _, J, _ = keypoints.shape
    check(load().egotap_stereo_triangulate_streams(_ptr(keypoints), B, J, _ptr(table), int(S), _ptr(pose), pose.shape[1] if pose is not None else 0, int(pose_row0),
                                                   _ptr(joints3d), _ptr(frame), _stream(dev)))


def stereo_triangulate_streams(keypoints, table, S, pose=None, pose_row0=0):
    """``stereo_triangulate`` with a rig per stream (egotap_stereo_triangulate_streams, ``spec.stereo_triangulate_streams_ref``): keypoints float32
    [B, 2, J, 4] of T frames of S streams, time-major (frame b = t * S + s); ``table`` the device table of ``stereo_rigs_table``; frame b is
    triangulated through rig b % S.  Rows s, s + S, .. equal ``stereo_triangulate`` on those rows with rig s in every bit.  One launch."""
    import torch
    who = "stereo_triangulate_streams"
    if not torch.is_tensor(keypoints) or keypoints.dim() != 4 or keypoints.shape[1] != 2 or keypoints.shape[3] != 4:
        raise ValueError(f"{who}: keypoints are a tensor [B, 2, J, 4], got {tuple(getattr(keypoints, 'shape', ()))}")
    B, _, J, _ = (int(v) for v in keypoints.shape)
    if not 1 <= J <= 64:
        raise ValueError(f"{who}: 1 .. 64 joints, got {J}")
    if pose is not None and (not torch.is_tensor(pose) or pose.dim() != 3 or pose.shape[0] != B or pose.shape[2] != 3 or pose_row0 < 0
                             or pose_row0 + J > pose.shape[1]):
        raise ValueError(f"{who}: pose is a tensor [B, P, 3] with pose_row0 + J <= P, got {tuple(getattr(pose, 'shape', ()))}, "
                         f"pose_row0 = {pose_row0}, J = {J}")
    _check_rig_table(who, table, S, B, None)
    if not keypoints.is_cuda or (pose is not None and pose.device != keypoints.device) or table.device != keypoints.device:
        raise EgotapError(f"{who} runs on the GPU only (no CPU fallback); keypoints, pose and the rig table on one cuda device")
    kp = keypoints.detach().float().contiguous()
    ps = pose.detach().float().contiguous() if pose is not None else None
    joints3d = torch.empty((B, J, 8), dtype=torch.float32, device=kp.device)
    frame = torch.empty((B, 8), dtype=torch.float32, device=kp.device)
    if B == 0:
        return joints3d, frame
    with torch.cuda.device(kp.device):
        stereo_triangulate_streams_into(table, S, kp, ps, pose_row0, joints3d, frame, kp.device)
    return joints3d, frame


def stereo_fuse_streams_into(table, S, prm, keypoints, pose, pose_row0, frame, fused, pose_fused, stats, dev):
    """the launch itself on ``dev``'s current stream: ``prm`` from ``fuse_params_struct``, tensors as the ABI takes them (pose_fused may be pose)"""
    B, _, J, _ = keypoints.shape
    check(load().egotap_stereo_fuse_streams(_ptr(keypoints), B, J, _ptr(table), int(S), _ptr(pose), pose.shape[1], int(pose_row0), _ptr(frame), C.byref(prm),
                                            _ptr(fused), _ptr(pose_fused), _ptr(stats), _stream(dev)))


def _stereo_fuse_streams_run(who, table, S, prm, keypoints, pose, frame, pose_row0):
    import torch
    B, J, P = _stereo_fuse_shapes(who, keypoints, pose, frame, pose_row0)
    _check_rig_table(who, table, S, B, None)
    if not _on_one_gpu(keypoints, pose, frame, table):
        raise EgotapError(f"{who} runs on the GPU only (no CPU fallback); keypoints, pose, frame and the rig table on one cuda device")
    kp, ps, fr = _f32c(keypoints), _f32c(pose), _f32c(frame)
    pose_fused = torch.empty((B, P, 3), dtype=torch.float32, device=kp.device)
    fused = torch.empty((B, J, 8), dtype=torch.float32, device=kp.device)
    stats = torch.empty((B, 8), dtype=torch.float32, device=kp.device)
    if B == 0:
        return pose_fused, fused, stats
    with torch.cuda.device(kp.device):
        stereo_fuse_streams_into(table, S, prm, kp, ps, pose_row0, fr, fused, pose_fused, stats, kp.device)
    return pose_fused, fused, stats


def stereo_fuse_streams(keypoints, pose, frame, table, S, params, pose_row0=0):
    """``stereo_fuse`` with a rig per stream (egotap_stereo_fuse_streams, ``spec.stereo_fuse_streams_ref``): the tensors are ``stereo_fuse``'s for T
    frames of S streams, time-major; ``table`` the device table of ``stereo_rigs_table``; one ``params`` (``spec.FuseParams``) serves all streams.
    Rows s, s + S, .. equal ``stereo_fuse`` on those rows with rig s in every bit.  One launch."""
    return _stereo_fuse_streams_run("stereo_fuse_streams", table, S, fuse_params_struct(params), keypoints, pose, frame, pose_row0)


def track_params_struct(params=None) -> EgotapTrackParams:
    """a ``spec.TrackParams`` (None: the defaults) as the ABI takes it (egotap_track_params, by pointer to host memory)"""
    from . import spec
    prm = spec.TrackParams() if params is None else params
    o = EgotapTrackParams()
    for c in spec.TRACK_CLASSES:
        for n, v in zip(("min_cutoff", "beta", "d_cutoff"), getattr(prm, c)):
            setattr(o, f"{c}_{n}", v)
    o.max_disagree, o.max_gap, o.max_joint_gap, o.min_joints, o.max_hold = prm.max_disagree, prm.max_gap, prm.max_joint_gap, prm.min_joints, prm.max_hold
    return o


def pose_track_into(prm, pose, frame, joints3d, T, S, dts, dt, state_in, state_out, tracks, placed, dev):
    """the launch itself on ``dev``'s current stream: ``prm`` from ``track_params_struct``, tensors as the ABI takes them (frame, joints3d, dts may be
    None; dt is read only without dts)"""
    check(load().egotap_pose_track(_ptr(pose), _ptr(frame), _ptr(joints3d), int(T), int(S), pose.shape[1], joints3d.shape[1] if joints3d is not None else 0,
                                   _ptr(dts), C.c_double(0.0 if dt is None else float(dt)), C.byref(prm), _ptr(state_in), _ptr(state_out), _ptr(tracks),
                                   _ptr(placed), _stream(dev)))


def _pose_track_args(who, pose, state, dt, dts, params, frame, joints3d, streams):
    """the shape, dtype and value checks ``pose_track`` and ``pose_track_world`` make alike, under the face's name -> (prm, T, S, P, J); each face
    then checks what is its own and, last, the devices"""
    import torch
    prm = track_params_struct(params)
    S = int(streams)
    if not torch.is_tensor(pose) or pose.dim() != 3 or pose.shape[2] != 3 or S < 1 or pose.shape[0] < S or pose.shape[0] % S:
        raise ValueError(f"{who}: pose is a tensor [T * streams, P, 3] with T >= 1, got {tuple(getattr(pose, 'shape', ()))} for {streams} streams")
    B, P, _ = (int(v) for v in pose.shape)
    T = B // S
    if not 1 <= P <= 64:
        raise ValueError(f"{who}: 1 .. 64 pose rows, got {P}")
    J = 0
    if joints3d is not None:
        if not torch.is_tensor(joints3d) or joints3d.dim() != 3 or joints3d.shape[0] != B or joints3d.shape[2] != 8 or not 1 <= joints3d.shape[1] <= 64:
            raise ValueError(f"{who}: joints3d is a tensor [T * streams, J, 8] with 1 .. 64 joints, got {tuple(getattr(joints3d, 'shape', ()))} for {B} frames")
        J = int(joints3d.shape[1])
    if frame is not None and (not torch.is_tensor(frame) or tuple(frame.shape) != (B, 8)):
        raise ValueError(f"{who}: frame is a tensor [T * streams, 8], got {tuple(getattr(frame, 'shape', ()))} for {B} frames")
    K = P + 1 + J
    if not torch.is_tensor(state) or tuple(state.shape) != (S, K, 12) or state.dtype != torch.float64 or not state.is_contiguous():
        raise ValueError(f"{who}: state is a contiguous float64 tensor [streams, P + 1 + J, 12] = {(S, K, 12)}, got "
                         f"{getattr(state, 'dtype', type(state).__name__)} {tuple(getattr(state, 'shape', ()))}")
    if (dt is None) == (dts is None):
        raise ValueError(f"{who}: give exactly one of dt (seconds per step) and dts (a float32 tensor [T] on the device)")
    if dts is not None and (not torch.is_tensor(dts) or tuple(dts.shape) != (T,) or dts.dtype != torch.float32):
        raise ValueError(f"{who}: dts is a float32 tensor [T] = [{T}], got {getattr(dts, 'dtype', type(dts).__name__)} {tuple(getattr(dts, 'shape', ()))}")
    if dt is not None and not (float(dt) > 0 and float(dt) != float("inf")):
        raise ValueError(f"{who}: dt must be finite and > 0, got {dt}")
    return prm, T, S, P, J


def heat_u8(hm, c0: int = 0, n=None, groups: int = 1):
    """The reference's picture of a heatmap stack per group of channels (egotap_heat_u8, ``spec.heat_u8``, bit for bit): hm [B, C, S, S], float32 or
    bfloat16 on the GPU, also a dim-1 slice of a larger contiguous tensor (read in place) -> uint8 [B, groups, S, S]: channels c0 .. c0 + n - 1
    (None: all from c0 on) in ``groups`` groups of consecutive channels, each added up, clamped to [0, 1] and scaled to a byte.  One launch."""
    import torch
    if not torch.is_tensor(hm):
        raise EgotapError("heat_u8 takes a torch tensor on the GPU")
    if hm.dtype not in (torch.float32, torch.bfloat16):
        raise EgotapError(f"heat_u8 takes float32 or bfloat16 maps, got {hm.dtype}")
    if hm.dim() != 4 or hm.shape[2] != hm.shape[3]:
        raise ValueError(f"heat_u8: maps are [B, C, S, S], got {tuple(hm.shape)}")
    B, Cn, S, _ = (int(v) for v in hm.shape)
    c0, groups = int(c0), int(groups)
    n = Cn - c0 if n is None else int(n)
    if c0 < 0 or n < 1 or c0 + n > Cn or groups < 1 or n % groups:
        raise ValueError(f"heat_u8: channels {c0} .. {c0 + n - 1} in {groups} groups are not a slice of the {Cn} channels in equal groups")
    if B > 0 and (hm.stride(3) != 1 or hm.stride(2) != S or hm.stride(1) != S * S or (B > 1 and hm.stride(0) < Cn * S * S)):
        raise EgotapError("heat_u8: the maps must be contiguous per image (a dim-1 slice of a contiguous tensor is; nothing is copied)")
    if not hm.is_cuda:                                   # (after the argument checks, so those can be exercised without a GPU)
        raise EgotapError("heat_u8 runs on the GPU only (no CPU fallback); move the maps to cuda")
    out = torch.empty((B, groups, S, S), dtype=torch.uint8, device=hm.device)
    if B == 0:
        return out
    with torch.cuda.device(hm.device):
        check(load().egotap_heat_u8(_ptr(hm), F32 if hm.dtype == torch.float32 else BF16, B, Cn, S, hm.stride(0) if B > 1 else Cn * S * S, c0, n, groups,
                                    _ptr(out), _stream(hm.device)))
    return out


def overlay_style_struct(style) -> EgotapOverlayStyle:
    """a ``spec.OverlayStyle`` as the ABI takes it (egotap_overlay_style, by pointer to host memory)"""
    from . import spec
    if not isinstance(style, spec.OverlayStyle):
        raise ValueError(f"overlay_u8: style is a spec.OverlayStyle (spec.overlay_style(joint_preset) makes a preset's), got {type(style).__name__}")
    o = EgotapOverlayStyle()
    o.n_marks, o.n_bones, o.r16, o.w16, o.min_score = len(style.mark_rgba), len(style.bones), style.r16, style.w16, style.min_score
    o.heat_rgba[:] = style.heat_rgba
    for l, (i, j) in enumerate(style.bones):
        o.bones[l][:] = (i, j)
        o.bone_rgba[l][:] = style.bone_rgba[l]
    for j, c in enumerate(style.mark_rgba):
        o.mark_rgba[j][:] = c
    return o


def overlay_tap_tables(affine, S: int, Hc: int, Wc: int, device):
    """the heat layer's tap tables of one eye on ``device``: (tx int32 [Wc], ty int32 [Hc]) from the eye's keypoint affine (ax, bx, ay, by)
    (``spec.overlay_taps``, built on the host in float64)"""
    import torch
    from . import spec
    ax, bx, ay, by = (float(v) for v in affine)
    return (torch.from_numpy(spec.overlay_taps(ax, bx, S, Wc)).to(device), torch.from_numpy(spec.overlay_taps(ay, by, S, Hc)).to(device))


def overlay_u8(left8, right8, style, marks=None, heat8=None, taps=None, out=None):
    """Three layers blended onto packed RGB8 canvases (egotap_overlay_u8, ``spec.overlay_u8``, equal in every byte): left8 / right8 uint8
    [B, Hc, Wc, 3] on the GPU (``right8`` None: one eye, E = 1; else E = 2), Wc a multiple of 4 -> (out_left, out_right or None).  ``style`` a
    ``spec.OverlayStyle``; ``marks`` float32 [B, E, M, 4] = (x, y, score, _) in canvas pixels with M the style's number of marks (None: neither marks nor
    bones); ``heat8`` uint8 [B, E, S, S] (``heat_u8`` with groups = E) with ``taps`` = per eye (tx, ty) from ``overlay_tap_tables`` (None: no heat);
    ``out`` = (out_left, out_right) to write into -- the inputs themselves draw in place -- or None for new tensors.  One launch."""
    import torch
    who = "overlay_u8"
    prm = overlay_style_struct(style)
    eyes = [left8] if right8 is None else [left8, right8]
    E = len(eyes)
    for t in eyes:
        if not torch.is_tensor(t) or t.dtype != torch.uint8 or t.dim() != 4 or t.shape[3] != 3 or t.shape != left8.shape:
            raise ValueError(f"{who}: canvases are uint8 tensors [B, Hc, Wc, 3] of one shape, got {[tuple(getattr(e, 'shape', ())) for e in eyes]}")
    B, Hc, Wc, _ = (int(v) for v in left8.shape)
    if Wc % 4 or Wc < 4 or Hc < 1 or Hc > 16384 or Wc > 16384:
        raise ValueError(f"{who}: a canvas is 1 .. 16384 rows of 4 .. 16384 pixels, the width a multiple of 4, got {Hc} x {Wc}")
    M = len(style.mark_rgba)
    if marks is None:
        if M or style.bones:
            raise ValueError(f"{who}: the style has {M} marks and {len(style.bones)} bones and no marks are given")
    elif not torch.is_tensor(marks) or tuple(marks.shape) != (B, E, M, 4):
        raise ValueError(f"{who}: marks are a tensor [B, E, M, 4] = {(B, E, M, 4)} with M the style's marks, got {tuple(getattr(marks, 'shape', ()))}")
    S = 0
    if heat8 is not None:
        if not torch.is_tensor(heat8) or heat8.dtype != torch.uint8 or heat8.dim() != 4 or tuple(heat8.shape[:2]) != (B, E) or heat8.shape[2] != heat8.shape[3]:
            raise ValueError(f"{who}: heat8 is a uint8 tensor [B, E, S, S] with (B, E) = {(B, E)}, got {tuple(getattr(heat8, 'shape', ()))}")
        S = int(heat8.shape[2])
        if taps is None or len(taps) != E or any(tuple(tx.shape) != (Wc,) or tuple(ty.shape) != (Hc,) or tx.dtype != torch.int32 or ty.dtype != torch.int32
                                                 for tx, ty in taps):
            raise ValueError(f"{who}: with heat8, taps are per eye (tx int32 [{Wc}], ty int32 [{Hc}]) from overlay_tap_tables")
    if out is not None:
        out = list(out) + [None] * (2 - len(out))
        if any(not torch.is_tensor(o) or o.dtype != torch.uint8 or o.shape != left8.shape for o in out[:E]) or (E == 1 and out[1] is not None):
            raise ValueError(f"{who}: out is (out_left, out_right) of the canvases' dtype and shape, out_right None for one eye")
    tensors = eyes + [t for t in (marks, heat8) if t is not None] + [t for pair in (taps if heat8 is not None else ()) for t in pair] + (out[:E] if out else [])
    if not all(t.is_cuda and t.device == left8.device for t in tensors):
        raise EgotapError(f"{who} runs on the GPU only (no CPU fallback); every tensor on one cuda device")
    if not all(t.is_contiguous() for t in tensors if t is not marks):
        raise EgotapError(f"{who}: the canvases, heat8, the tap tables and out must be contiguous (the bytes are read and written in place)")
    mk = _f32c(marks)
    if out is None:
        out = [torch.empty_like(t) for t in eyes] + [None] * (2 - E)
    if B == 0:
        return out[0], out[1]
    tl = taps[0] if heat8 is not None else (None, None)
    tr = taps[1] if heat8 is not None and E == 2 else (None, None)
    with torch.cuda.device(left8.device):
        check(load().egotap_overlay_u8(_ptr(left8), _ptr(right8), B, Hc, Wc, _ptr(heat8), S, _ptr(tl[0]), _ptr(tl[1]), _ptr(tr[0]), _ptr(tr[1]), _ptr(mk),
                                       C.byref(prm), _ptr(out[0]), _ptr(out[1]), _stream(left8.device)))
    return out[0], out[1]


def _on_one_gpu(pose, *others):
    return pose.is_cuda and all(t is None or t.device == pose.device for t in others)


def _f32c(t):
    """a float tensor as the ABI reads it (None stays None)"""
    return t.detach().float().contiguous() if t is not None else None


def pose_track(pose, state, dt=None, dts=None, params=None, frame=None, joints3d=None, streams=1):
    """The pose, the root and the stereo joints filtered over time (egotap_pose_track, ``spec.pose_track_ref``): a One-Euro filter per 3-vector whose
    state survives between calls.  pose float32 [T * streams, P, 3] on the GPU, T consecutive frames of ``streams`` camera rigs, time-major;
    ``frame`` float32 [T * streams, 8] and ``joints3d`` float32 [T * streams, J, 8]: the last two results of a ``return_triangulation=True`` serving
    call (None: the root / the joints are not tracked); ``state`` float64 [streams, P + 1 + J, 12] on the same device, all zeros for "never seen",
    UPDATED IN PLACE; ``dt`` a positive number of seconds per step, or ``dts`` float32 [T] on the device (exactly one of the two); ``params`` a
    ``spec.TrackParams`` (None: its defaults) -> (tracks float32 [T * streams, P + 1 + J, 8] = (x^, v^, cutoff, status), placed float32
    [T * streams, P, 3] = the filtered pose plus the filtered root).  One launch on the current stream, no synchronisation."""
    import torch
    prm, T, S, P, J = _pose_track_args("pose_track", pose, state, dt, dts, params, frame, joints3d, streams)
    if not _on_one_gpu(pose, frame, joints3d, dts, state):
        raise EgotapError("pose_track runs on the GPU only (no CPU fallback); pose, frame, joints3d, dts and state on one cuda device")
    ps, fr, j3 = _f32c(pose), _f32c(frame), _f32c(joints3d)
    B, K = T * S, P + 1 + J
    tracks = torch.empty((B, K, 8), dtype=torch.float32, device=ps.device)
    placed = torch.empty((B, P, 3), dtype=torch.float32, device=ps.device)
    with torch.cuda.device(ps.device):
        pose_track_into(prm, ps, fr, j3, T, S, dts.contiguous() if dts is not None else None, dt, state, state, tracks, placed, ps.device)
    return tracks, placed


def pose_track_world_into(prm, pose, frame, joints3d, rig_pose, T, S, dts, dt, ortho_tol, state_in, state_out, tracks, placed_world, placed_cam, dev):
    """the launch itself on ``dev``'s current stream, as ``pose_track_into``; rig_pose float64 [T * S, 12]"""
    check(load().egotap_pose_track_world(_ptr(pose), _ptr(frame), _ptr(joints3d), _ptr(rig_pose), int(T), int(S), pose.shape[1],
                                         joints3d.shape[1] if joints3d is not None else 0, _ptr(dts), C.c_double(0.0 if dt is None else float(dt)), C.byref(prm),
                                         C.c_double(float(ortho_tol)), _ptr(state_in), _ptr(state_out), _ptr(tracks), _ptr(placed_world), _ptr(placed_cam),
                                         _stream(dev)))


def pose_track_world(pose, state, rig_pose, dt=None, dts=None, params=None, frame=None, joints3d=None, streams=1, ortho_tol=1e-6):
    """``pose_track`` in a world frame (egotap_pose_track_world, ``spec.pose_track_world_ref``): ``rig_pose`` float64 [T * streams, 12] on the pose's
    device holds, per frame, the row-major 3 x 4 (R | t) of the LEFT CAMERA IN THE WORLD, x_w = R x_c + t, t in the pose's units (``spec.rig_pose`` /
    ``spec.rig_compose`` build it).  A frame whose rig pose is not finite, not orthonormal within ``ortho_tol`` or left-handed accepts no track: the
    tracks hold as over any missing sample.  The other arguments are ``pose_track``'s; ``state`` is UPDATED IN PLACE and belongs to the frame it was
    made in (zeros suit both) -> (tracks float32 [T * streams, P + 1 + J, 8] in the world, placed_world float32 [T * streams, P, 3], placed_cam float32
    [T * streams, P, 3] = placed_world back in each frame's own camera, zeros for a frame whose rig pose is not seen).  One launch, no synchronisation."""
    import torch
    prm, T, S, P, J = _pose_track_args("pose_track_world", pose, state, dt, dts, params, frame, joints3d, streams)
    B, K = T * S, P + 1 + J
    if not torch.is_tensor(rig_pose) or rig_pose.dtype != torch.float64 or tuple(rig_pose.shape) != (B, 12):
        raise ValueError(f"pose_track_world: rig_pose is a float64 tensor [T * streams, 12] = {(B, 12)}, got "
                         f"{getattr(rig_pose, 'dtype', type(rig_pose).__name__)} {tuple(getattr(rig_pose, 'shape', ()))}")
    if not float(ortho_tol) >= 0:
        raise ValueError(f"pose_track_world: ortho_tol must be >= 0, got {ortho_tol}")
    if not _on_one_gpu(pose, frame, joints3d, dts, state, rig_pose):
        raise EgotapError("pose_track_world runs on the GPU only (no CPU fallback); pose, frame, joints3d, dts, state and rig_pose on one cuda device")
    ps, fr, j3 = _f32c(pose), _f32c(frame), _f32c(joints3d)
    tracks = torch.empty((B, K, 8), dtype=torch.float32, device=ps.device)
    placed_world = torch.empty((B, P, 3), dtype=torch.float32, device=ps.device)
    placed_cam = torch.empty((B, P, 3), dtype=torch.float32, device=ps.device)
    with torch.cuda.device(ps.device):
        pose_track_world_into(prm, ps, fr, j3, rig_pose.detach().contiguous(), T, S, dts.contiguous() if dts is not None else None, dt, ortho_tol, state, state,
                              tracks, placed_world, placed_cam, ps.device)
    return tracks, placed_world, placed_cam


def skeleton_rig_struct(rig) -> EgotapSkeletonRig:
    """a ``spec.SkeletonRig`` as the ABI takes it (egotap_skeleton_rig, by pointer to host memory)"""
    from . import spec
    if not isinstance(rig, spec.SkeletonRig):
        raise ValueError(f"skeleton_fit: rig is a spec.SkeletonRig (spec.skeleton_rig builds one), got {type(rig).__name__}")
    o = EgotapSkeletonRig()
    o.P, o.has_mirror, o.has_fixed_length = rig.P, rig.mirror is not None, rig.fixed_length is not None
    o.frame_rows[:] = rig.frame_rows
    for j in range(rig.P):
        o.parent[j] = rig.parents[j]
        o.mirror[j] = rig.mirror[j] if rig.mirror is not None else -1
        o.rest_pos[j][:] = [float(v) for v in rig.rest_pos[j]]
        o.fixed_length[j] = float(rig.fixed_length[j]) if rig.fixed_length is not None else 0.0
    return o


def skeleton_params_struct(params=None, track_rows=0) -> EgotapSkeletonParams:
    """a ``spec.SkeletonParams`` (None: the defaults) as the ABI takes it; ``track_rows``: K of the tracks array (0: none, or exactly P)"""
    from . import spec
    prm = spec.SkeletonParams() if params is None else params
    if not isinstance(prm, spec.SkeletonParams):
        raise ValueError(f"skeleton_fit: params is a spec.SkeletonParams, got {type(prm).__name__}")
    return EgotapSkeletonParams(prm.max_dev, prm.window, prm.min_samples, int(prm.freeze), int(track_rows))


def skeleton_fit_into(rig_c, prm_c, points, tracks, T, S, state_in, state_out, rigid, rotations, lengths, dev):
    """the launch itself on ``dev``'s current stream: ``rig_c`` / ``prm_c`` from ``skeleton_rig_struct`` / ``skeleton_params_struct``, tensors as the
    ABI takes them (tracks may be None; the states too with a fixed_length rig)"""
    check(load().egotap_skeleton_fit(_ptr(points), _ptr(tracks), int(T), int(S), C.byref(rig_c), C.byref(prm_c), _ptr(state_in), _ptr(state_out), _ptr(rigid),
                                     _ptr(rotations), _ptr(lengths), _stream(dev)))


def skeleton_twist_struct(twist) -> EgotapSkeletonTwist:
    """a ``spec.SkeletonTwist`` as the ABI takes it (egotap_skeleton_twist, by pointer to host memory)"""
    from . import spec
    if not isinstance(twist, spec.SkeletonTwist):
        raise ValueError(f"skeleton_fit_twist: twist is a spec.SkeletonTwist (spec.skeleton_twist builds one), got {type(twist).__name__}")
    o = EgotapSkeletonTwist()
    o.bend_lo, o.bend_hi = twist.bend_lo, twist.bend_hi
    for j in range(64):
        o.pole[j] = twist.pole[j] if j < twist.P else -1
        if j < twist.P:
            o.hinge[j][:] = [float(v) for v in twist.hinge[j]]
    return o


def skeleton_fit_twist_into(rig_c, twist_c, prm_c, points, tracks, T, S, state_in, state_out, rigid, rotations, lengths, dev):
    """the launch itself on ``dev``'s current stream, as ``skeleton_fit_into`` with ``twist_c`` from ``skeleton_twist_struct``"""
    check(load().egotap_skeleton_fit_twist(_ptr(points), _ptr(tracks), int(T), int(S), C.byref(rig_c), C.byref(twist_c), C.byref(prm_c), _ptr(state_in),
                                           _ptr(state_out), _ptr(rigid), _ptr(rotations), _ptr(lengths), _stream(dev)))


def skeleton_fit(points, state, rig, params=None, tracks=None, streams=1, _structs=None):
    """A rigid skeleton and a rotation per bone from tracked joint positions (egotap_skeleton_fit, ``spec.skeleton_fit_ref``): points float32
    [T * streams, P, 3] on the GPU, T consecutive frames of ``streams`` camera rigs, time-major -- a tracker's ``placed``, ``placed_world`` or
    ``placed_cam``; ``state`` float64 [streams, P, 2] = (L^, n) per row on the same device, all zeros for uncalibrated, UPDATED IN PLACE (None with a
    rig that has ``fixed_length``, which reads and writes none); ``rig`` a ``spec.SkeletonRig`` of the same P; ``params`` a ``spec.SkeletonParams``
    (None: its defaults); ``tracks`` float32 [T * streams, K, 8] the tracker's records (a row then also needs status 1 or 2 to count as seen)
    -> (rigid float32 [T * streams, P, 4] = (x, y, z, flags), rotations float32 [T * streams, P, 8] = (global wxyz, local wxyz), lengths float32
    [T * streams, P, 2] = (the length used, n)).  One launch on the current stream, no synchronisation."""
    return _skeleton_fit("skeleton_fit", points, state, rig, None, params, tracks, streams, _structs)


def skeleton_fit_twist(points, state, rig, twist, params=None, tracks=None, streams=1, _structs=None):
    """``skeleton_fit`` with the bone twist taken from the bend plane of the child bone (egotap_skeleton_fit_twist, ``spec.skeleton_fit_twist_ref``):
    ``twist`` a ``spec.SkeletonTwist`` of the same rig (``spec.skeleton_twist`` builds one); every other argument and the three results as
    ``skeleton_fit``'s, with flags = 1 (position ok) + 2 (rotation ok) + 4 (twist observed).  rigid[..., :3], lengths and the state are
    ``skeleton_fit``'s in bits.  One launch on the current stream, no synchronisation."""
    twist_c = _structs[2] if _structs is not None else skeleton_twist_struct(twist)
    if twist.P != getattr(rig, "P", twist.P):              # (a rig of another type is refused below, by name)
        raise ValueError(f"skeleton_fit_twist: the twist table has P = {twist.P} rows, the rig {rig.P}")
    return _skeleton_fit("skeleton_fit_twist", points, state, rig, twist_c, params, tracks, streams, None if _structs is None else _structs[:2])


def _skeleton_fit(who, points, state, rig, twist_c, params, tracks, streams, _structs):
    """the argument checks, the outputs and the launch of ``skeleton_fit`` (``twist_c`` None) and ``skeleton_fit_twist``"""
    import torch
    rig_c, prm_c = _structs if _structs is not None else (skeleton_rig_struct(rig), skeleton_params_struct(params))
    S, P = int(streams), rig.P
    if not torch.is_tensor(points) or points.dim() != 3 or points.shape[2] != 3 or S < 1 or points.shape[0] < S or points.shape[0] % S:
        raise ValueError(f"{who}: points is a tensor [T * streams, P, 3] with T >= 1, got {tuple(getattr(points, 'shape', ()))} for {streams} streams")
    if points.shape[1] != P:
        raise ValueError(f"{who}: the rig has P = {P} rows, points has {points.shape[1]}")
    if points.dtype != torch.float32 or not points.is_contiguous():
        raise ValueError(f"{who}: points is a contiguous float32 tensor, got {points.dtype}{'' if points.is_contiguous() else ', not contiguous'}")
    B = int(points.shape[0])
    T = B // S
    K = 0
    if tracks is not None:
        if not torch.is_tensor(tracks) or tracks.dim() != 3 or tracks.shape[0] != B or tracks.shape[1] < P or tracks.shape[2] != 8:
            raise ValueError(f"{who}: tracks is a tensor [T * streams, K, 8] with K >= P = {P}, got {tuple(getattr(tracks, 'shape', ()))} for {B} frames")
        if tracks.dtype != torch.float32 or not tracks.is_contiguous():
            raise ValueError(f"{who}: tracks is a contiguous float32 tensor, got {tracks.dtype}{'' if tracks.is_contiguous() else ', not contiguous'}")
        K = int(tracks.shape[1])
    fixed = rig.fixed_length is not None
    if fixed and state is not None:
        raise ValueError(f"{who}: a rig with fixed_length calibrates nothing: it reads and writes no state (pass state=None)")
    if not fixed and (not torch.is_tensor(state) or tuple(state.shape) != (S, P, 2) or state.dtype != torch.float64 or not state.is_contiguous()):
        raise ValueError(f"{who}: state is a contiguous float64 tensor [streams, P, 2] = {(S, P, 2)}, got "
                         f"{getattr(state, 'dtype', type(state).__name__)} {tuple(getattr(state, 'shape', ()))}")
    if not _on_one_gpu(points, tracks, state):
        raise EgotapError(f"{who} runs on the GPU only (no CPU fallback); points, tracks and state on one cuda device")
    prm_c.track_rows = K
    rigid = torch.empty((B, P, 4), dtype=torch.float32, device=points.device)
    rotations = torch.empty((B, P, 8), dtype=torch.float32, device=points.device)
    lengths = torch.empty((B, P, 2), dtype=torch.float32, device=points.device)
    with torch.cuda.device(points.device):
        trk = tracks.detach() if tracks is not None else None
        if twist_c is None:
            skeleton_fit_into(rig_c, prm_c, points.detach(), trk, T, S, state, state, rigid, rotations, lengths, points.device)
        else:
            skeleton_fit_twist_into(rig_c, twist_c, prm_c, points.detach(), trk, T, S, state, state, rigid, rotations, lengths, points.device)
    return rigid, rotations, lengths


KINEMATIC_PARENTS = {          # utils/util.py:51-52
    "UnrealEgo": [0, 0, 1, 1, 2, 3, 4, 5, 2, 3, 8, 9, 10, 11, 12, 13],
    "EgoCap": [0, 0, 1, 2, 3, 4, 1, 6, 7, 8, 2, 10, 11, 12, 6, 14, 15, 16],
}


def synth_heatmaps(pts2d_left, pts2d_right, pose3d, joint_preset: str = "UnrealEgo", res: int = 64):
    """Ground-truth heatmaps on the device (egotap_synth_heatmaps): joints [B, J+1, 2] x 2 eyes in the 1024-pixel frame and
    gt_local_pose [B, J+1, 3] -> dict with the data loader's keys plus ``cat`` [B, 6J, res, res], the lifting head's input."""
    import torch
    parents = KINEMATIC_PARENTS[joint_preset]
    J1 = len(parents)
    J = J1 - 1
    pl, pr, p3 = (t.detach().float().contiguous() for t in (pts2d_left, pts2d_right, pose3d))
    _need_cuda_f32(pl, pr, p3)
    B = pl.shape[0]
    if tuple(pl.shape) != (B, J1, 2) or tuple(pr.shape) != (B, J1, 2) or tuple(p3.shape) != (B, J1, 3):
        raise ValueError(f"expected [B, {J1}, 2] x 2 and [B, {J1}, 3] for {joint_preset}")
    dev = pl.device
    par = torch.tensor(parents, dtype=torch.int32, device=dev)
    cat = torch.empty((B, 6 * J, res, res), device=dev)
    plen = torch.empty((B, 2, J), device=dev)
    theta = torch.empty((B, J), device=dev)
    check(load().egotap_synth_heatmaps(_ptr(pl), _ptr(pr), _ptr(p3), _ptr(par), B, J, res, _ptr(cat), _ptr(plen), _ptr(theta), _stream()))
    return {"cat": cat, "gt_heatmap_left": cat[:, :J], "gt_heatmap_right": cat[:, J:2 * J],
            "gt_limb_heatmap_left": cat[:, 2 * J:4 * J], "gt_limb_heatmap_right": cat[:, 4 * J:],
            "gt_plength_left": plen[:, 0].repeat(1, 2), "gt_plength_right": plen[:, 1].repeat(1, 2), "gt_limb_theta": theta}


def layernorm(x, gamma, beta, eps: float = 1e-12):
    import torch
    _need_cuda_f32(x, gamma, beta)
    y = torch.empty_like(x)
    rows = x.numel() // x.shape[-1]
    check(load().egotap_layernorm_f32(_ptr(x), _ptr(y), _ptr(gamma), _ptr(beta), rows, x.shape[-1], eps, _stream()))
    return y


def attention_f32_shared(qkv, B: int, N: int, heads: int, shared_from: int):
    """(test hook, egotap_debug.h) the exact-fp32 attention where tokens [shared_from, N) are the same in every image: their q | k | v rows are
    read from image 0, rows (b > 0, n >= shared_from) of qkv not at all.  qkv [B*N, 3*heads*128] -> ctx [B*N, heads*128]"""
    import torch
    _need_cuda_f32(qkv)
    ctx = torch.empty((B * N, heads * 128), device=qkv.device, dtype=torch.float32)
    check(load().egotap_debug_attention_f32_shared(_ptr(qkv), _ptr(ctx), B, N, heads, shared_from, _stream()))
    return ctx


def _attention_out(out, rows: int, heads: int, dev):
    """the ctx buffer of an attention wrapper: a fresh [rows, heads*128], or the caller's ``out`` (at least that many rows; the tests put sentinel
    rows behind them)"""
    import torch
    if out is None:
        return torch.empty((rows, heads * 128), device=dev, dtype=torch.float32)
    _need_cuda_f32(out)
    if out.dim() != 2 or out.shape[0] < rows or out.shape[1] != heads * 128 or out.device != dev:
        raise ValueError(f"out: a float32 tensor [>= {rows}, {heads * 128}] on {dev}, got {tuple(out.shape)} on {out.device}")
    return out


def attention_f32_ksplit(B: int, N: int, heads: int, scratch_floats: int, num_cu: int = 256) -> int:
    """(test aid, host only) the key-split count the fp32 attention of a forward picks: 1 = unsplit"""
    k = load().egotap_debug_attention_f32_ksplit(B, N, heads, scratch_floats, num_cu)
    if k <= 0:
        check(1)
    return k


TN_FAMILIES = {0: "none", 1: "f32_big", 2: "f32_small", 3: "f32_dma", 4: "bf16x3", 5: "bf16"}      # egotap_debug.h EGOTAP_TN_*
PU_WGRADS = ("x2f0", "x2h0", "b2h0", "h2h0", "x2f1", "x2h1", "h2h1")                                   # the order of egotap_train_pu_bwd's grads
PU_DGRADS = ("step", "x2h1", "x2f1", "b2h0", "x2h0", "x2f0")


def pu_train_routes(h, B: int, resident=None, num_cu: int = 256) -> dict:
    """(test aid, egotap_debug.h) which kernels the PU stage of training launches at batch ``B`` on handle ``h``, as a dictionary: "chain" (0 per
    step, 1, 2), "chunks", "row_blocks", "last_rows", "colsum_gy", and per GEMM name "wgrad_splits", "wgrad_family" (TN_FAMILIES), "wgrad_capped",
    "dgrad_splitk".  ``resident`` = None asks the device; (resident1, resident2) with ``num_cu`` is host only."""
    out = (C.c_int * 32)()
    if resident is None:
        check(load().egotap_debug_pu_train_routes(h, B, out, 32))
    else:
        check(load().egotap_debug_pu_train_routes_for(h, B, int(resident[0]), int(resident[1]), num_cu, out, 32))
    v = list(out)
    return {"chain": v[0], "chunks": v[1], "row_blocks": v[2], "last_rows": v[3], "colsum_gy": v[31],
            "wgrad_splits": dict(zip(PU_WGRADS, v[4:11])), "wgrad_family": {k: TN_FAMILIES[f] for k, f in zip(PU_WGRADS, v[11:18])},
            "wgrad_capped": dict(zip(PU_WGRADS, v[18:25])), "dgrad_splitk": dict(zip(PU_DGRADS, v[25:31]))}


def attention_f32_split(qkv, B: int, N: int, heads: int, scratch, scratch_floats: int, num_cu: int = 256, out=None):
    """(test hook, egotap_debug.h) the exact-fp32 attention as the forward launches it, key-split partials in the first ``scratch_floats`` floats
    of ``scratch``; the split count is ``attention_f32_ksplit`` of the same arguments.  qkv [B*N, 3*heads*128] -> ctx [B*N, heads*128]"""
    _need_cuda_f32(qkv, scratch)
    if scratch.numel() < scratch_floats:
        raise ValueError(f"scratch holds {scratch.numel()} floats, scratch_floats = {scratch_floats}")
    ctx = _attention_out(out, B * N, heads, qkv.device)
    check(load().egotap_debug_attention_f32_split(_ptr(qkv), _ptr(ctx), B, N, heads, _ptr(scratch), scratch_floats, num_cu, _stream()))
    return ctx


def attention_f32_live(q, ldq: int, Nq: int, qkv, B: int, N: int, heads: int, out=None):
    """(test hook, egotap_debug.h) Nq live queries per image -- row b*Nq + i of ``q``, row stride ``ldq`` floats (``q`` may be ``qkv`` itself with
    ldq = 3*heads*128: the product's layout) -- against the keys and values of all N tokens of qkv [B*N, 3*heads*128] -> ctx [B*Nq, heads*128]"""
    _need_cuda_f32(q, qkv)
    if q.numel() < (B * Nq - 1) * ldq + heads * 128:
        raise ValueError(f"q holds {q.numel()} floats: fewer than {B * Nq} rows of stride {ldq}")
    ctx = _attention_out(out, B * Nq, heads, qkv.device)
    check(load().egotap_debug_attention_f32_live(_ptr(q), ldq, Nq, _ptr(qkv), _ptr(ctx), B, N, heads, _stream()))
    return ctx


def attention(qkv, B: int, N: int, heads: int, precision: str = "f32", out=None):
    """qkv [B*N, 3*heads*128] (q|k|v) -> ctx [B*N, heads*128] (``out``: the caller's buffer of at least that many rows)"""
    _need_cuda_f32(qkv)
    ctx = _attention_out(out, B * N, heads, qkv.device)
    check(load().egotap_attention(_ptr(qkv), _ptr(ctx), B, N, heads, PRECISIONS[precision], _stream()))
    return ctx
