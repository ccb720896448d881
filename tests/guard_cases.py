"""The closed set of the guard-band suite: which entries of the headers (include/ov3d.h and the
include/ov3d_*.h beside it) the cases of tests/test_guard_*_gpu.py and of the feature GPU files
run between guard bands (read from each file's ENTRIES tuple, without importing it: no GPU
needed), and which writing entries are not guarded yet, each with a one-line reason.
tests/test_guard_cpu.py checks that the two cover every entry that has a writable pointer
parameter and that no name is in both."""
import ast
import os

HERE = os.path.dirname(os.path.abspath(__file__))
MODULES = ("test_guard_gemm_gpu", "test_guard_rows_gpu", "test_guard_attention_gpu",
           "test_guard_points_gpu", "test_lift_gpu", "test_lift_single_gpu", "test_box_eval_gpu",
           "test_backproj_gpu", "test_pool_label_gpu", "test_open_vocab_gpu", "test_detect_gpu",
           "test_nms_large_gpu", "test_label_vote_gpu")


def path(module):
    return os.path.join(HERE, module + ".py")


def _entries(module):
    for node in ast.parse(open(path(module)).read()).body:
        if isinstance(node, ast.Assign) and any(getattr(t, "id", None) == "ENTRIES" for t in node.targets):
            return tuple(ast.literal_eval(node.value))
    raise AssertionError(f"{module}: no ENTRIES tuple")


CASE_FILES = {m: _entries(m) for m in MODULES}


def guarded():
    return {name for names in CASE_FILES.values() for name in names}


_SA = "fused SA chain: fixed 64-row tiles with R % 64 == 0 enforced, no ragged tail"
_GEOM = "one thread per element (geometry / set loss); next after the tiled kernels"
_CLIP = "RegionCLIP image kernel; next after the tiled kernels"
_LOADER = "data loader (SUN RGB-D / ScanNet batches); next after the tiled kernels"
_EVAL = "evaluation kernel; next after the tiled kernels"
_HOST = "host-only: writes no device memory"
_BN1 = "per-channel BatchNorm finalize of the fused SA chain: C threads, no row tiles"

NOT_GUARDED = {
    **{n: _SA for n in (
        "ov3d_sa_l1_fwd", "ov3d_sa_l1_fwd_cin", "ov3d_sa_layer_fwd", "ov3d_sa_layer_fwd_x0",
        "ov3d_sa_layer_pool_fwd", "ov3d_sa_layer_dy", "ov3d_sa_dy2_fused", "ov3d_sa_dy_fused",
        "ov3d_sa_pool_fwd", "ov3d_sa_pool_bwd", "ov3d_bn_relu_bwd", "ov3d_bn_relu_bwd_cin")},
    **{n: _BN1 for n in ("ov3d_bn_finalize", "ov3d_bn_stats_finalize", "ov3d_bn_bwd_stats_finalize",
                         "ov3d_bn_bwd_finalize")},
    **{n: _GEOM for n in (
        "ov3d_giou3d", "ov3d_giou3d_bwd", "ov3d_giou3d_bwd_aligned", "ov3d_hungarian",
        "ov3d_nms_boxes_from_corners", "ov3d_matcher_cost", "ov3d_targets_prep", "ov3d_set_loss_fwd",
        "ov3d_set_loss_fwd_split", "ov3d_set_loss_bwd", "ov3d_box_param_fwd", "ov3d_box_param_bwd",
        "ov3d_project_box2d", "ov3d_fourier_pe")},
    **{n: _CLIP for n in (
        "ov3d_clip_preprocess", "ov3d_roi_align_fwd", "ov3d_roi_align_pool2_fwd", "ov3d_im2col3x3",
        "ov3d_bias_residual_act", "ov3d_avgpool2_nhwc", "ov3d_attnpool_tokens", "ov3d_attnpool_mean",
        "ov3d_attnpool_fused")},
    **{n: _LOADER for n in (
        "ov3d_sun_aug_points", "ov3d_sun_aug_boxes", "ov3d_sun_cuboid_eval", "ov3d_sun_crop_sample",
        "ov3d_sun_labels", "ov3d_scan_sample_aug", "ov3d_scan_labels", "ov3d_rows_gather")},
    **{n: _EVAL for n in ("ov3d_box3d_iou_eval", "ov3d_ap_match", "ov3d_ap_curve")},
    "ov3d_adamw_step": "AdamW: one chunk table per tensor list; next after the tiled kernels",
    "ov3d_adamw_set_grads": "AdamW table setup (one pointer per tensor); next after the tiled kernels",
    "ov3d_multi_copy": "byte copies between caller-sized buffers; next after the tiled kernels",
    "ov3d_seed_next": "two int64 scalars, one thread",
    "ov3d_stream_create": _HOST,
    "ov3d_stamps_get": _HOST,
    "ov3d_wgrad_group_workspace": _HOST + " (a size function; its value is the G5 case of ov3d_wgrad_group)",
    "ov3d_stamps_arm": "measurement only: arms launch stamps into a bench.py buffer",
    "ov3d_lngemm_stamps_arm": "measurement only: arms phase clocks into a bench.py buffer",
}
