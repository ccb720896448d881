"""Synthetic inputs of tests/golden/evaldet_large.npz and tests/golden/nms_large.npz (shared by
make_eval_large_golden.py and the tests): evaluation at more proposals than the small kernels
take, and the 2D NMS.  Scenes as in eval_cases.py, regenerated bit-identically from numpy
PCG64 seeds; the objectness of a scene is made tie-free (eval_cases gives its low-objectness
boxes one shared value, and the reference's order among equal scores is numpy's quicksort)."""
import numpy as np

from eval_cases import _scene
from ov3d_amd import synthetic
from ov3d_amd.dataset_config import SunrgbdDatasetConfig

NMS_THRESHOLD = 0.25
# every overlap the reference compares with the NMS threshold is further than this from it
MARGIN = 1e-9


def _data(K, seed, copies=None):
    return dict(num_batches=1, batch=2, K=K, num_points=4000, num_classes=20, seed=seed, copies=copies)


# copies: jittered predictions per GT box (eval_cases._scene draws 1 - 3, which leaves the
# class-wise NMS under 20 boxes to suppress in a scene of at most 10 objects)
CONFIGS = {
    "exact_576": dict(data=_data(576, 0, copies=(4, 10)), ap=dict(remove_empty_box=True)),
    "any_class_576": dict(data=_data(576, 1), ap=dict(remove_empty_box=True, cls_nms=False)),
    "old_type_640": dict(data=_data(640, 2), ap=dict(use_old_type_nms=True, remove_empty_box=False)),
    "nms2d_64": dict(data=_data(64, 81), ap=dict(use_3d_nms=False, remove_empty_box=True)),
    "nms2d_576": dict(data=_data(576, 4), ap=dict(use_3d_nms=False, remove_empty_box=False)),
}


def _tie_free(rng, obj):
    """redraw every repeated objectness (below the 0.05 confidence threshold, as eval_cases
    puts them) until the scene's float32 scores are distinct"""
    obj = obj.copy()
    while True:
        _, first, counts = np.unique(obj, return_index=True, return_counts=True)
        if (counts == 1).all():
            return obj
        dup = np.ones(obj.shape[0], bool)
        dup[first] = False
        obj[dup] = rng.uniform(0, 0.05, int(dup.sum())).astype(np.float32)


def _scene_copies(rng, K, num_points, C, copies):
    """eval_cases._scene with copies[0] .. copies[1] jittered predictions per GT box"""
    cfg = SunrgbdDatasetConfig()
    sc = synthetic.make_scene(rng, num_points=num_points, cfg=cfg)
    nobj = int(sc["gt_box_present"].sum())
    src = np.concatenate([np.full(int(rng.integers(copies[0], copies[1] + 1)), g) for g in range(nobj)])[:K]
    n = src.size
    cen = np.zeros((K, 3), np.float32)
    siz = np.zeros((K, 3), np.float32)
    ang = np.zeros(K, np.float32)
    cen[:n] = sc["gt_box_centers"][src] + rng.normal(0, 0.12, (n, 3))
    siz[:n] = sc["gt_box_sizes"][src] * rng.uniform(0.75, 1.25, (n, 3))
    ang[:n] = sc["gt_box_angles"][src] + rng.normal(0, 0.15, n)
    cls = rng.integers(0, C, K)
    right = rng.random(n) < 0.8
    cls[:n][right] = sc["gt_box_sem_cls_label"][src][right]
    m = K - n          # boxes elsewhere in the room (many of them empty)
    cen[n:] = np.stack([rng.uniform(-2.8, 2.8, m), rng.uniform(0.7, 6.3, m), rng.uniform(0.1, 2.5, m)], 1)
    siz[n:] = rng.uniform(0.2, 1.5, (m, 3))
    ang[n:] = rng.uniform(-np.pi, np.pi, m)
    corners = cfg.box_parametrization_to_corners_np(cen[None], siz[None], ang[None])[0]
    logits = rng.normal(0, 1, (K, C))
    logits[np.arange(K), cls] += rng.uniform(1.0, 4.0, K)
    p = np.exp(logits - logits.max(1, keepdims=True))
    p /= p.sum(1, keepdims=True)
    return {
        "point_clouds": sc["point_clouds"],
        "pred_corners": corners.astype(np.float32),
        "sem_cls_prob": p.astype(np.float32),
        "objectness_prob": rng.uniform(0, 1, K).astype(np.float32),
        "gt_box_corners": sc["gt_box_corners"],
        "gt_box_sem_cls_label": sc["gt_box_sem_cls_label"],
        "gt_box_present": sc["gt_box_present"],
    }


def make_batches(num_batches, batch, K, num_points, num_classes, seed, copies=None):
    out = []
    for bi in range(num_batches):
        scenes = []
        for i in range(batch):
            rng = np.random.Generator(np.random.PCG64(1000 * seed + 10 * bi + i))
            sc = (_scene(rng, K, num_points, num_classes) if copies is None else
                  _scene_copies(rng, K, num_points, num_classes, copies))
            sc["objectness_prob"] = _tie_free(rng, sc["objectness_prob"])
            scenes.append(sc)
        out.append({k: np.stack([s[k] for s in scenes]) for k in scenes[0]})
    return out


# ---- nms_large.npz: box tables past the small kernel's 512 rows, and 2D tables ----
NMS3D_K = (513, 1100, 2048)
NMS2D_K = (37, 700)


def nms3d_table(i):
    """(K, 8) [x1,y1,z1,x2,y2,z2,score,cls], distinct scores, 4 classes"""
    K = NMS3D_K[i]
    rng = np.random.Generator(np.random.PCG64(7700 + i))
    lo = rng.uniform(-1.2, 1.2, (K, 3))
    sz = rng.uniform(0.2, 1.5, (K, 3))
    boxes = np.zeros((K, 8))
    boxes[:, 0:3] = lo
    boxes[:, 3:6] = lo + sz
    boxes[:, 6] = rng.permutation(K) / K + rng.uniform(0, 1e-4, K)
    boxes[:, 7] = rng.integers(0, 4, K)
    return boxes


def nms2d_table(i):
    """(K, 5) [x1,y1,x2,y2,score], distinct scores"""
    K = NMS2D_K[i]
    rng = np.random.Generator(np.random.PCG64(7800 + i))
    half = (K / 37.0) ** 0.5   # the same density at both sizes
    lo = rng.uniform(-half, half, (K, 2))
    sz = rng.uniform(0.2, 1.5, (K, 2))
    boxes = np.zeros((K, 5))
    boxes[:, 0:2] = lo
    boxes[:, 2:4] = lo + sz
    boxes[:, 4] = rng.permutation(K) / K + rng.uniform(0, 1e-4, K)
    return boxes
