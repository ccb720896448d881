"""TEST INFRASTRUCTURE ONLY: plain-numpy restatement of one ScanNet loader item.

The checker of ov3d_amd.scannet / csrc/scanaug.hip at sizes the golden file does not hold.  It
restates ScannetDetectionDataset.__getitem__ (datasets/scannet.py:256-417, use_image /
use_height off) for one raw scan and a numpy RandomState, with numpy's own dtype rules, so the
rounding is the reference's: colour normalisation (:287-293), random_sampling (:319-321), flips
and rotation (:339-357), labels and normalisations (:359-416).  Pinned against the reference's own
outputs by tests/test_scannet_aug_ref_cpu.py (tests/golden/scannet_aug.npz).
"""
import numpy as np

MEAN_RGB = np.array([109.8, 97.2, 83.8])


def _rotz(t):
    c, s = np.cos(t), np.sin(t)
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])


def _realign(boxes, R):
    """rotate_aligned_boxes (:148-169): rotated centres; twice the largest rotated corner
    offset in x and in y; z length kept.  float32 boxes in, float64 out."""
    half = boxes[:, 3:5] / 2.0
    ext = np.zeros((len(boxes), 4, 3))
    for q, (sx, sy) in enumerate(((-1, -1), (1, -1), (1, 1), (-1, 1))):
        off = np.zeros((len(boxes), 3))
        off[:, 0] = sx * half[:, 0]
        off[:, 1] = sy * half[:, 1]
        ext[:, q] = np.dot(off, R.T)
    return np.concatenate([np.dot(boxes[:, 0:3], R.T), 2.0 * ext[:, :, 0].max(1)[:, None],
                           2.0 * ext[:, :, 1].max(1)[:, None], boxes[:, 5:6]], axis=1)


def _corners_camera(sizes, centers):
    """flip_axis_to_camera_np + get_3d_box_batch_np at angle 0 (box_util.py:255-285)"""
    cam = centers[:, [0, 2, 1]].copy()
    cam[:, 1] *= -1
    R = np.zeros((len(sizes), 3, 3))
    ang = np.zeros(len(sizes), np.float32)
    R[:, 0, 0], R[:, 0, 2], R[:, 1, 1], R[:, 2, 0], R[:, 2, 2] = np.cos(ang), np.sin(ang), 1, -np.sin(ang), np.cos(ang)
    l, w, h = (sizes[:, k:k + 1] for k in range(3))
    loc = np.zeros((len(sizes), 8, 3))
    loc[..., 0] = np.concatenate((l / 2, l / 2, -l / 2, -l / 2, l / 2, l / 2, -l / 2, -l / 2), -1)
    loc[..., 1] = np.concatenate((h / 2, h / 2, h / 2, h / 2, -h / 2, -h / 2, -h / 2, -h / 2), -1)
    loc[..., 2] = np.concatenate((w / 2, -w / 2, -w / 2, w / 2, w / 2, -w / 2, -w / 2, w / 2), -1)
    return np.matmul(loc, np.swapaxes(R, -1, -2)) + cam[:, None, :]


def scannet_item(vert, boxes, rng, id2class, num_points=40000, use_color=False, augment=True,
                 G=64, feature=None):
    """one reference __getitem__ -> dict (numpy).  vert (n, 6) float32|float64, boxes (k, 7),
    id2class {nyu40 id: class}, feature: feature_2d[pre_subsample_inds] (n, D) or None."""
    vert = vert.copy()
    if use_color:
        pc = vert[:, 0:6]
        pc[:, 3:] = (pc[:, 3:] - MEAN_RGB) / 256.0
        color = pc[:, 3:]
    else:
        pc, color = vert[:, 0:3], vert[:, 3:6]
    n, k = pc.shape[0], boxes.shape[0]
    sel = rng.choice(n, num_points, replace=n < num_points)
    pc, color = pc[sel], color[sel]
    target = np.zeros((G, 6), np.float32)
    present = np.zeros(G, np.float32)
    present[:k] = 1
    target[:k] = boxes[:, 0:6]
    if augment:
        if rng.random() > 0.5:
            pc[:, 0] = -1 * pc[:, 0]
            target[:, 0] = -1 * target[:, 0]
        if rng.random() > 0.5:
            pc[:, 1] = -1 * pc[:, 1]
            target[:, 1] = -1 * target[:, 1]
        R = _rotz((rng.random() * np.pi / 18) - np.pi / 36)
        pc[:, 0:3] = np.dot(pc[:, 0:3], R.T)
        target = _realign(target, R)
    sizes = target[:, 3:6].astype(np.float32)
    centers = target.astype(np.float32)[:, 0:3]
    dmin, dmax = pc.min(axis=0)[:3], pc.max(axis=0)[:3]
    one, zero = np.ones((1, 3), np.float32), np.zeros((1, 3), np.float32)
    centers_n = (((centers - dmin[None]) * (one - zero)) / (dmax[None] - dmin[None]) + zero) * present[:, None]
    sizes_n = sizes * (1.0 / (dmax - dmin)[None])
    sem = np.zeros(G)
    sem[:k] = [id2class[int(x)] for x in boxes[:, -1]]
    out = {
        "point_clouds": pc.astype(np.float32),
        "gt_box_corners": _corners_camera(sizes, centers).astype(np.float32),
        "gt_box_centers": centers,
        "gt_box_centers_normalized": centers_n.astype(np.float32),
        "gt_angle_class_label": np.zeros(G, np.int64),
        "gt_angle_residual_label": np.zeros(G, np.float32),
        "gt_box_sem_cls_label": sem.astype(np.int64),
        "gt_box_present": present,
        "pcl_color": color,
        "gt_box_sizes": sizes,
        "gt_box_sizes_normalized": sizes_n.astype(np.float32),
        "gt_box_angles": np.zeros(G, np.float32),
        "point_cloud_dims_min": dmin.astype(np.float32),
        "point_cloud_dims_max": dmax.astype(np.float32),
    }
    if feature is not None:
        out["feature_2d"] = feature[sel]
    return out
