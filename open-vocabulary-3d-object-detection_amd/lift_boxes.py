"""3D pseudo boxes from 2D detections (stage 3 of the open-vocabulary pipeline), on the device.

Replaces ``3DOVDet_tools/scannet/lift_boxes.py`` (``VIEW='multi'``, ``PSEUDO_FLAG=True``,
``USE_GSS=True``) and ``3DOVDet_tools/sunrgbd/lift_boxes.py`` with their helpers in
``utils/projection.py`` and ``utils/box_3d_utils.py``.  Inputs are arrays; decoding images is
not part of it.

Host (numpy, a few hundred tiny operations per scan): the edge filter, the eight frustum
corners and six plane normals of every 2D box with the calls the reference makes
(``np.linalg.inv`` of the float32 intrinsic, the float32 pose product, ``np.cross``, the
division by the squared norm), the inverse of the alignment matrix, and the compaction and row
order after the single read-back.

Device (csrc/lift.hip behind include/ov3d_lift.h), back to back on the current stream with no
synchronisation in between: the lift (``ov3d_lift_frustum`` over the vertices, or
``ov3d_lift_image`` over each box's pixel rectangle), the class-wise NMS with the tools'
arithmetic (``ov3d_lift_nms``), the match against the proposal pool with the labelled pool rows
(``ov3d_lift_match``), and the size NMS (``ov3d_lift_nms`` again).  One device-to-host copy.

The scripts' ``VIEW='single'`` is ``lift_scannet_scan_single`` (``ScannetBoxLifter(view="single")``
from files): no vertex cloud; a 2D box lifts every pixel of its frame whose class equals its
label (the rectangle is not consulted, as in the reference) through depth, pose and alignment.
Host: the halved copy of the intrinsic and numpy's inverse of it, the widened poses, the edge
filter and the table of slots, one per distinct (frame, label) pair.  Device
(csrc/liftview.hip behind include/ov3d_liftview.h): ``ov3d_liftview_frames``, one workgroup per
slot and a second launch that gives every box its slot's bounds, then the same chain.  Depth is
float32 metres or raw uint16 millimetres; per-frame labels may be a device int32 tensor (the
first result of ``open_vocab.classify_frames``), which is read where it lies.  PIL decodes the
PNGs of the file driver and is imported inside that call only.

Number formats: 2D boxes keep the dtype they come in for the plane construction (as in the
reference); the proposal pool and the alignment are taken as float64; float32 vertices are
widened on the device.  Scores must be finite.  Ties between equal scores go to the higher row
(the reference leaves them to ``argsort``); nothing pins that rule.

Limits: at most 2048 lifted boxes per class and 8192 per scan (one NMS workgroup); beyond them
``ValueError`` before any launch.
"""
import os

import numpy as np
import torch

from . import _native as nat

NYU40IDS = np.array([3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14, 16, 24, 28, 33, 34, 36, 39])
SUNRGBD37IDS = (36, 4, 10, 29, 5, 12, 14, 8, 17, 35, 32, 18, 34, 6, 7, 25, 33)
IGNORE_LABEL = -100
PSEUDO_IGNORE_FROM = 18            # pseudo labels of this value and above are ignored
DEPTH_MIN, DEPTH_MAX = 0.1, 10.0
IMAGE_DIMS = (240, 320)            # the frames the 2D boxes live in; the intrinsic is 640 x 480
MAX_PER_CLASS = 2048
MAX_BOXES = 8192                   # OV3D_LIFT_NMS_MAX
_NEVER_POINT, _NEVER_BOX = -2 ** 31, -2 ** 31 + 1

# corners (a, b, o) of each plane: its inward normal is cross(a - o, b - o)
_PLANE_A, _PLANE_B, _PLANE_O = [3, 2, 3, 0, 1, 6], [1, 5, 6, 7, 4, 4], [0, 1, 2, 3, 0, 5]


def edge_filter(boxes, image_dims):
    """drop the 2D boxes that touch the image border (exact float compares)"""
    if boxes.shape[0] == 0:
        return boxes
    keep = ((boxes[:, 0] != 0) & (boxes[:, 1] != 0) & (boxes[:, 0] + boxes[:, 2] != image_dims[1])
            & (boxes[:, 1] + boxes[:, 3] != image_dims[0]))
    return boxes[keep]


def frustum_planes(intrinsic, pose, boxes):
    """(k,24) float64 per 2D box of one frame: six inward normals, then corners 2 and 4.
    intrinsic: the halved (4,4) float32 matrix; pose: (4,4) float32 camera-to-world."""
    out = np.empty((len(boxes), 24))
    inv = np.linalg.inv(intrinsic[:3, :3])
    depth = np.repeat(np.array([DEPTH_MIN, DEPTH_MAX]), 4)
    with np.errstate(all="ignore"):
        for i, box in enumerate(boxes):
            x, y, w, h = box[:4]
            u = np.array([x, x + w, x + w, x, x, x + w, x + w, x])
            v = np.array([y, y, y + h, y + h, y, y, y + h, y + h])
            uv1 = np.stack([u, v, np.ones_like(u)], axis=1)
            cam = np.ones((8, 4))
            cam[:, :3] = (inv.dot(uv1.T) * depth).T
            corners = (pose @ cam[:, :, None])[:, :3, 0]
            base = corners[_PLANE_O]
            normals = np.cross(corners[_PLANE_A] - base, corners[_PLANE_B] - base)
            normals /= np.sum(normals ** 2, axis=-1, keepdims=True)
            out[i, :18] = normals.reshape(-1)
            out[i, 18:21] = corners[2]
            out[i, 21:24] = corners[4]
    return out


def _int_labels(values, never):
    """float or integer labels -> int32; what is no int32 integer becomes `never`"""
    v = np.asarray(values)
    if v.dtype.kind in "iu":
        ok = (v >= -2 ** 31 + 2) & (v < 2 ** 31)
        return np.where(ok, v, never).astype(np.int32)
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(v) & (v == np.trunc(v)) & (np.abs(v) < 2 ** 31 - 2)
    return np.where(ok, np.where(ok, v, 0), never).astype(np.int32)


def _box_labels(boxes):
    """int(box[-1]) of every 2D box as int32"""
    lab = np.asarray(boxes[:, 5], dtype=np.float64)
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(lab) & (np.abs(lab) < 2 ** 31 - 2)
    return np.where(ok, np.trunc(np.where(ok, lab, 0)), _NEVER_BOX).astype(np.int32)


def _check_boxes(boxes2d):
    if boxes2d.ndim != 2 or boxes2d.shape[1] != 6 or boxes2d.dtype.kind != "f":
        raise ValueError(f"2D boxes: expected a float (k,6) array, got {boxes2d.dtype} {boxes2d.shape}")
    if not np.isfinite(boxes2d[:, 4]).all():
        raise ValueError("2D boxes: scores must be finite")


def _check_counts(plabel):
    if len(plabel) > MAX_BOXES:
        raise ValueError(f"{len(plabel)} 2D boxes in one scan: at most {MAX_BOXES}")
    if len(plabel) and np.unique(plabel, return_counts=True)[1].max() > MAX_PER_CLASS:
        raise ValueError(f"more than {MAX_PER_CLASS} 2D boxes of one class in one scan")


def _pool(gss_pool):
    pool = np.ascontiguousarray(np.asarray(gss_pool, dtype=np.float64))
    if pool.ndim != 2 or pool.shape[1] != 7 or pool.shape[0] == 0:
        raise ValueError(f"gss_pool: expected (P,7) with P >= 1, got {pool.shape}")
    return pool


def _want(t, name, dtype, shape):
    """device tensor of this dtype, contiguous, of this shape (None: any extent)"""
    nat.check(t, name, dtype, len(shape))
    if any(w is not None and w != g for w, g in zip(shape, t.shape)):
        raise ValueError(f"{name}: expected shape {shape}, got {tuple(t.shape)}")
    return t


def nms_boxes(boxes, thresh, valid=None, use_size_score=False, rank=None):
    """ov3d_lift_nms on device rows (K, ld) f64 -> (rank (K) int32, keep (K) uint8)"""
    nat.check(boxes, "boxes", torch.float64, 2)
    K, ld = boxes.shape
    if K > MAX_BOXES:
        raise ValueError(f"{K} boxes: at most {MAX_BOXES}")
    if ld < 8 + bool(use_size_score):
        raise ValueError(f"boxes: {ld} columns, the NMS reads {8 + bool(use_size_score)}")
    if valid is not None:
        _want(valid, "valid", torch.int32, (K,))
    if rank is None:
        rank = torch.empty(K, dtype=torch.int32, device=boxes.device)
    _want(rank, "rank", torch.int32, (K,))
    keep = torch.empty(K, dtype=torch.uint8, device=boxes.device)
    nat.call("ov3d_lift_nms", boxes, ld, K, valid, int(bool(use_size_score)), float(thresh), rank,
             keep, like=boxes)
    return rank, keep


def match_pool(boxes, rank, pool, match, out=None):
    """ov3d_lift_match -> dict of device tensors amax, maxiou, win, rows (M,10), out (M,10)"""
    nat.check(boxes, "boxes", torch.float64, 2)
    M, ld = boxes.shape
    _want(rank, "rank", torch.int32, (M,))
    _want(pool, "pool", torch.float64, (None, 7))
    P = pool.shape[0]
    if ld < 8 or M < 1 or P < 1:
        raise ValueError(f"boxes (M >= 1, >= 8 columns) and pool (P >= 1): got {tuple(boxes.shape)}, P = {P}")
    if out is not None:
        _want(out, "out", torch.float64, (M, 10))
    dev = boxes.device
    owner = torch.empty(P, dtype=torch.int32, device=dev)
    r = {"amax": torch.empty(M, dtype=torch.int32, device=dev),
         "maxiou": torch.empty(M, dtype=torch.float64, device=dev),
         "win": torch.empty(M, dtype=torch.int32, device=dev),
         "rows": torch.empty(M, 10, dtype=torch.float64, device=dev),
         "out": torch.empty(M, 10, dtype=torch.float64, device=dev) if out is None else out}
    nat.call("ov3d_lift_match", boxes, ld, rank, M, pool, P, float(match), owner, r["amax"],
             r["maxiou"], r["win"], r["rows"], r["out"], like=boxes)
    return r


def lift_frusta(points, labels, align, align_inv, planes, plabel, rows, count=None):
    """ov3d_lift_frustum: fills columns 0-5 of the device rows (M, ld) -> count (M) int32"""
    nat.check(points, "points", None, 2)
    if points.dtype not in (torch.float32, torch.float64) or points.shape[1] != 3:
        raise TypeError("points: expected (N,3) float32 or float64")
    N, M = points.shape[0], planes.shape[0]
    _want(labels, "labels", torch.int32, (N,))
    _want(align, "align", torch.float64, (4, 4))
    _want(align_inv, "align_inv", torch.float64, (4, 4))
    _want(planes, "planes", torch.float64, (M, 24))
    _want(plabel, "plabel", torch.int32, (M,))
    _want(rows, "rows", torch.float64, (M, None))
    if rows.shape[1] < 6 or N < 1 or M < 1:
        raise ValueError("rows: at least 6 columns; at least one point and one frustum")
    ws = torch.empty(N, 6, dtype=torch.float64, device=points.device)
    if count is None:
        count = torch.empty(M, dtype=torch.int32, device=points.device)
    _want(count, "count", torch.int32, (M,))
    nat.call("ov3d_lift_frustum", points, int(points.dtype == torch.float64), N, labels, align,
             align_inv, planes, plabel, M, ws, rows, rows.shape[1], count, like=points)
    return count


def lift_image(depth, seg, lut, boxes, plabel, calib, rows, count=None):
    """ov3d_lift_image: fills columns 0-5 of the device rows (k, ld) -> count (k) int32"""
    nat.check(depth, "depth", None, 2)
    if depth.dtype not in (torch.int32, torch.float64):
        raise TypeError("depth: expected int32 or float64")
    H, W = depth.shape
    _want(seg, "seg", torch.int32, (H, W))
    _want(boxes, "boxes", torch.float64, (None, 6))
    k = boxes.shape[0]
    _want(plabel, "plabel", torch.int32, (k,))
    _want(calib, "calib", torch.float64, (13,))
    _want(rows, "rows", torch.float64, (k, None))
    if lut is not None:
        _want(lut, "lut", torch.int32, (None,))
    if rows.shape[1] < 6 or k < 1 or H < 1 or W < 1:
        raise ValueError("rows: at least 6 columns; at least one box and one pixel")
    if count is None:
        count = torch.empty(k, dtype=torch.int32, device=depth.device)
    _want(count, "count", torch.int32, (k,))
    nat.call("ov3d_lift_image", depth, int(depth.dtype == torch.float64), seg, lut,
             0 if lut is None else lut.numel(), H, W, boxes, plabel, k, calib, rows, rows.shape[1],
             count, like=depth)
    return count


def lift_views(depth, seg, lut, ignore_from, kinv, pose, align, slot_frame, slot_label, box_slot, rows,
               count=None):
    """ov3d_liftview_frames: fills columns 0-5 of the device rows (M, ld) from the slot of every
    box -> count (M) int32.  depth (F,H,W) float32 metres or uint16 raw millimetres; seg (F,H,W)
    int32; lut (n) int32 or None; ignore_from: without a lut, seg >= ignore_from reads as -100
    (None: off); kinv (3,3), pose (F,12) = R then t per frame, align (4,4), all float64."""
    nat.check(depth, "depth", None, 3)
    if depth.dtype not in (torch.float32, torch.uint16):
        raise TypeError("depth: expected float32 or uint16")
    F, H, W = depth.shape
    _want(seg, "seg", torch.int32, (F, H, W))
    _want(kinv, "kinv", torch.float64, (3, 3))
    _want(pose, "pose", torch.float64, (F, 12))
    _want(align, "align", torch.float64, (4, 4))
    _want(slot_frame, "slot_frame", torch.int32, (None,))
    S = slot_frame.shape[0]
    _want(slot_label, "slot_label", torch.int32, (S,))
    _want(box_slot, "box_slot", torch.int32, (None,))
    M = box_slot.shape[0]
    _want(rows, "rows", torch.float64, (M, None))
    if lut is not None:
        _want(lut, "lut", torch.int32, (None,))
    if rows.shape[1] < 6 or min(F, H, W, S, M) < 1 or H * W >= 2 ** 31:
        raise ValueError("rows: at least 6 columns; at least one pixel, slot and box; H * W < 2^31")
    if count is None:
        count = torch.empty(M, dtype=torch.int32, device=depth.device)
    _want(count, "count", torch.int32, (M,))
    slot_lohi = torch.empty(S, 6, dtype=torch.float64, device=depth.device)
    slot_count = torch.empty(S, dtype=torch.int32, device=depth.device)
    nat.call("ov3d_liftview_frames", depth, int(depth.dtype == torch.uint16), seg, lut,
             0 if lut is None else lut.numel(), 2 ** 31 if ignore_from is None else int(ignore_from),
             F, H, W, kinv, pose, align, slot_frame, slot_label, S, box_slot, M, slot_lohi, slot_count,
             rows, rows.shape[1], count, like=depth)
    return count


def result_buffer(M, device):
    """one allocation for everything the host reads back: -> (packed uint8, out (M,10) f64,
    count (M) int32, rank2 (M) int32), the last three views of the first"""
    packed = torch.empty(M * 88, dtype=torch.uint8, device=device)
    return (packed, packed[:M * 80].view(torch.float64).view(M, 10),
            packed[M * 80:M * 84].view(torch.int32), packed[M * 84:].view(torch.int32))


def chain_tail(rows, count, pool, out, rank2, nms=0.7, match=0.3, size_nms=0.0):
    """first NMS -> pool match -> size NMS on device tensors, no synchronisation.  rows (M,8):
    lifted min, max, score, label; count (M) int32 (0: nothing lifted); out, rank2: views of
    result_buffer.  -> the intermediate device tensors by name."""
    rank1, keep1 = nms_boxes(rows, nms, valid=count)
    m = match_pool(rows, rank1, pool, match, out=out)
    nms_boxes(m["rows"], size_nms, valid=m["win"], use_size_score=True, rank=rank2)
    return dict(m, rank1=rank1, keep1=keep1, rank2=rank2)


def _finish(packed, M, empty_width):
    """the single read-back, then compaction and pick order on the host"""
    host = packed.cpu().numpy()
    out = host[:M * 80].view(np.float64).reshape(M, 10)
    count = host[M * 80:M * 84].view(np.int32)
    rank2 = host[M * 84:].view(np.int32)
    if not (count > 0).any():
        return np.zeros((0, empty_width))
    kept = np.nonzero(rank2 >= 0)[0]
    if kept.size == 0:
        return np.zeros((0, 10))
    return np.ascontiguousarray(out[kept[np.argsort(rank2[kept])]])


def scannet_host_plan(intrinsic, poses, boxes2d):
    """edge filter and planes of every frame -> (planes (M,24), score_label (M,2), plabel (M))"""
    K = np.array(intrinsic, dtype=np.float32)
    K[0] /= 2.0
    K[1] /= 2.0
    planes, sl = [], []
    for pose, boxes in zip(poses, boxes2d):
        boxes = np.asarray(boxes)
        _check_boxes(boxes)
        boxes = edge_filter(boxes, IMAGE_DIMS)
        if boxes.shape[0] == 0:
            continue
        planes.append(frustum_planes(K, np.asarray(pose, dtype=np.float32), boxes))
        sl.append(boxes[:, 4:6].astype(np.float64))
    if not planes:
        return np.zeros((0, 24)), np.zeros((0, 2)), np.zeros(0, np.int32)
    sl = np.concatenate(sl)
    plabel = _box_labels(np.concatenate([np.zeros((len(sl), 4)), sl], 1))
    _check_counts(plabel)
    return np.concatenate(planes), sl, plabel


def lift_scannet_scan(points, labels, axis_align_matrix, intrinsic, poses, boxes2d, gss_pool,
                      nms=0.7, match=0.3, size_nms=0.0, device="cuda", return_lifted=False):
    """One ScanNet scan -> the array the reference saves: (k,10) float64
    [centre, size, label, score x volume, volume, area] in the size NMS's pick order, (0,10)
    when no pool box was labelled, (0,7) when nothing was lifted.  return_lifted: also the
    lifted rows (m,8) before the first NMS (a second read-back, for tests)."""
    pool = _pool(gss_pool)
    A = np.ascontiguousarray(np.asarray(axis_align_matrix, dtype=np.float64))
    if A.shape != (4, 4):
        raise ValueError("axis_align_matrix: expected (4,4)")
    Ainv = np.ascontiguousarray(np.linalg.inv(A))
    points = np.asarray(points)
    if points.ndim != 2 or points.shape[1] != 3 or len(poses) != len(boxes2d):
        raise ValueError("points: expected (N,3); one pose per frame of boxes")
    planes, sl, plabel = scannet_host_plan(intrinsic, poses, boxes2d)
    M = planes.shape[0]
    if M == 0 or points.shape[0] == 0:
        empty = np.zeros((0, 7))
        return (empty, np.zeros((0, 8))) if return_lifted else empty
    lab = np.array(labels, dtype=np.float64)
    lab[lab >= 18] = IGNORE_LABEL
    dev = torch.device(device)
    pts = torch.from_numpy(np.ascontiguousarray(points, dtype=np.float32 if points.dtype == np.float32
                                                else np.float64)).to(dev)
    rows_h = np.zeros((M, 8))
    rows_h[:, 6:] = sl
    rows = torch.from_numpy(rows_h).to(dev)
    up = lambda a: torch.from_numpy(a).to(dev)                      # noqa: E731
    packed, out, count, rank2 = result_buffer(M, dev)
    lift_frusta(pts, up(_int_labels(lab, _NEVER_POINT)), up(A), up(Ainv), up(planes), up(plabel),
                rows, count)
    chain_tail(rows, count, up(pool), out, rank2, nms, match, size_nms)
    final = _finish(packed, M, 7)
    if return_lifted:
        r, c = rows.cpu().numpy(), count.cpu().numpy()
        return final, r[c > 0]
    return final


def nyu40_lut():
    """nyu40 id -> class 0..17, -100 for every other id (ProjectionHelper.project_label)"""
    lut = np.full(int(NYU40IDS.max()) + 1, IGNORE_LABEL, np.int32)
    lut[NYU40IDS] = np.arange(len(NYU40IDS), dtype=np.int32)
    return lut


def single_host_plan(intrinsic, poses, boxes2d, image_dims=IMAGE_DIMS):
    """Host side of the single-view mode -> dict(kinv (3,3) f64, pose (F,12) f64 = R then t per
    frame, score_label (M,2), plabel (M) int32, slot_frame, slot_label (S) int32, box_slot (M)
    int32).  The intrinsic is halved in a copy; its inverse is numpy's, of the float32 matrix,
    widened.  The M boxes are those the edge filter leaves, frame by frame; a slot is a distinct
    (frame, int label) pair, sorted by frame, then label."""
    K = np.array(intrinsic, dtype=np.float32)
    P = np.asarray(poses, dtype=np.float32)
    if K.shape != (4, 4) or P.ndim != 3 or P.shape[1:] != (4, 4) or len(boxes2d) != P.shape[0]:
        raise ValueError("intrinsic: expected (4,4); poses: (F,4,4), one per frame of boxes")
    K[0] /= 2.0
    K[1] /= 2.0
    if not (np.isfinite(K).all() and np.isfinite(P).all()):
        raise ValueError("intrinsic and poses must be finite (the device's min / max skip a NaN)")
    kinv = np.linalg.inv(K[:3, :3]).astype(np.float64)
    if not np.isfinite(kinv).all():
        raise ValueError("intrinsic: its inverse is not finite")
    P = P.astype(np.float64)
    plan = dict(kinv=np.ascontiguousarray(kinv),
                pose=np.ascontiguousarray(np.concatenate([P[:, :3, :3].reshape(-1, 9), P[:, :3, 3]], 1)))
    frame, sl = [], []
    for f, boxes in enumerate(boxes2d):
        boxes = np.asarray(boxes)
        _check_boxes(boxes)
        boxes = edge_filter(boxes, image_dims)
        frame.append(np.full(boxes.shape[0], f, np.int32))
        sl.append(boxes[:, 4:6].astype(np.float64))
    sl = np.concatenate(sl) if sl else np.zeros((0, 2))
    frame = np.concatenate(frame) if frame else np.zeros(0, np.int32)
    plabel = _box_labels(np.concatenate([np.zeros((len(sl), 4)), sl], 1))
    _check_counts(plabel)
    pairs, box_slot = np.unique(np.stack([frame, plabel], 1), axis=0, return_inverse=True)
    return dict(plan, score_label=sl, plabel=plabel, slot_frame=np.ascontiguousarray(pairs[:, 0]),
                slot_label=np.ascontiguousarray(pairs[:, 1]), box_slot=box_slot.reshape(-1).astype(np.int32))


def _frames(x, name, dtypes):
    """(F,H,W) frames: a device tensor as it is, anything else as one numpy array"""
    if not isinstance(x, torch.Tensor):
        x = np.asarray(x)
    if x.ndim != 3 or (dtypes and x.dtype not in dtypes):
        raise ValueError(f"{name}: expected (F,H,W)" + (f" of {' or '.join(map(str, dtypes))}" if dtypes else "")
                         + f", got {x.dtype} {tuple(x.shape)}")
    return x


def lift_scannet_scan_single(depths, labels, axis_align_matrix, intrinsic, poses, boxes2d, gss_pool,
                             pseudo=True, nms=0.7, match=0.3, size_nms=0.0, device="cuda",
                             return_lifted=False):
    """One ScanNet scan in the reference's ``VIEW='single'`` mode -> what lift_scannet_scan
    returns.  Every 2D box lifts all pixels of its frame whose class equals its label (the
    rectangle is not consulted, as in the reference) through depth, pose and alignment.

    depths (F,H,W): float32 metres or uint16 raw millimetres (read as raw / 1000 in float32),
    numpy or a device tensor.  labels (F,H,W): numpy of any number type, or a device int32
    tensor such as the first result of open_vocab.classify_frames, which is used where it is.
    pseudo=True: class indices, values >= 18 ignored (negatives stay); pseudo=False: nyu40 ids,
    mapped to 0..17 on the device, every other id ignored.  The edge filter uses the frames' own
    (H, W).  Poses, intrinsic, alignment and host depths must be finite (ValueError); for a
    device float depth tensor that is the caller's precondition."""
    pool = _pool(gss_pool)
    A = np.ascontiguousarray(np.asarray(axis_align_matrix, dtype=np.float64))
    if A.shape != (4, 4) or not np.isfinite(A).all():
        raise ValueError("axis_align_matrix: expected a finite (4,4)")
    depths = _frames(depths, "depths", (torch.float32, torch.uint16) if isinstance(depths, torch.Tensor)
                     else (np.dtype(np.float32), np.dtype(np.uint16)))
    labels = _frames(labels, "labels", (torch.int32,) if isinstance(labels, torch.Tensor) else ())
    if tuple(depths.shape) != tuple(labels.shape) or depths.shape[0] != len(boxes2d):
        raise ValueError(f"depths {tuple(depths.shape)} and labels {tuple(labels.shape)}: expected the "
                         f"same (F,H,W) with one frame per list of boxes ({len(boxes2d)})")
    host_d, host_l = not isinstance(depths, torch.Tensor), not isinstance(labels, torch.Tensor)
    if host_d and depths.dtype.kind == "f" and not np.isfinite(depths).all():
        raise ValueError("depths must be finite (the device's min / max skip a NaN)")
    plan = single_host_plan(intrinsic, poses, boxes2d, tuple(depths.shape[1:]))
    M = plan["box_slot"].shape[0]
    if M == 0 or depths.shape[1] * depths.shape[2] == 0:
        empty = np.zeros((0, 7))
        return (empty, np.zeros((0, 8))) if return_lifted else empty
    dev = labels.device if not host_l else depths.device if not host_d else torch.device(device)
    slot_frame, pose = plan["slot_frame"], plan["pose"]
    if host_d and host_l:                                  # upload the frames that hold a slot only
        used, slot_frame = np.unique(slot_frame, return_inverse=True)
        depths, labels, pose = depths[used], labels[used], pose[used]
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
    if host_d:
        depths = up(depths)
    if host_l:
        labels = up(_int_labels(labels, _NEVER_POINT))
    rows_h = np.zeros((M, 8))
    rows_h[:, 6:] = plan["score_label"]
    rows = up(rows_h)
    packed, out, count, rank2 = result_buffer(M, dev)
    lift_views(depths.contiguous(), labels.contiguous(), None if pseudo else up(nyu40_lut()),
               PSEUDO_IGNORE_FROM if pseudo else None, up(plan["kinv"]), up(pose), up(A),
               up(slot_frame.reshape(-1).astype(np.int32)), up(plan["slot_label"]), up(plan["box_slot"]),
               rows, count)
    chain_tail(rows, count, up(pool), out, rank2, nms, match, size_nms)
    final = _finish(packed, M, 7)
    if return_lifted:
        r, c = rows.cpu().numpy(), count.cpu().numpy()
        return final, r[c > 0]
    return final


def lift_sunrgbd_scan(depth, seg, Rtilt, K, boxes2d, gss_pool, nms=0.7, match=0.3, size_nms=0.0,
                      device="cuda", return_lifted=False):
    """One SUN RGB-D image -> the array the reference saves ((0,8) when nothing was lifted).
    depth (H,W) raw integers (or floats), seg (H,W) labels (already + 1 for pseudo labels)."""
    pool = _pool(gss_pool)
    depth, seg = np.asarray(depth), np.asarray(seg)
    boxes = np.asarray(boxes2d)
    _check_boxes(boxes)
    if depth.ndim != 2 or depth.shape != seg.shape:
        raise ValueError("depth and seg: expected the same (H,W)")
    boxes = np.ascontiguousarray(edge_filter(boxes, seg.shape).astype(np.float64))
    M = boxes.shape[0]
    if M == 0 or depth.size == 0:
        empty = np.zeros((0, 8))
        return (empty, empty) if return_lifted else empty
    plabel = _box_labels(boxes)
    _check_counts(plabel)
    Rtilt, K = np.asarray(Rtilt, dtype=np.float64), np.asarray(K, dtype=np.float64)
    calib = np.concatenate([[K[0, 0], K[1, 1], K[0, 2], K[1, 2]], Rtilt.reshape(-1)])
    lut = np.full(max(SUNRGBD37IDS) + 1, IGNORE_LABEL, np.int32)
    lut[list(SUNRGBD37IDS)] = np.arange(len(SUNRGBD37IDS), dtype=np.int32)
    dev = torch.device(device)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
    d = depth.astype(np.int32) if depth.dtype.kind in "iu" else depth.astype(np.float64)
    rows_h = np.zeros((M, 8))
    rows_h[:, 6:] = boxes[:, 4:6]
    rows = up(rows_h)
    packed, out, count, rank2 = result_buffer(M, dev)
    lift_image(up(d), up(_int_labels(seg, _NEVER_POINT)), up(lut), up(boxes), up(plabel), up(calib),
               rows, count)
    chain_tail(rows, count, up(pool), out, rank2, nms, match, size_nms)
    final = _finish(packed, M, 8)
    if return_lifted:
        r, c = rows.cpu().numpy(), count.cpu().numpy()
        return final, r[c > 0]
    return final


def to_training_format(boxes):
    """adjust_format.py: columns 0-6 with the class index mapped to its nyu40 id, the layout
    ScannetDetectionDataset(use_pbox=True) reads"""
    box = np.array(boxes[:, 0:7])
    if box.shape[1] != 7:
        raise ValueError(f"expected rows of at least 7 columns, got {boxes.shape}")
    box[:, -1] = NYU40IDS[box[:, -1].astype(np.int64)]
    return box


def read_pose(path):
    """(4,4) float32 from four lines of blank-separated numbers"""
    with open(path) as f:
        lines = f.read().splitlines()
    if len(lines) != 4:
        raise ValueError(f"{path}: expected 4 lines")
    return np.asarray([ln.split(" ")[:4] for ln in lines]).astype(np.float32)


def read_alignment(path):
    with open(path) as f:
        for line in f:
            if "axisAlignment" in line:
                vals = [float(x) for x in line.split("=", 1)[1].split()]
                return np.array(vals).reshape(4, 4)
    raise ValueError(f"{path}: no axisAlignment line")


class ScannetBoxLifter:
    """File-level driver: numpy reads only (allow_pickle off), one ``<scan>_bbox.npy`` per scan.

    label_dir/<scan>.npy            (N,4) aligned xyz + LSeg class
    frames_dir/<scan>/pose/<id>.txt, frames_dir/<scan>/intrinsic_depth.txt
    boxes2d_dir/<scan>/color/<id>.npy   (k,6) x, y, w, h, score, label; the frame ids come from
                                        this listing, sorted as the reference sorts its frames
    gss_dir/<scan>_prop.npy         (P,7) proposals
    scans_dir/<scan>/<scan>.txt     the axisAlignment line

    view="single" (the reference's ``VIEW='single'``; lift_scannet_scan_single) reads instead
    of the vertex file, and decodes PNGs with PIL, imported only then:
    label_dir/<scan>.npy            the per-frame class maps open_vocab.save_frame_labels writes:
                                    a pickled dict {int(frame id): (H,W) map}, because that is the
                                    file the reference's single-view branch loads (allow_pickle
                                    on: open files you trust only); used with pseudo=True
    frames_dir/<scan>/depth/<id>.png         16-bit depth in millimetres
    frames_dir/<scan>/label-mapped/<id>.png  nyu40 ids, read in place of the dict file with
                                             pseudo=False (the reference's PSEUDO_FLAG = False)
    """

    def __init__(self, label_dir, frames_dir, boxes2d_dir, gss_dir, scans_dir, out_dir, nms=0.7,
                 match=0.3, size_nms=0.0, device="cuda", view="multi", pseudo=True):
        if view not in ("multi", "single"):
            raise ValueError(f"view: 'multi' or 'single', got {view!r}")
        self.label_dir, self.frames_dir, self.boxes2d_dir = label_dir, frames_dir, boxes2d_dir
        self.gss_dir, self.scans_dir, self.out_dir = gss_dir, scans_dir, out_dir
        self.nms, self.match, self.size_nms, self.device = nms, match, size_nms, device
        self.view, self.pseudo = view, pseudo

    def _lift_one_single(self, scan, frames, box_dir):
        from PIL import Image

        def png(kind, f):
            with Image.open(os.path.join(self.frames_dir, scan, kind, f + ".png")) as im:
                return np.array(im)
        depths = np.stack([png("depth", f) for f in frames])
        if depths.dtype != np.uint16:
            if depths.dtype.kind not in "iu" or depths.min() < 0 or depths.max() >= 2 ** 16:
                raise ValueError(f"{scan}: depth PNGs are not 16-bit")
            depths = depths.astype(np.uint16)
        if self.pseudo:
            from . import open_vocab
            labels = open_vocab.load_frame_labels(os.path.join(self.label_dir, scan + ".npy"), frames)
        else:
            labels = np.stack([png("label-mapped", f) for f in frames])
        frame_dir = os.path.join(self.frames_dir, scan)
        return lift_scannet_scan_single(
            depths, labels, read_alignment(os.path.join(self.scans_dir, scan, scan + ".txt")),
            read_pose(os.path.join(frame_dir, "intrinsic_depth.txt")),
            [read_pose(os.path.join(frame_dir, "pose", f + ".txt")) for f in frames],
            [np.load(os.path.join(box_dir, f + ".npy"), allow_pickle=False) for f in frames],
            np.load(os.path.join(self.gss_dir, scan + "_prop.npy"), allow_pickle=False),
            self.pseudo, self.nms, self.match, self.size_nms, self.device)

    def lift_one(self, scan):
        box_dir = os.path.join(self.boxes2d_dir, scan, "color")
        frames = [n.split(".")[0] for n in sorted(os.listdir(box_dir))]
        if self.view == "single":
            out = self._lift_one_single(scan, frames, box_dir)
            os.makedirs(self.out_dir, exist_ok=True)
            np.save(os.path.join(self.out_dir, scan + "_bbox.npy"), out)
            return out.shape[0]
        sem = np.load(os.path.join(self.label_dir, scan + ".npy"), allow_pickle=False)
        frame_dir = os.path.join(self.frames_dir, scan)
        out = lift_scannet_scan(
            sem[:, :3], sem[:, 3], read_alignment(os.path.join(self.scans_dir, scan, scan + ".txt")),
            read_pose(os.path.join(frame_dir, "intrinsic_depth.txt")),
            [read_pose(os.path.join(frame_dir, "pose", f + ".txt")) for f in frames],
            [np.load(os.path.join(box_dir, f + ".npy"), allow_pickle=False) for f in frames],
            np.load(os.path.join(self.gss_dir, scan + "_prop.npy"), allow_pickle=False),
            self.nms, self.match, self.size_nms, self.device)
        os.makedirs(self.out_dir, exist_ok=True)
        np.save(os.path.join(self.out_dir, scan + "_bbox.npy"), out)
        return out.shape[0]

    def lift(self, scan_names):
        """-> the number of boxes written per scan"""
        return [self.lift_one(s) for s in scan_names]
