"""3D NMS on the ov3d HIP kernel (replaces reference utils/nms.py:79-162).

* ``nms_3d_faster_samecls(boxes, overlap_threshold, old_type=False)`` and
  ``nms_3d_faster(...)``: same signature and return value (pick list, in pick
  order) as the reference numpy functions for one scene;
* ``nms_2d_faster(boxes, overlap_threshold, old_type=False)``: the reference's 2D NMS
  (utils/nms.py:43-76) on the same kernel, each row lifted to a box of unit depth;
* ``nms3d_batched``: all scenes of a batch in one launch, straight from device
  tensors -> (B, K) keep mask, the ``pred_mask`` of ap_calculator.py:153-190.
Float64 arithmetic in the reference's evaluation order; score ties break
towards the larger index (np.argsort(kind="stable") read from the back).
Up to ``MAX_K`` = 2048 boxes per scene (the encoders emit at most 2048 points, and the
queries are a subset of them); ``large_kernels(1)`` runs the kernels for the large shapes
at every shape.
"""
import numpy as np
import torch

from . import _native as nat

MAX_K = 2048


def large_kernels(on=-1):
    """ov3d_eval_large_kernels: 1 = ov3d_nms3d and ov3d_ap_match use their large-shape kernels
    at every shape, 0 = dispatch on the shape (default), -1 = only query.  -> previous setting."""
    return int(nat.load().ov3d_eval_large_kernels(int(on)))


def nms3d_batched(boxes, overlap_threshold, old_type=False, samecls=True, valid=None):
    """boxes (B,K,7|8) float64 cuda, valid (B,K) bool/uint8 or None -> keep (B,K) uint8."""
    boxes = nat.check(boxes.to(torch.float64).contiguous(), "boxes", torch.float64, 3)
    B, K, stride = boxes.shape
    if K > MAX_K:
        raise ValueError(f"nms3d supports K <= {MAX_K} boxes per scene")
    v = None
    if valid is not None:
        v = nat.check(valid.to(device=boxes.device, dtype=torch.uint8).contiguous(), "valid",
                      torch.uint8, 2)
    keep = torch.empty((B, K), dtype=torch.uint8, device=boxes.device)
    nat.call("ov3d_nms3d", boxes, v, B, K, stride, float(overlap_threshold), int(bool(old_type)),
             int(bool(samecls)), keep, like=boxes)
    return keep


def nms_boxes_from_corners(corners, obj_prob, sem_cls=None):
    """(B,K,8,3) corners, (B,K) objectness, (B,K) class -> (B,K,8) float64 NMS table
    [xmin,ymin,zmin,xmax,ymax,zmax,obj,cls] (ap_calculator.py:153-187)."""
    c = nat.check(corners.detach().float().contiguous(), "corners", torch.float32, 4)
    B, K = c.shape[:2]
    o = nat.check(obj_prob.detach().float().contiguous(), "obj", torch.float32, 2)
    cl = None
    if sem_cls is not None:
        cl = nat.check(sem_cls.to(torch.int64).contiguous(), "cls", torch.int64, 2)
    out = torch.empty((B, K, 8), dtype=torch.float64, device=c.device)
    nat.call("ov3d_nms_boxes_from_corners", c, o, cl, B, K, out, like=c)
    return out


def boxes2d_as_3d(boxes2d):
    """(..., >=5) rows (x1, y1, x2, y2, score) -> (..., 7) rows [x1, 0, y1, x2, 1, y2, score]:
    the product with the unit extent is exact, so volume = area and intersection = w * h"""
    out = boxes2d.new_zeros(boxes2d.shape[:-1] + (7,))
    out[..., 0] = boxes2d[..., 0]
    out[..., 2] = boxes2d[..., 1]
    out[..., 3] = boxes2d[..., 2]
    out[..., 4] = 1.0
    out[..., 5] = boxes2d[..., 3]
    out[..., 6] = boxes2d[..., 4]
    return out


def _single(boxes, thr, old_type, samecls, two_d=False):
    dev = torch.device("cuda", torch.cuda.current_device())
    b = torch.as_tensor(np.ascontiguousarray(boxes, dtype=np.float64), device=dev)[None]
    if two_d:
        b = boxes2d_as_3d(b)
    keep = nms3d_batched(b, thr, old_type=old_type, samecls=samecls)[0]
    score = b[0, :, 6]
    idx = torch.nonzero(keep).flatten()
    # pick order = descending score, ties -> larger index first
    order = sorted(idx.tolist(), key=lambda i: (-float(score[i]), -i))
    return order


def nms_3d_faster(boxes, overlap_threshold, old_type=False):
    return _single(boxes, overlap_threshold, old_type, samecls=False)


def nms_3d_faster_samecls(boxes, overlap_threshold, old_type=False):
    return _single(boxes, overlap_threshold, old_type, samecls=True)


def nms_2d_faster(boxes, overlap_threshold, old_type=False):
    return _single(boxes, overlap_threshold, old_type, samecls=False, two_d=True)
