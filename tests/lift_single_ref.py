"""numpy restatement of the single-view lift (ov3d_amd.lift_boxes.lift_scannet_scan_single,
csrc/liftview.hip): elementwise float64 with every sum written out in the order
include/ov3d_liftview.h states, so the device results are expected bit for bit; NMS, match and
rows are lift_ref's.  tests/test_lift_single_cpu.py holds it to the reference's recorded
results (tests/golden/lift_single.npz)."""
import numpy as np

import lift_ref as R

IGNORE = -100
IGNORE_FROM = 18


def classes(seg, lut=None, ignore_from=None):
    """per-pixel class of an integer map: through the table, or seg with seg >= ignore_from
    ignored"""
    seg = np.asarray(seg).astype(np.int64)
    if lut is not None:
        ok = (seg >= 0) & (seg < len(lut))
        return np.where(ok, np.asarray(lut, np.int64)[np.where(ok, seg, 0)], IGNORE)
    return seg if ignore_from is None else np.where(seg >= ignore_from, IGNORE, seg)


def nyu40_lut():
    lut = np.full(int(R.NYU40.max()) + 1, IGNORE, np.int64)
    lut[R.NYU40] = np.arange(len(R.NYU40))
    return lut


def metres(depth):
    """uint16 raw millimetres -> float32 metres as the reference's load_depth; float32 as is"""
    depth = np.asarray(depth)
    return depth.astype(np.float32) / 1000.0 if depth.dtype == np.uint16 else depth


def lift_slots(depth, cls, kinv, pose, A, slot_frame, slot_label):
    """depth (F,H,W) float32 metres, cls (F,H,W) classes, kinv (3,3), pose (F,12) = R then t,
    A (4,4), all float64 -> lohi (S,6) (zeros where no pixel), count (S) int32"""
    S = len(slot_frame)
    lohi, count = np.zeros((S, 6)), np.zeros(S, np.int32)
    for s in range(S):
        f = int(slot_frame[s])
        if not 0 <= f < len(depth):
            continue
        v, u = np.nonzero(cls[f] == slot_label[s])
        count[s] = len(u)
        if not len(u):
            continue
        d = depth[f][v, u].astype(np.float64)
        ud, vd = u.astype(np.float64), v.astype(np.float64)
        Rm, t = pose[f, :9].reshape(3, 3), pose[f, 9:]
        c = [((kinv[i, 0] * ud + kinv[i, 1] * vd) + kinv[i, 2]) * d for i in range(3)]
        w = [((c[0] * Rm[i, 0] + c[1] * Rm[i, 1]) + c[2] * Rm[i, 2]) + t[i] for i in range(3)]
        a = np.stack([((A[i, 0] * w[0] + A[i, 1] * w[1]) + A[i, 2] * w[2]) + A[i, 3] for i in range(3)], 1)
        lohi[s] = np.concatenate([a.min(0), a.max(0)])
    return lohi, count


def plan(intrinsic, poses, boxes2d, dims):
    """-> kinv, pose (F,12), score_label (M,2), frame (M), label (M) after the edge filter"""
    K = np.array(intrinsic, dtype=np.float32)
    K[:2] /= 2.0
    kinv = np.linalg.inv(K[:3, :3]).astype(np.float64)
    P = np.asarray(poses, np.float32).astype(np.float64)
    pose = np.concatenate([P[:, :3, :3].reshape(-1, 9), P[:, :3, 3]], 1)
    frame, sl = [], []
    for f, boxes in enumerate(boxes2d):
        for b in R.not_on_edge(np.asarray(boxes), dims):
            frame.append(f)
            sl.append(np.asarray(b[4:6], np.float64))
    sl = np.stack(sl) if sl else np.zeros((0, 2))
    return kinv, pose, sl, np.array(frame, np.int64), np.trunc(sl[:, 1]).astype(np.int64)


def scan(depths, labels, axis_align_matrix, intrinsic, poses, boxes2d, gss_pool, pseudo=True,
         nms_t=0.7, match=0.3, size_t=0.0):
    """-> the saved array, the lifted rows before the first NMS.  Every box is its own slot
    here; the product's deduplication must not change a byte."""
    depth = metres(depths)
    kinv, pose, sl, frame, label = plan(intrinsic, poses, boxes2d, depth.shape[1:])
    if len(sl) == 0:
        return np.zeros((0, 7)), np.zeros((0, 8))
    cls = classes(labels, ignore_from=IGNORE_FROM) if pseudo else classes(labels, lut=nyu40_lut())
    lohi, count = lift_slots(depth, cls, kinv, pose, np.asarray(axis_align_matrix, np.float64), frame, label)
    return R.tail(lohi, count, sl, gss_pool, nms_t, match, size_t, 7)
