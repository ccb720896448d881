"""numpy restatement of the pseudo-box lifting chain (ov3d_amd.lift_boxes, csrc/lift.hip):
frustum planes, the two lifts, the tools' class-wise NMS, the pool match (as the reference's
sequential loop and in closed form) and the labelled pool rows.  Elementwise float64 with every
sum written out in the order include/ov3d_lift.h states, so the device results are expected
bit for bit; tests/test_lift_ref_cpu.py holds it to the reference's recorded results
(tests/golden/lift_boxes.npz)."""
import numpy as np

IGNORE = -100
PLANE_CORNERS = ((3, 1, 0), (2, 5, 1), (3, 6, 2), (0, 7, 3), (1, 4, 0), (6, 4, 5))
SUN_IDS = (36, 4, 10, 29, 5, 12, 14, 8, 17, 35, 32, 18, 34, 6, 7, 25, 33)
NYU40 = np.array([3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14, 16, 24, 28, 33, 34, 36, 39])


def not_on_edge(boxes, dims):
    if len(boxes) == 0:
        return boxes
    ok = [b[0] != 0 and b[1] != 0 and b[0] + b[2] != dims[1] and b[1] + b[3] != dims[0] for b in boxes]
    return boxes[np.array(ok, dtype=bool)]


def planes_of(intrinsic_half, pose, box, near=0.1, far=10.0):
    """(24,) normals, corner 2, corner 4 of one 2D box (numpy's own inv / matmul / cross)"""
    x, y, w, h = box[:4]
    u = np.array([x, x + w, x + w, x] * 2)
    v = np.array([y, y, y + h, y + h] * 2)
    d = np.array([near] * 4 + [far] * 4)
    inv = np.linalg.inv(intrinsic_half[:3, :3])
    with np.errstate(all="ignore"):
        cam = np.ones((8, 4))
        cam[:, :3] = (inv.dot(np.stack([u, v, np.ones_like(u)], 1).T) * d).T
        c = (pose @ cam[:, :, None])[:, :3, 0]
        n = np.stack([np.cross(c[a] - c[o], c[b] - c[o]) for a, b, o in PLANE_CORNERS])
        n = n / np.sum(n ** 2, axis=-1, keepdims=True)
    return np.concatenate([n.reshape(-1), c[2], c[4]])


def scannet_plan(intrinsic, poses, boxes2d, dims=(240, 320)):
    """-> planes (M,24), score_label (M,2), box label (M) int64 after the edge filter"""
    K = np.array(intrinsic, dtype=np.float32)
    K[:2] /= 2.0
    planes, sl = [], []
    for pose, boxes in zip(poses, boxes2d):
        for b in not_on_edge(np.asarray(boxes), dims):
            planes.append(planes_of(K, np.asarray(pose, np.float32), b))
            sl.append(np.asarray(b[4:6], np.float64))
    if not planes:
        return np.zeros((0, 24)), np.zeros((0, 2)), np.zeros(0, np.int64)
    sl = np.stack(sl)
    return np.stack(planes), sl, np.trunc(sl[:, 1]).astype(np.int64)


def affine(m, p):
    """rows ((m0 x + m1 y) + m2 z) + m3 of a (4,4) matrix over points (N,3)"""
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    return np.stack([((m[i, 0] * x + m[i, 1] * y) + m[i, 2] * z) + m[i, 3] for i in range(3)], 1)


def dot3(a, n):
    return (a[:, 0] * n[0] + a[:, 1] * n[1]) + a[:, 2] * n[2]


def lift_frusta(points, labels, align, align_inv, planes, plabel):
    """-> lohi (M,6) (zeros where nothing was lifted), count (M)"""
    p = np.asarray(points).astype(np.float64)
    orig = affine(align_inv, p)
    again = affine(align, orig)
    M = len(planes)
    lohi, count = np.zeros((M, 6)), np.zeros(M, np.int32)
    with np.errstate(all="ignore"):
        for m in range(M):
            n = planes[m, :18].reshape(6, 3)
            v, w = orig - planes[m, 18:21], orig - planes[m, 21:24]
            v = v / ((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])[:, None]
            w = w / ((w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1]) + w[:, 2] * w[:, 2])[:, None]
            inside = labels == plabel[m]
            for k in range(3):
                inside = inside & (dot3(v, n[k]) < 0) & (dot3(w, n[3 + k]) < 0)
            count[m] = inside.sum()
            if count[m]:
                lohi[m] = np.concatenate([again[inside].min(0), again[inside].max(0)])
    return lohi, count


def scannet_labels(labels):
    lab = np.array(labels, dtype=np.float64)
    lab[lab >= 18] = IGNORE
    return lab


def sun_classes(seg):
    out = np.full(seg.shape, IGNORE, np.int64)
    for i, c in enumerate(SUN_IDS):
        out[seg == c] = i
    return out


def lift_image(depth, cls, boxes, plabel, Rtilt, K):
    """-> lohi (k,6), count (k); cls: per-pixel class (after the id table)"""
    H, W = cls.shape
    v, u = np.indices((H, W))
    fu, fv, cu, cv = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    k = len(boxes)
    lohi, count = np.zeros((k, 6)), np.zeros(k, np.int32)
    for b in range(k):
        x, y, w, h = (float(t) for t in boxes[b, :4])
        m = (u >= x) & (u <= x + w) & (v >= y) & (v <= y + h) & (cls == plabel[b])
        count[b] = m.sum()
        if not count[b]:
            continue
        d = depth[m].astype(np.float64)
        p0 = ((u[m] - cu) * d) / fu
        p2 = -(((v[m] - cv) * d) / fv)
        pts = np.stack([(Rtilt[i, 0] * p0 + Rtilt[i, 1] * d) + Rtilt[i, 2] * p2 for i in range(3)], 1)
        lohi[b] = np.concatenate([pts.min(0), pts.max(0)])
    return lohi, count


def nms(boxes, thresh, valid=None, use_size_score=False):
    """-> rows in pick order (indices into boxes).  Descending key, equal keys: higher row first."""
    K = len(boxes)
    ok = np.ones(K, bool) if valid is None else np.asarray(valid) != 0
    key = boxes[:, 6] * boxes[:, 8] if use_size_score else boxes[:, 6]
    idx = np.nonzero(ok)[0]
    live = list(idx[np.lexsort((idx, key[idx]))][::-1])
    vol = ((boxes[:, 3] - boxes[:, 0]) * (boxes[:, 4] - boxes[:, 1])) * (boxes[:, 5] - boxes[:, 2]) + 1e-8
    picks = []
    with np.errstate(all="ignore"):
        while live:
            i = live.pop(0)
            picks.append(i)
            rest = np.array(live, dtype=np.int64)
            if rest.size == 0:
                break
            side = [np.maximum(0, np.minimum(boxes[i, 3 + a], boxes[rest, 3 + a])
                               - np.maximum(boxes[i, a], boxes[rest, a])) for a in range(3)]
            inter = (side[0] * side[1]) * side[2]
            o = inter / ((vol[i] + vol[rest]) - inter)
            o = o * (boxes[i, 7] == boxes[rest, 7])
            live = [j for j, gone in zip(live, o > thresh) if not gone]
    return np.array(picks, dtype=np.int64)


def ranks(picks, K):
    r = np.full(K, -1, np.int32)
    r[picks] = np.arange(len(picks), dtype=np.int32)
    return r


def pool_vv(pool):
    lo = pool[:, :3] - pool[:, 3:6] / 2
    return np.concatenate([lo, pool[:, 3:6] + lo], 1)


def iou_to_pool(box, vv):
    vq = ((box[3] - box[0]) * (box[4] - box[1])) * (box[5] - box[2])
    vk = ((vv[:, 3] - vv[:, 0]) * (vv[:, 4] - vv[:, 1])) * (vv[:, 5] - vv[:, 2])
    side = [np.maximum(np.minimum(box[3 + a], vv[:, 3 + a]) - np.maximum(box[a], vv[:, a]), 0) for a in range(3)]
    inter = (side[0] * side[1]) * side[2]
    return inter / (((vq + vk) - inter) + 1e-5)


def match_loop(boxes, picks, vv, match):
    """the sequential update: -> label (P) (-100: none), score (P)"""
    label, score = np.full(len(vv), float(IGNORE)), np.zeros(len(vv))
    for b in picks:
        iou = iou_to_pool(boxes[b], vv)
        if iou.max() < match:
            continue
        j = int(np.argmax(iou))
        if boxes[b, 6] > score[j]:
            label[j], score[j] = boxes[b, 7], boxes[b, 6]
    return label, score


def match_closed(boxes, picks, vv, match):
    """closed form: -> amax (M), maxiou (M), owner (P) (the winning row, -1: none)"""
    M = len(boxes)
    amax, maxiou = np.full(M, -1, np.int32), np.zeros(M)
    owner = np.full(len(vv), -1, np.int64)
    for b in picks:
        iou = iou_to_pool(boxes[b], vv)
        amax[b], maxiou[b] = int(np.argmax(iou)), iou.max()
        if not maxiou[b] < match and boxes[b, 6] > 0 and owner[amax[b]] < 0:
            owner[amax[b]] = b
    return amax, maxiou, owner


def pool_rows(boxes, owner, vv):
    """per lifted row (M): win, rows (M,10) for the size NMS, out (M,10) final layout"""
    M = len(boxes)
    win, rows, out = np.zeros(M, np.int32), np.zeros((M, 10)), np.zeros((M, 10))
    for j in np.nonzero(owner >= 0)[0]:
        b = owner[j]
        s = vv[j, 3:6] - vv[j, :3]
        vol = (s[0] * s[1]) * s[2]
        area = 2 * ((s[0] * s[2] + s[1] * s[0]) + s[2] * s[1])
        win[b] = 1
        rows[b] = np.concatenate([vv[j], [boxes[b, 6], boxes[b, 7], vol, area]])
        out[b] = np.concatenate([vv[j, :3] + s / 2, s, [boxes[b, 7], boxes[b, 6] * vol, vol, area]])
    return win, rows, out


def tail(lohi, count, sl, pool, nms_t=0.7, match=0.3, size_t=0.0, empty_width=8):
    """lifted rows -> the saved array; also the lifted rows before the first NMS"""
    boxes = np.concatenate([lohi, sl], 1)
    lifted = boxes[count > 0]
    if len(lifted) == 0:
        return np.zeros((0, empty_width)), lifted
    vv = pool_vv(np.asarray(pool, np.float64))
    picks = nms(boxes, nms_t, valid=count)
    _, _, owner = match_closed(boxes, picks, vv, match)
    win, rows, out = pool_rows(boxes, owner, vv)
    if not win.any():
        return np.zeros((0, 10)), lifted
    return out[nms(rows, size_t, valid=win, use_size_score=True)], lifted


def scannet_scan(points, labels, axis_align_matrix, intrinsic, poses, boxes2d, gss_pool, nms_t=0.7,
                 match=0.3, size_t=0.0):
    align, pool = axis_align_matrix, gss_pool
    planes, sl, plabel = scannet_plan(intrinsic, poses, boxes2d)
    if len(planes) == 0:
        return np.zeros((0, 7)), np.zeros((0, 8))
    A = np.asarray(align, np.float64)
    lohi, count = lift_frusta(points, scannet_labels(labels), A, np.linalg.inv(A), planes, plabel)
    return tail(lohi, count, sl, pool, nms_t, match, size_t, 7)


def sun_scan(depth, seg, Rtilt, K, boxes2d, gss_pool, nms_t=0.7, match=0.3, size_t=0.0):
    pool = gss_pool
    boxes = not_on_edge(np.asarray(boxes2d), seg.shape).astype(np.float64)
    if len(boxes) == 0:
        return np.zeros((0, 8)), np.zeros((0, 8))
    plabel = np.trunc(boxes[:, 5]).astype(np.int64)
    lohi, count = lift_image(depth, sun_classes(seg), boxes, plabel, Rtilt, K)
    return tail(lohi, count, boxes[:, 4:6], pool, nms_t, match, size_t, 8)


def training_format(boxes):
    out = np.array(boxes[:, :7])
    out[:, 6] = NYU40[out[:, 6].astype(np.int64)]
    return out
