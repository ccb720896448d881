"""numpy restatement of the two entries of include/ov3d_poollabel.h, in the header's order, and
of the device halves of ov3d_amd.pool_label / ov3d_amd.label_assess built on them.
tests/test_pool_label_cpu.py holds it to the reference's recorded results
(tests/golden/pool_label.npz); tests/test_pool_label_gpu.py holds the kernels to it."""
import numpy as np


def vote(pts, labels, pt_off, boxes, box_off, min_label, C):
    """ov3d_poollabel_vote: pts (N, ld >= 3) f32 / f64, labels (N) uint8, boxes (P, 6) f64 closed
    bounds, pt_off / box_off (S+1) -> counts (P, C) int32, mode (P) int32"""
    P = len(boxes)
    counts = np.zeros((P, C), np.int32)
    for s in range(len(pt_off) - 1):
        xyz = pts[pt_off[s]: pt_off[s + 1], :3].astype(np.float64)      # exact for float32
        lab = labels[pt_off[s]: pt_off[s + 1]].astype(np.int64)
        votes = (lab >= min_label) & (lab < C)
        xyz, lab = xyz[votes], lab[votes]
        for b in range(box_off[s], box_off[s + 1]):
            with np.errstate(invalid="ignore"):
                inside = ((xyz >= boxes[b, :3]) & (xyz <= boxes[b, 3:6])).all(1)
            counts[b] = np.bincount(lab[inside], minlength=C)
    mode = np.where(counts.max(1, initial=0) > 0, counts.argmax(1), -1).astype(np.int32)
    return counts, mode


def confusion(gt, pseudo, frame_off, gt_map, K):
    """ov3d_poollabel_confusion: gt, pseudo (F, HW) uint8, frame_off (S+1), gt_map (256) uint8 ->
    conf (S, K+1, K+1) int64"""
    S = len(frame_off) - 1
    conf = np.zeros((S, K + 1, K + 1), np.int64)
    for s in range(S):
        g = np.minimum(gt_map[gt[frame_off[s]: frame_off[s + 1]]].astype(np.int64), K)
        p = np.minimum(pseudo[frame_off[s]: frame_off[s + 1]].astype(np.int64), K)
        conf[s] = np.bincount((g * (K + 1) + p).reshape(-1), minlength=(K + 1) ** 2).reshape(K + 1, K + 1)
    return conf


def vote_group(scans, device=None):
    """stands in for ov3d_amd.pool_label.vote_group (host tests)"""
    off = lambda sizes: np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)     # noqa: E731
    pt_off, box_off = off([len(s[0]) for s in scans]), off([len(s[2]) for s in scans])
    if box_off[-1] == 0:
        return [np.zeros(0, np.int32) for _ in scans]
    dt = np.float32 if all(s[0].dtype == np.float32 for s in scans) else np.float64
    _, mode = vote(np.concatenate([s[0].astype(dt) for s in scans]), np.concatenate([s[1] for s in scans]),
                   pt_off, np.concatenate([s[2][:, :6] for s in scans]), box_off, 3, 64)
    return [mode[box_off[i]: box_off[i + 1]] for i in range(len(scans))]


def group(frames, device=None):
    """stands in for ov3d_amd.label_assess._group (host tests)"""
    from ov3d_amd.label_assess import GT_MAP
    off = np.concatenate([[0], np.cumsum([len(g) for g, _ in frames])])
    return confusion(np.concatenate([g for g, _ in frames]), np.concatenate([p for _, p in frames]), off,
                     GT_MAP, 18)
