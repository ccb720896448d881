"""utils/label_formatter.py restated in plain numpy (no torch, no scipy): step / compute /
gen_pseudo of the reference's LabelFormatter, and the label vote (counts, mode) of
ov3d_box_points_count kind 1.  tests/test_pseudo_label_cpu.py holds it to the reference's
recorded arrays (tests/golden/pseudo_label.npz); it is the checker at every other shape."""
import numpy as np

IGNORE_LABEL = -100


def step_rows(outputs, scan_idx):
    """label_formatter.py:99-105 -> (B * Q, 10) float32: centre, size, label, score,
    objectness, scan index; torch.max's index is the first maximum"""
    prob = np.asarray(outputs["sem_cls_prob"])
    B, Q, _ = prob.shape
    f = np.float32
    tail = np.stack([prob.argmax(-1).astype(f), prob.max(-1).astype(f),
                     np.asarray(outputs["objectness_prob"]).astype(f),
                     np.repeat(np.asarray(scan_idx)[:, None], Q, 1).astype(f)], -1)
    return np.concatenate([np.asarray(outputs["center_unnormalized"]).astype(f),
                           np.asarray(outputs["size_unnormalized"]).astype(f), tail], -1).reshape(B * Q, 10)


def compute(rows, th_s, th_o, num_classes=18):
    """label_formatter.py:121-132: class-major, step order within a class; the thresholds are
    compared in the array's float32"""
    rows = np.concatenate(rows, 0)
    out = []
    for label in range(num_classes):
        r = rows[rows[:, 6] == label]
        out.append(r[np.logical_and(r[:, 7] >= np.float32(th_s), r[:, 8] >= np.float32(th_o))])
    return np.concatenate(out, 0)


def crop_pc(pc, box):
    """label_formatter.py:183-188: box is a float32 row, pc keeps its own dtype"""
    return np.all(pc >= box[0:3] - box[3:6] / 2, -1) & np.all(pc <= box[0:3] + box[3:6] / 2, -1)


def gen_pseudo(pseudo_boxes, idx, raw, num_classes=18):
    """label_formatter.py:134-166 for scan `idx` with file contents `raw` (n, 4) -> the array
    the reference saves: float64 (n, 7)"""
    pc = raw[:, :3]
    lab = raw[:, 3].copy()
    lab[lab >= num_classes] = IGNORE_LABEL
    out = np.zeros((0, 7))
    kept = []
    for box in pseudo_boxes[pseudo_boxes[:, -1] == idx]:
        mask = crop_pc(pc, box) & (lab != IGNORE_LABEL)
        if mask.sum() > 0:
            vals, cnt = np.unique(lab[mask], return_counts=True)
            if vals[np.argmax(cnt)] == box[6]:          # scipy.stats.mode: smallest of the most frequent
                kept.append(box)
    if kept:
        out = np.concatenate([out, np.stack(kept, 0)[:, :7]], 0)
    return out


def bounds(rows):
    """float32 lo / hi of (n, 10) float32 rows, as crop_pc forms them"""
    half = rows[:, 3:6] / 2
    return rows[:, 0:3] - half, rows[:, 0:3] + half


def vote(points, labels, lo, hi, num_classes):
    """ov3d_box_points_count kind 1: points (B,N,3) f32 / f64, labels (B,N) uint8, lo / hi
    (B,K,3) f32 -> counts (B,K,C) int32, mode (B,K) int32 (-1: no vote)"""
    B, N = labels.shape
    K = lo.shape[1]
    counts = np.zeros((B, K, num_classes), np.int32)
    mode = np.full((B, K), -1, np.int32)
    for b in range(B):
        votes = labels[b] < num_classes
        for k in range(K):
            with np.errstate(invalid="ignore"):
                inside = (np.all(points[b] >= lo[b, k], -1) & np.all(points[b] <= hi[b, k], -1)) & votes
            counts[b, k] = np.bincount(labels[b][inside], minlength=num_classes)[:num_classes]
            if counts[b, k].max() > 0:
                mode[b, k] = np.argmax(counts[b, k])
    return counts, mode


def vote_torch(points, labels, lo, hi, num_classes):
    """`vote` behind box_label_votes' signature (tensors in, tensors out), for the host tests"""
    import torch
    c, m = vote(points.numpy(), labels.numpy(), lo.numpy(), hi.numpy(), num_classes)
    return torch.from_numpy(c), torch.from_numpy(m)
