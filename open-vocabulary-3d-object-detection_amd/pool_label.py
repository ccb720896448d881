"""Labels for an unlabelled proposal pool, by a per-box vote over per-vertex labels on the device.

Replaces ``3DOVDet_tools/scannet/assign_box_label_from_gt.py`` (``labeling``): every box of a
scan's GSS pool (``<scan>_prop.npy``, the pool ``lift_boxes`` matches against) takes the most
frequent ground-truth label (nyu40 id >= 3) among the scan's vertices inside it and is kept iff
that label is one of the 18 detection classes.  The files it writes are the supervised upper
bound that ``box_eval`` scores pseudo boxes against.  The reference makes one numpy pass over
all vertices per pool box in a process pool; here ``group`` scans are one launch of
``ov3d_poollabel_vote`` (csrc/poollabel.hip behind include/ov3d_poollabel.h), the scans in CSR
form, and one read-back of the modes.

The device does the vote; the host does, with the reference's own in-place expressions in
float64, what touches only boxes: ``cs2vv`` (lo = c - s/2 and then hi = s + lo, which is not
always c + s/2), the ``label in nyu40ids`` filter, the label into column 6 and ``vv2cs`` on the
kept rows.  A float32 vertex is compared with the float64 bounds in float64, as numpy does, so
a bound one float64 ulp from a vertex decides as in the reference; every kept number is copied
or computed by the same expression, so the files equal the reference's byte for byte.  The
pool's row order is kept.

Deliberate differences: a per-vertex label must be an integer in [0, 64); anything else (a
negative, a non-integer, NaN, 64 or more) raises ValueError naming the scan, where the
reference would vote on any value >= 3; nyu40 labels end at 40.  A pool box with a non-finite
number is refused the same way (the device's compares would drop it silently).  The pool is
(P, 7), as GSS writes it, and is taken as float64; vertices are float32 or float64.
"""
import os

import numpy as np
import torch

from . import _native as nat
from .lift_boxes import NYU40IDS

MIN_LABEL = 3                      # labeling: selected_label >= 3
NUM_BINS = 64                      # OV3D_POOLLABEL_MAX_C: every accepted label has a bin


def vote(points, labels, pt_off, boxes, box_off, min_label=MIN_LABEL, num_bins=NUM_BINS):
    """ov3d_poollabel_vote on device tensors, no synchronisation.  points (N, ld >= 3) float32
    or float64, labels (N) uint8, boxes (P, 6) float64 closed bounds lo | hi, pt_off / box_off
    (S+1) int32: the scans in CSR form.  -> (counts (P, C) int32, mode (P) int32: the smallest
    label among the most frequent of min_label .. C-1, -1 without a vote)."""
    pts = nat.check(points, "points", None, 2)
    if pts.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"points: expected float32 or float64, got {pts.dtype}")
    nat.check(labels, "labels", torch.uint8, 1)
    nat.check(boxes, "boxes", torch.float64, 2)
    nat.check(pt_off, "pt_off", torch.int32, 1)
    nat.check(box_off, "box_off", torch.int32, 1)
    N, P, S, C = pts.shape[0], boxes.shape[0], pt_off.numel() - 1, int(num_bins)
    if pts.shape[1] < 3 or labels.shape[0] != N or boxes.shape[1] != 6 or S < 1 or box_off.numel() != S + 1:
        raise ValueError("points (N, >= 3), labels (N), boxes (P, 6), pt_off and box_off (S + 1) expected")
    if not (1 <= C <= NUM_BINS and 0 <= min_label <= C):
        raise ValueError(f"1 <= num_bins <= {NUM_BINS} and 0 <= min_label <= num_bins")
    counts = torch.empty((P, C), dtype=torch.int32, device=pts.device)
    mode = torch.empty((P,), dtype=torch.int32, device=pts.device)
    nat.call("ov3d_poollabel_vote", pts, int(pts.dtype == torch.float64), pts.shape[1], labels, pt_off, N,
             boxes, box_off, P, S, int(min_label), C, counts, mode, like=boxes)
    return counts, mode


def _scan(points, sem_labels, pool, name):
    """validated (xyz (N, 3) float32 / float64, labels (N) uint8, pool (P, 7) float64 copy in
    two-vertex form)"""
    pts = np.asarray(points)
    if pts.ndim != 2 or pts.shape[1] < 3 or pts.dtype not in (np.float32, np.float64):
        raise ValueError(f"{name}: vertices must be a float32 / float64 (N, >= 3) array, got {pts.dtype} {pts.shape}")
    lab = np.asarray(sem_labels)
    if lab.shape != (pts.shape[0],) or lab.dtype.kind not in "iuf":
        raise ValueError(f"{name}: one numeric label per vertex expected, got {lab.dtype} {lab.shape}")
    with np.errstate(invalid="ignore"):
        bad = ~((lab >= 0) & (lab < NUM_BINS) & (lab == np.floor(lab)))
    if bad.any():
        raise ValueError(f"{name}: per-vertex label {lab[bad][0].item()!r} is not an integer in [0, {NUM_BINS})")
    boxes = np.array(pool, dtype=np.float64)                # a copy: cs2vv works in place
    if boxes.ndim != 2 or boxes.shape[1] != 7:
        raise ValueError(f"{name}: the pool must be (P, 7), got {boxes.shape}")
    if not np.isfinite(boxes).all():
        raise ValueError(f"{name}: pool box {int(np.nonzero(~np.isfinite(boxes).all(1))[0][0])} is not finite")
    boxes[:, :3] -= boxes[:, 3:6] / 2                       # cs2vv
    boxes[:, 3:6] += boxes[:, :3]
    return np.ascontiguousarray(pts[:, :3]), lab.astype(np.uint8), boxes


def _finish(boxes, mode):
    """the rows labeling saves, from the pool in two-vertex form and every box's mode"""
    keep = np.isin(mode, NYU40IDS)                          # -1 (no vote) is not one of them
    rows = boxes[keep]
    rows[:, 6] = mode[keep]
    rows[:, 3:6] -= rows[:, :3]                             # vv2cs
    rows[:, :3] += rows[:, 3:6] / 2
    return rows                                             # (0, 7), (1, 7) or the stack: float64


def vote_group(scans, device="cuda"):
    """the modes of a group of validated scans [(xyz, labels, boxes in two-vertex form)]: one
    launch and one read-back.  -> list of (P_s,) int32 arrays.  Float32 vertices go up as they
    are when the whole group is float32, else widened to float64, which is exact."""
    n_box = [len(s[2]) for s in scans]
    if sum(n_box) == 0:
        return [np.zeros(0, np.int32) for _ in scans]
    dt = np.float32 if all(s[0].dtype == np.float32 for s in scans) else np.float64
    off = lambda sizes: np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)    # noqa: E731
    pt_off, box_off = off([len(s[0]) for s in scans]), off(n_box)
    if pt_off[-1] >= 2 ** 31 or box_off[-1] >= 2 ** 31:
        raise ValueError("more than 2^31 - 1 vertices or boxes in a group")
    dev = torch.device(device)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)                 # noqa: E731
    _, mode = vote(up(np.concatenate([s[0].astype(dt, copy=False) for s in scans])),
                   up(np.concatenate([s[1] for s in scans])), up(pt_off.astype(np.int32)),
                   up(np.concatenate([s[2][:, :6] for s in scans])), up(box_off.astype(np.int32)))
    mode = mode.cpu().numpy()
    return [mode[box_off[i]: box_off[i + 1]] for i in range(len(scans))]


def label_pool(points, sem_labels, pool, device="cuda"):
    """One scan: points (N, >= 3) float32 or float64 vertices, sem_labels (N) nyu40 ids, pool
    (P, 7) centre, size and a seventh column that is overwritten -> what labeling saves:
    (n, 7) float64, centre, size, nyu40 id of the kept boxes in the pool's order."""
    scan = _scan(points, sem_labels, pool, "label_pool")
    return _finish(scan[2], vote_group([scan], device)[0])


class PoolLabeler:
    """assign_box_label_from_gt.py over files: ``<vert_dir>/<scan>_vert.npy`` (columns 0-2),
    ``<label_dir>/<scan>_sem_label.npy`` and ``<pool_dir>/<scan>_prop.npy`` ->
    ``<output_dir>/<scan>_bbox.npy``.  `group` scans share a launch and a read-back."""

    def __init__(self, vert_dir, label_dir, pool_dir, output_dir, device="cuda", group=8):
        if group < 1:
            raise ValueError("group: at least one scan per launch")
        self.vert_dir, self.label_dir, self.pool_dir, self.output_dir = vert_dir, label_dir, pool_dir, output_dir
        self.device, self.group = device, int(group)

    def _out(self, scan_name):
        return os.path.join(self.output_dir, scan_name + "_bbox.npy")

    def _read(self, scan_name):
        return _scan(np.load(os.path.join(self.vert_dir, scan_name) + "_vert.npy", allow_pickle=False)[:, :3],
                     np.load(os.path.join(self.label_dir, scan_name + "_sem_label.npy"), allow_pickle=False),
                     np.load(os.path.join(self.pool_dir, scan_name + "_prop.npy"), allow_pickle=False), scan_name)

    def _label(self, names):
        scans = [self._read(n) for n in names]
        os.makedirs(self.output_dir, exist_ok=True)
        counts = []
        for name, scan, mode in zip(names, scans, vote_group(scans, self.device)):
            rows = _finish(scan[2], mode)
            np.save(self._out(name), rows)
            counts.append(rows.shape[0])
        return counts

    def _existing(self, scan_name):
        return np.load(self._out(scan_name), allow_pickle=False).shape[0]

    def labeling(self, scan_name, replace=True):
        """one scan; -> the number of boxes written (replace=False and a file already there: the
        number of boxes in it, nothing is computed)"""
        if not replace and os.path.isfile(self._out(scan_name)):
            return self._existing(scan_name)
        return self._label([scan_name])[0]

    def run(self, scene_list, replace=True):
        """every scan of scene_list, `group` per launch -> the list of box counts"""
        scene_list = list(scene_list)
        counts = {}
        todo = []
        for i, name in enumerate(scene_list):
            if not replace and os.path.isfile(self._out(name)):
                counts[i] = self._existing(name)
            else:
                todo.append(i)
        for start in range(0, len(todo), self.group):
            part = todo[start: start + self.group]
            counts.update(zip(part, self._label([scene_list[i] for i in part])))
        return [counts[i] for i in range(len(scene_list))]
