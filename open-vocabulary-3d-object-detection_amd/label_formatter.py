"""Pseudo-label generation on the device.

Drop-in for utils/label_formatter.py ``LabelFormatter`` (the reference's third program,
generate_pseudo_label.py -> engine.py:235-302 inference): the trained model runs over the
training scans, every query's box is thresholded on class confidence and objectness, and a box
is kept only if the most frequent LSeg label among the scan's vertices inside it is the box's
own class; the kept boxes are written as ``<scan>_bbox.npy``, which the next training phase
reads through ``use_pbox`` / ``pseudo_box_dir`` (scannet.py).

* ``step`` (label_formatter.py:81-106) keeps the ten columns of each batch ON THE DEVICE: no
  host synchronisation, no copy, legal inside a hipGraph capture.
* ``compute`` (:117-132) does the one device -> host read and the thresholding, in the
  reference's order (class-major, within a class in step order) and in float32.
* ``gen_pseudo`` / ``save`` (:134-174) vote on the device: the scans of a group are padded to
  one (B, N) block (label 255), their candidate boxes to one (B, K) block (empty boxes), and
  one launch of ``ov3d_box_points_count`` kind 1 per group and point dtype returns every
  box's most frequent label (csrc/evaldet.hip box_label_vote_kernel).  No process pool, no
  numpy pass over the vertices per box.

Everything compared is an integer or a copied float32, so the files equal the reference's
exactly.  One deliberate difference: a per-vertex label must be an integer in [0, num_classes)
(a class), or >= num_classes or -100 (ignored: project_label(..., True) and IGNORE_LABEL).
Anything else (a negative other than -100, a non-integer, NaN) raises ValueError naming the
scan; the reference would count such a value as a label of its own, and no segmentation output
holds one.
"""
import os

import numpy as np
import torch

from . import _native as nat

IGNORE_LABEL = -100
PAD_LABEL = 255            # a byte that never votes (the entry ignores every value >= C)
MAX_CLASSES = 32           # ov3d_box_points_count kind 1


def box_label_votes(points, labels, lo, hi, num_classes):
    """Label vote of every box: points (B,N,3) float32 or float64, labels (B,N) uint8 (a value
    >= num_classes does not vote), lo / hi (B,K,3) float32 closed bounds -> (counts (B,K,C)
    int32, mode (B,K) int32: the smallest label among the most frequent, -1 without a vote)."""
    pts = nat.check_device(points.detach(), "points")
    if pts.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"points: expected float32 or float64, got {pts.dtype}")
    if pts.dim() != 3 or pts.shape[2] < 3:
        raise ValueError(f"points: expected (B, N, 3), got shape {tuple(pts.shape)}")
    if pts.stride(2) != 1:
        pts = pts.contiguous()
    lab = nat.check(labels.detach(), "labels", torch.uint8, 2)
    boxes = nat.check(torch.cat([lo.detach(), hi.detach()], -1).contiguous(), "lo | hi",
                      torch.float32, 3)
    B, N = lab.shape
    K, C = boxes.shape[1], int(num_classes)
    if pts.shape[:2] != (B, N) or boxes.shape[0] != B or boxes.shape[2] != 6:
        raise ValueError("points (B,N,3), labels (B,N), lo / hi (B,K,3) expected")
    counts = torch.empty((B, K, C), dtype=torch.int32, device=pts.device)
    mode = torch.empty((B, K), dtype=torch.int32, device=pts.device)
    nat.call("ov3d_box_points_count", pts, int(pts.dtype == torch.float64), pts.stride(0),
             pts.stride(1), N, boxes, 1, lab, C, B, K, counts, mode, like=pts)
    return counts, mode


def scan_labels(raw, num_classes, name):
    """per-vertex labels of a scan (its 4th column) -> uint8, PAD_LABEL where ignored; see the
    module docstring for what raises"""
    lab = np.asarray(raw)
    ignored = (lab >= num_classes) | (lab == IGNORE_LABEL)
    cls = (lab >= 0) & (lab < num_classes) & (lab == np.floor(lab))
    bad = ~(ignored | cls)
    if bad.any():
        raise ValueError(f"{name}: per-vertex label {lab[bad][0]!r} is neither a class in "
                         f"[0, {num_classes}) nor ignored (>= {num_classes} or {IGNORE_LABEL})")
    return np.where(cls, lab, PAD_LABEL).astype(np.uint8)


class LabelFormatter:
    """utils/label_formatter.py:66-206 with the reference's four leading arguments and method
    names.  `scans` (a list of (n, 4) arrays: xyz + label, float32 or float64, one per name of
    `scene_list`) replaces reading ``label_path/<scan>.npy``; `group` scans share a launch."""

    def __init__(self, box_path, output_path, label_path, scene_list, device="cuda",
                 num_classes=18, scans=None, group=8):
        if not 1 <= num_classes <= MAX_CLASSES:
            raise ValueError(f"num_classes must be in 1..{MAX_CLASSES}")
        self.boxes = []
        self.pseudo_box_dir = box_path
        self.output_path = output_path
        self.scene_list = list(scene_list)
        self.raw_label_path = os.path.join(label_path, "{}.npy") if label_path is not None else None
        self.IGNORE_LABEL = IGNORE_LABEL
        self.device = torch.device(device)
        self.num_classes = int(num_classes)
        self.group = int(group)
        self._scans = None
        if scans is not None:
            if len(scans) != len(self.scene_list):
                raise ValueError("one scan per name of scene_list")
            self._scans = [self._split(s, n) for s, n in zip(scans, self.scene_list)]

    # ---- scans
    def _split(self, raw, name):
        raw = np.asarray(raw)
        if raw.ndim != 2 or raw.shape[1] < 4 or raw.dtype not in (np.float32, np.float64):
            raise ValueError(f"{name}: a scan must be a float32 / float64 (n, 4) array: xyz + label")
        return np.ascontiguousarray(raw[:, :3]), scan_labels(raw[:, 3], self.num_classes, name)

    def _scan(self, idx):
        """-> (xyz (n, 3) in the file's dtype, labels (n,) uint8), validated when read"""
        if self._scans is not None:
            return self._scans[idx]
        name = self.scene_list[idx]
        return self._split(np.load(self.raw_label_path.format(name)), name)

    # ---- label_formatter.py:81-106
    def step(self, outputs, batch_data_label):
        """box: center, size, label, score, objectness prob, idx; kept on the device"""
        prob = outputs["sem_cls_prob"].detach()
        B, Q, C = prob.shape
        score = prob.amax(-1)
        # torch.max's index on the host: the first maximum (a NaN row: the first NaN)
        hit = (prob == score[..., None]) | (prob.isnan() & score.isnan()[..., None])
        cls = torch.arange(C, device=prob.device)
        label = torch.where(hit, cls, C).amin(-1)
        scan = batch_data_label["scan_idx"].to(prob.device)[:, None].expand(B, Q)
        rows = torch.cat([outputs["center_unnormalized"].detach(), outputs["size_unnormalized"].detach(),
                          torch.stack([label, score, outputs["objectness_prob"].detach(), scan], -1)],
                         -1).view(B * Q, 10)
        self.boxes.append(rows.float())

    # ---- label_formatter.py:117-132
    def compute(self, k, th_s, th_o):
        """thresholds per class; `k` is accepted and unused, as in the reference.  The one
        device -> host read."""
        if isinstance(self.boxes, list):
            if not self.boxes:
                raise ValueError("compute() before any step()")
            self.boxes = torch.cat(self.boxes, 0).cpu().numpy()
        rows = self.boxes
        # numpy compares a float32 array with a Python float in float32
        keep = (rows[:, 7] >= np.float32(th_s)) & (rows[:, 8] >= np.float32(th_o))
        self.pseudo_boxes = np.concatenate(
            [rows[(rows[:, 6] == label) & keep] for label in range(self.num_classes)], 0)

    # ---- label_formatter.py:134-174
    def _candidates(self, idx):
        return self.pseudo_boxes[self.pseudo_boxes[:, -1] == idx]

    def _vote_group(self, idxs):
        """-> {scan index: kept rows (n, 10)} for the scans of `idxs` that have candidates"""
        todo = {}
        for i in idxs:
            xyz, lab = self._scan(i)                    # every scan is read (and validated)
            cand = self._candidates(i)
            if cand.shape[0] and xyz.shape[0]:
                todo[i] = (xyz, lab, cand)
        kept = {}
        for dt in (np.float32, np.float64):
            part = [i for i in todo if todo[i][0].dtype == dt]
            if not part:
                continue
            n_max = max(todo[i][0].shape[0] for i in part)
            k_max = max(todo[i][2].shape[0] for i in part)
            pts = np.zeros((len(part), n_max, 3), dt)
            lab = np.full((len(part), n_max), PAD_LABEL, np.uint8)
            lo = np.ones((len(part), k_max, 3), np.float32)      # padding: lo > hi, empty
            hi = np.zeros((len(part), k_max, 3), np.float32)
            for r, i in enumerate(part):
                xyz, lb, cand = todo[i]
                pts[r, : xyz.shape[0]] = xyz
                lab[r, : lb.shape[0]] = lb
                half = cand[:, 3:6] / 2                           # float32, as crop_pc (:184-185)
                lo[r, : cand.shape[0]] = cand[:, 0:3] - half
                hi[r, : cand.shape[0]] = cand[:, 0:3] + half
            dev = self.device
            _, mode = box_label_votes(torch.from_numpy(pts).to(dev), torch.from_numpy(lab).to(dev),
                                      torch.from_numpy(lo).to(dev), torch.from_numpy(hi).to(dev),
                                      self.num_classes)
            mode = mode.cpu().numpy()
            for r, i in enumerate(part):
                cand = todo[i][2]
                kept[i] = cand[mode[r, : cand.shape[0]] == cand[:, 6]]
        return kept

    def _write(self, idx, rows):
        """the reference's np.concatenate([zeros((0, 7)), rows[:, :7]]): float64 (n, 7)"""
        out = np.zeros((0, 7))
        if rows is not None and rows.shape[0]:
            out = np.concatenate([out, rows[:, :7]], 0)
        np.save(os.path.join(self.output_path, self.scene_list[idx]) + "_bbox.npy", out)
        return out.shape[0]

    def gen_pseudo(self, idx):
        return self._write(idx, self._vote_group([idx]).get(idx))

    def save(self):
        os.makedirs(self.output_path, exist_ok=True)
        total = 0
        for start in range(0, len(self.scene_list), self.group):
            idxs = range(start, min(start + self.group, len(self.scene_list)))
            kept = self._vote_group(idxs)
            total += sum(self._write(i, kept.get(i)) for i in idxs)
        return total

    def process(self, k, th_s, th_o):
        self.compute(k, th_s, th_o)
        n = self.save()
        print("Done! Acquired {} boxes.".format(n))


def generate(model, dataset, formatter, batch_size, rng=None):
    """The body of engine.py:267-298 for the device loader: every scan of `dataset` once, in
    order, through model.eval() under no_grad into formatter.step; nothing synchronises inside
    the loop.  -> formatter (call process(k, th_s, th_o) next)."""
    if getattr(dataset, "augment", False):
        raise ValueError("pseudo labels are generated from unaugmented scans (augment=False)")
    model.eval()
    with torch.no_grad():
        for start in range(0, len(dataset), batch_size):
            batch = dataset.get_batch(list(range(start, min(start + batch_size, len(dataset)))), rng)
            outputs = model({k: batch[k] for k in ("point_clouds", "point_cloud_dims_min",
                                                   "point_cloud_dims_max")})
            formatter.step(outputs["outputs"], batch)
    return formatter
