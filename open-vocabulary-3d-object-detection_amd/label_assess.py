"""How well the 2D pseudo labels agree with the ground-truth frames, counted on the device.

Replaces ``3DOVDet_tools/scannet/assess_pseudo_label.py`` (``match``): LSeg's per-pixel class
indices against the ``label-mapped`` frames of a scan.  The reference reports one ratio per
scan; here ``group`` scans are one launch of ``ov3d_poollabel_confusion`` (csrc/poollabel.hip
behind include/ov3d_poollabel.h) that returns the per-class confusion counts, and the
reference's ``count`` and ``total`` fall out of them exactly: ``total`` is every pixel and
``count`` the trace including the ignored-ignored cell, because the reference projects both
sides' ignored pixels to -100 and counts them as agreeing.

Rows of the matrix are the ground truth, columns the pseudo labels; index 18 is "ignored".
The ground truth is mapped as ``ProjectionHelper.project_label(., False)`` does: nyu40ids[i]
becomes class i, everything else is ignored.  A pseudo label is a class 0..17 or ignored (>= 18
as ``project_label(., True)`` has it, or -100).

Out of scope, as elsewhere: decoding the frames and reading LSeg's pickled dicts; arrays go
in.  Deliberate difference: a ground-truth value must be an integer in [0, 256) and a pseudo
label a class or ignored; anything else (a negative other than -100, a non-integer, NaN)
raises ValueError naming the scan, where the reference would compare the stray value as a
label of its own.
"""
import numpy as np
import torch

from . import _native as nat
from .lift_boxes import NYU40IDS

NUM_CLASSES = 18
IGNORE_LABEL = -100
IGNORED_BYTE = 255                 # any byte >= the class count lands in the "ignored" bin

GT_MAP = np.full(256, NUM_CLASSES, np.uint8)
GT_MAP[NYU40IDS] = np.arange(NUM_CLASSES, dtype=np.uint8)


def confusion(gt, pseudo, frame_off, gt_map, num_classes=NUM_CLASSES):
    """ov3d_poollabel_confusion on device tensors, no synchronisation.  gt, pseudo (F, HW)
    uint8, frame_off (S+1) int32 (scan s owns the frames frame_off[s] .. frame_off[s+1]-1),
    gt_map (256) uint8 -> conf (S, K+1, K+1) int64, cleared by the entry itself."""
    nat.check(gt, "gt", torch.uint8, 2)
    nat.check(pseudo, "pseudo", torch.uint8, 2)
    nat.check(frame_off, "frame_off", torch.int32, 1)
    nat.check(gt_map, "gt_map", torch.uint8, 1)
    F, HW = gt.shape
    S, K = frame_off.numel() - 1, int(num_classes)
    if pseudo.shape != gt.shape or S < 1 or gt_map.numel() != 256 or HW < 1 or not 1 <= K <= 31:
        raise ValueError("gt and pseudo (F, HW >= 1), frame_off (S + 1), gt_map (256), 1 <= classes <= 31 expected")
    conf = torch.empty((S, K + 1, K + 1), dtype=torch.int64, device=gt_map.device)
    nat.call("ov3d_poollabel_confusion", gt, pseudo, frame_off, F, HW, S, gt_map, K, conf, like=gt_map)
    return conf


def _frames(gt_frames, pseudo_frames, name):
    """one scan's (F, H, W) arrays -> validated uint8 (F, H*W) pair"""
    gt, ps = np.asarray(gt_frames), np.asarray(pseudo_frames)
    if gt.ndim != 3 or ps.shape != gt.shape or gt.dtype.kind not in "iuf" or ps.dtype.kind not in "iuf":
        raise ValueError(f"{name}: two numeric (F, H, W) arrays of one shape expected, got {gt.shape} and {ps.shape}")
    with np.errstate(invalid="ignore"):
        bad = ~((gt >= 0) & (gt < 256) & (gt == np.floor(gt)))
        if bad.any():
            raise ValueError(f"{name}: ground-truth label {gt[bad][0].item()!r} is not an integer in [0, 256)")
        cls = (ps >= 0) & (ps < NUM_CLASSES) & (ps == np.floor(ps))
        bad = ~(cls | (ps >= NUM_CLASSES) | (ps == IGNORE_LABEL))
    if bad.any():
        raise ValueError(f"{name}: pseudo label {ps[bad][0].item()!r} is neither a class in [0, {NUM_CLASSES}) nor "
                         f"ignored (>= {NUM_CLASSES} or {IGNORE_LABEL})")
    F, HW = gt.shape[0], gt.shape[1] * gt.shape[2]
    return gt.astype(np.uint8).reshape(F, HW), np.where(cls, ps, IGNORED_BYTE).astype(np.uint8).reshape(F, HW)


def _group(frames, device):
    """[(gt bytes, pseudo bytes)] of one pixel count per frame -> (S, 19, 19) int64 on the host:
    one launch, one read-back"""
    dev = torch.device(device)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)                 # noqa: E731
    off = np.concatenate([[0], np.cumsum([len(g) for g, _ in frames])])
    if off[-1] >= 2 ** 31:
        raise ValueError("more than 2^31 - 1 frames in a group")
    conf = confusion(up(np.concatenate([g for g, _ in frames])), up(np.concatenate([p for _, p in frames])),
                     up(off.astype(np.int32)), up(GT_MAP))
    return conf.cpu().numpy()


def frame_confusion(gt_frames, pseudo_frames, device="cuda"):
    """One scan: gt_frames (F, H, W) nyu40 ids as load_label gives them (float32 or an integer
    type), pseudo_frames (F, H, W) LSeg class indices -> (19, 19) int64, conf[g][p] the pixels
    with ground-truth class g and pseudo class p, index 18 being "ignored"."""
    return _group([_frames(gt_frames, pseudo_frames, "frame_confusion")], device)[0]


def _count_total(conf):
    return int(np.trace(conf)), int(conf.sum())


def match(gt_frames, pseudo_frames, device="cuda"):
    """assess_pseudo_label.py match for one scan's arrays -> (count, total) as Python ints"""
    return _count_total(frame_confusion(gt_frames, pseudo_frames, device))


def assess(scans, device="cuda", group=8):
    """scans: an iterable of (name, gt_frames, pseudo_frames); `group` scans per launch (fewer
    where the frame size changes).  -> (the per-scan (count, total) pairs, the sum of the
    counts, the sum of the totals, the summed (19, 19) confusion matrix)."""
    if group < 1:
        raise ValueError("group: at least one scan per launch")
    pairs, total_conf = [], np.zeros((NUM_CLASSES + 1, NUM_CLASSES + 1), np.int64)
    pending = []

    def flush():
        if pending:
            for conf in _group(pending, device):
                pairs.append(_count_total(conf))
                total_conf[...] += conf
            pending.clear()

    for name, gt_frames, pseudo_frames in scans:
        frames = _frames(gt_frames, pseudo_frames, name)
        if pending and (len(pending) == group or pending[0][0].shape[1] != frames[0].shape[1]):
            flush()
        pending.append(frames)
    flush()
    return pairs, sum(c for c, _ in pairs), sum(t for _, t in pairs), total_conf
