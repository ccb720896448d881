"""Pseudo boxes scored against ground-truth boxes: per-class precision and recall, on the device.

Replaces ``3DOVDet_tools/scannet/evaluate_box.py`` with ``utils/evaluation/pr_helper.py``
(``PRCalculator``) and the ``eval_det.py`` / ``evaluation/box_util.py`` functions under it, for
axis-aligned boxes.  The reference makes one Python call of ``calc_iou`` per (pseudo box, GT box)
pair in a pool of 10 processes, once per threshold; here a whole split is two launches
(csrc/boxeval.hip behind include/ov3d_boxeval.h: ``ov3d_boxeval_match`` with one workgroup per
scan, ``ov3d_boxeval_tally`` with one per class), back to back on the current stream, for up to
16 IoU thresholds at once, and one device-to-host copy of the counters.

The reference as published: neither ``evaluate_box.py`` can be imported
(``utils/constants.py`` has no ``DATASET_ROOT_DIR`` / ``BOX_ROOT``), so ``PRCalculator`` and
``eval_det`` are what the tests pin and ``compute_precision_recall`` follows the script's loop.
The SUN RGB-D script passes ``obb=True``, with which ``eval_det_cls`` reads ``bb[7]`` of
7-element boxes and raises on the first pair: the oriented mode is not built.

What is kept of ``PRCalculator.compute_metrics``: the key order ('<name> Precision' of every
class in ascending order, 'mPrecision', '<name> Recall' of every class, 'AR'); the names
(``class2type_map[key]``, else ``str(key)`` of the first scalar seen for the class, predictions
before GT: '3.0' for a class read from a float file, '3' for a class that only GT has); a class
with GT and no prediction reports Precision 0 outside the mean and Recall 0 inside it; no
prediction at all gives mPrecision nan.  Precision is TP / nd and recall TP / max(npos, eps) at
the last detection; they do not depend on the order among equal scores (closed form in
csrc/boxeval.hip).  ``compute_curves`` orders equal scores by (scan, row), which the reference
leaves to ``argsort``.

Refused on the host before any launch: non-finite boxes or scores (numpy's ``min`` propagates
NaN, the device's does not) and class ids that are not integers in [0, 4096).  Arrays are
checked where they are; a device tensor costs one two-number read-back when it is handed in.
"""
import os

import numpy as np
import torch

from . import _native as nat
from .dataset_config import ScannetDatasetConfig
from .lift_boxes import NYU40IDS

MAX_THRESHOLDS = 16                # OV3D_BOXEVAL_MAX_T
MAX_CLASSES = 4096
_EPS = np.finfo(np.float64).eps

# the tools' names (utils/io_utils.py class2type): the 18 detection classes, the last one
# (nyu40 id 39) called "other furniture" there
SCANNET_CLASS2TYPE = dict(ScannetDatasetConfig().class2type)
SCANNET_CLASS2TYPE[17] = "other furniture"


def _class_ids(values, what):
    """integer-valued ids in [0, MAX_CLASSES) -> int32, else ValueError"""
    v = np.asarray(values)
    if v.dtype.kind not in "iuf":
        raise ValueError(f"{what}: class ids must be numbers, got {v.dtype}")
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(v) & (v == np.trunc(v)) & (v >= 0) & (v < MAX_CLASSES)
    if not ok.all():
        raise ValueError(f"{what}: class ids must be integers in [0, {MAX_CLASSES})")
    return v.astype(np.int32)


def _finite(a, what):
    if not np.isfinite(a).all():
        raise ValueError(f"{what}: values must be finite")
    return a


def _boxes(a, what, width):
    a = np.asarray(a)
    if a.ndim != 2 or a.shape[1] < width or a.dtype.kind not in "iuf":
        raise ValueError(f"{what}: expected a numeric (k, >= {width}) array, got {a.dtype} {a.shape}")
    return a


def launch(pred, pred_cls, score, pred_off, gt, gt_cls, gt_off, thr, C):
    """ov3d_boxeval_match then ov3d_boxeval_tally on device tensors, no synchronisation.
    pred (P, ld >= 6), gt (G, ld >= 6) f64; pred_cls (P), gt_cls (G), pred_off, gt_off (S+1)
    int32; score (P), thr (T) f64.  -> dict of device tensors rank, jmax (P) int32, ovmax (P),
    best (G) f64, owner (T,G) int32, tp (T,P) uint8, counts ((2+T) C) int32 with its views nd (C),
    npos (C), ntp (T,C)."""
    P, G, S, T = pred.shape[0], gt.shape[0], pred_off.numel() - 1, thr.numel()
    for t, name, dt, shape in ((pred, "pred", torch.float64, (P, None)), (gt, "gt", torch.float64, (G, None)),
                               (pred_cls, "pred_cls", torch.int32, (P,)), (gt_cls, "gt_cls", torch.int32, (G,)),
                               (score, "score", torch.float64, (P,)), (thr, "thr", torch.float64, (T,)),
                               (pred_off, "pred_off", torch.int32, (S + 1,)),
                               (gt_off, "gt_off", torch.int32, (S + 1,))):
        nat.check(t, name, dt, len(shape))
        if any(w is not None and w != g for w, g in zip(shape, t.shape)):
            raise ValueError(f"{name}: expected shape {shape}, got {tuple(t.shape)}")
    if S < 1 or not 1 <= T <= MAX_THRESHOLDS or C < 1 or pred.shape[1] < 6 or gt.shape[1] < 6:
        raise ValueError("at least one scan and one class, 1 to 16 thresholds, boxes of >= 6 columns")
    dev = thr.device
    new = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)   # noqa: E731
    counts = new(((2 + T) * C,), torch.int32)
    r = {"rank": new((P,), torch.int32), "jmax": new((P,), torch.int32), "ovmax": new((P,), torch.float64),
         "best": new((G,), torch.float64), "owner": new((T, G), torch.int32), "tp": new((T, P), torch.uint8),
         "counts": counts, "nd": counts[:C], "npos": counts[C:2 * C], "ntp": counts[2 * C:].view(T, C)}
    nat.call("ov3d_boxeval_match", pred, pred.shape[1], pred_cls, score, pred_off, P, gt, gt.shape[1],
             gt_cls, gt_off, G, S, thr, T, r["rank"], r["jmax"], r["ovmax"], r["best"], r["owner"],
             r["tp"], like=thr)
    nat.call("ov3d_boxeval_tally", pred_cls, P, gt_cls, r["best"], G, thr, T, C, r["nd"], r["npos"],
             r["ntp"], like=thr)
    return r


def run_device(pack, thr, C, device, flags=False):
    """upload what is on the host, the two launches, one read-back.  pack: pred, pred_cls,
    score, pred_off, gt, gt_cls, gt_off as numpy arrays or device tensors.  -> numpy nd (C),
    npos (C), ntp (T,C); with flags also tp (T,P) and ovmax (P) (a second copy, for curves)."""
    dev = torch.device(device)
    up = lambda a: a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    t = {k: up(v) for k, v in pack.items()}
    T = len(thr)
    r = launch(t["pred"], t["pred_cls"], t["score"], t["pred_off"], t["gt"], t["gt_cls"], t["gt_off"],
               up(np.asarray(thr, np.float64)), C)
    counts = r["counts"].cpu().numpy()
    out = dict(nd=counts[:C], npos=counts[C:2 * C], ntp=counts[2 * C:].reshape(T, C))
    if flags:
        out.update(tp=r["tp"].cpu().numpy(), ovmax=r["ovmax"].cpu().numpy())
    return out


def voc_ap(rec, prec):
    """area under the precision envelope (eval_det.voc_ap without the 11-point variant)"""
    mrec = np.concatenate(([0.0], rec, [1.0]))
    mpre = np.concatenate(([0.0], prec, [0.0]))
    mpre = np.maximum.accumulate(mpre[::-1])[::-1]
    i = np.where(mrec[1:] != mrec[:-1])[0]
    return np.sum((mrec[i + 1] - mrec[i]) * mpre[i + 1])


class PRCalculator:
    """Precision and recall of accumulated predictions against ground truth (pr_helper.py
    PRCalculator).  ap_iou_thresh: a float, or a sequence of up to 16 thresholds evaluated by the
    same two launches (compute_metrics then returns {threshold: dict})."""

    def __init__(self, ap_iou_thresh=0.25, class2type_map=None, obb=False, device="cuda"):
        if obb:
            raise NotImplementedError(
                "oriented boxes (obb=True) are not built: the reference's own path reads bb[7] of "
                "7-element boxes in eval_det_cls and raises IndexError on its first pair")
        self.single = np.ndim(ap_iou_thresh) == 0
        self.thresholds = [float(t) for t in np.atleast_1d(np.asarray(ap_iou_thresh, np.float64))]
        if not 1 <= len(self.thresholds) <= MAX_THRESHOLDS or any(t != t for t in self.thresholds):
            raise ValueError(f"ap_iou_thresh: 1 to {MAX_THRESHOLDS} thresholds, none NaN")
        self.ap_iou_thresh = ap_iou_thresh
        self.class2type_map = class2type_map
        self.device = device
        self.reset()

    def reset(self):
        self._scans = []               # (pred6, pred_cls, score, gt6, gt_cls) per scan
        self._pred_key, self._gt_key = {}, {}
        self._max_cls = -1
        self._tensor_key = np.float64
        self.scan_cnt = 0

    # ------------------------------------------------------------ accumulation
    def _remember(self, keys, ids, raw):
        for c, k in zip(ids.tolist(), raw):
            if c not in keys:
                keys[c] = k
        if len(ids):
            self._max_cls = max(self._max_cls, int(ids.max()))

    def step(self, batch_pred_map_cls, batch_gt_map_cls):
        """batch_pred_map_cls: per scan a list of (class, box (>= 6), score);
        batch_gt_map_cls: per scan a list of (class, box (>= 6))"""
        if len(batch_pred_map_cls) != len(batch_gt_map_cls):
            raise ValueError("one GT list per prediction list")
        for preds, gts in zip(batch_pred_map_cls, batch_gt_map_cls):
            six = lambda rows: np.array([np.asarray(r[1], np.float64)[:6] for r in rows],  # noqa: E731
                                        np.float64).reshape(len(rows), 6)
            pkeys, gkeys = [r[0] for r in preds], [r[0] for r in gts]
            score = np.array([r[2] for r in preds], np.float64).reshape(len(preds))
            self._add(_finite(six(preds), "predictions"), _class_ids(np.array(pkeys, np.float64), "predictions"),
                      _finite(score, "scores"), pkeys, _finite(six(gts), "GT boxes"),
                      _class_ids(np.array(gkeys, np.float64), "GT boxes"), gkeys)

    def step_arrays(self, pred, gt, gt_cls):
        """one scan: pred (k, >= 7) centre, size, class index (the rows lift_scannet_scan
        returns), gt (g, >= 6) centre, size, gt_cls (g) class indices; numpy arrays, or tensors
        (device tensors are used where they are).  The score of a prediction is (sx sy) sz in
        pred's own dtype."""
        if any(isinstance(a, torch.Tensor) and a.device.type != "cpu" for a in (pred, gt, gt_cls)):
            return self._add_tensors(pred, gt, gt_cls)
        pred, gt, gt_cls = (a.numpy() if isinstance(a, torch.Tensor) else a for a in (pred, gt, gt_cls))
        pred, gt = _boxes(pred, "pred", 7), _boxes(gt, "gt", 6)
        gt_cls = np.asarray(gt_cls).reshape(-1)
        if len(gt_cls) != len(gt):
            raise ValueError("gt_cls: one class per GT box")
        _finite(pred[:, :6], "pred")
        score = (pred[:, 3] * pred[:, 4]) * pred[:, 5]
        self._add(pred[:, :6].astype(np.float64), _class_ids(pred[:, 6], "pred"),
                  _finite(score.astype(np.float64), "scores"), pred[:, 6],
                  _finite(gt[:, :6].astype(np.float64), "gt"), _class_ids(gt_cls, "gt_cls"), gt_cls)

    def _add(self, pred6, pcls, score, pkeys, gt6, gcls, gkeys):
        self._remember(self._pred_key, pcls, pkeys)
        self._remember(self._gt_key, gcls, gkeys)
        self._scans.append((pred6, pcls, score, gt6, gcls))
        self.scan_cnt += 1

    def _add_tensors(self, pred, gt, gt_cls):
        dev = torch.device(self.device)
        pred, gt, gt_cls = (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.asarray(a))
                            for a in (pred, gt, gt_cls))
        pred, gt, gt_cls = pred.to(dev), gt.to(dev), gt_cls.to(dev).reshape(-1)
        if pred.dim() != 2 or pred.shape[1] < 7 or gt.dim() != 2 or gt.shape[1] < 6 or len(gt_cls) != len(gt):
            raise ValueError("pred (k, >= 7), gt (g, >= 6), gt_cls (g)")
        score = ((pred[:, 3] * pred[:, 4]) * pred[:, 5]).to(torch.float64)
        pc, gc = pred[:, 6].to(torch.float64), gt_cls.to(torch.float64)
        p6, g6 = pred[:, :6].to(torch.float64), gt[:, :6].to(torch.float64)
        cls = torch.cat([pc, gc])
        if cls.numel():
            ok = (torch.isfinite(p6).all() & torch.isfinite(g6).all() & torch.isfinite(score).all()
                  & (cls == cls.trunc()).all() & (cls >= 0).all() & (cls < MAX_CLASSES).all())
            ok, top = torch.stack([ok.to(torch.float64), torch.nan_to_num(cls).max()]).cpu().tolist()
            if not ok:
                raise ValueError(f"boxes must be finite and class ids integers in [0, {MAX_CLASSES})")
            self._max_cls = max(self._max_cls, int(top))
        elem = np.dtype(str(pred.dtype).replace("torch.", "")).type
        self._scans.append((p6, pc.to(torch.int32), score, g6, gc.to(torch.int32)))
        self._tensor_key = elem
        self.scan_cnt += 1

    # ------------------------------------------------------------ evaluation
    def _pack(self):
        """-> (pack for run_device, C): the scans in CSR form"""
        scans = self._scans
        on_device = any(isinstance(s[0], torch.Tensor) for s in scans)
        off = lambda col: np.concatenate([[0], np.cumsum([len(s[col]) for s in scans])]).astype(np.int32)  # noqa: E731
        if on_device:
            dev = torch.device(self.device)
            up = lambda a: a if isinstance(a, torch.Tensor) else torch.from_numpy(a).to(dev)   # noqa: E731
            cat = lambda col: torch.cat([up(s[col]) for s in scans]).contiguous()              # noqa: E731
        else:
            cat = lambda col: np.concatenate([s[col] for s in scans])                          # noqa: E731
        pack = dict(pred=cat(0), pred_cls=cat(1), score=cat(2), pred_off=off(0), gt=cat(3), gt_cls=cat(4),
                    gt_off=off(3))
        if max(len(pack["pred"]), len(pack["gt"])) >= 2 ** 31:
            raise ValueError("more than 2^31 - 1 boxes")
        return pack, max(self._max_cls + 1, 1)

    def _key(self, c, predicted):
        if c in self._pred_key:
            return self._pred_key[c]
        if predicted:                  # seen only inside a device tensor: the scalar it would read as
            return self._tensor_key(c)
        return self._gt_key.get(c, c)

    def _name(self, key):
        return self.class2type_map[key] if self.class2type_map else str(key)

    def _metrics(self, nd, npos, ntp):
        """PRCalculator.compute_metrics from the counters of one threshold"""
        classes = [c for c in range(len(nd)) if nd[c] or npos[c]]
        names = [self._name(self._key(c, nd[c] > 0)) for c in classes]
        tp = ntp.astype(np.float64)
        ret, prec_list, rec_list = {}, [], []
        for c, name in zip(classes, names):
            if nd[c]:
                ret["%s Precision" % name] = tp[c] / np.maximum(np.float64(nd[c]), _EPS)
                prec_list.append(ret["%s Precision" % name])
            else:
                ret["%s Precision" % name] = 0
        ret["mPrecision"] = np.mean(prec_list) if prec_list else np.float64(np.nan)
        for c, name in zip(classes, names):
            ret["%s Recall" % name] = tp[c] / np.maximum(float(npos[c]), _EPS) if nd[c] else 0
            rec_list.append(ret["%s Recall" % name])
        ret["AR"] = np.mean(rec_list) if rec_list else np.float64(np.nan)
        return ret

    def compute_metrics(self):
        """-> the reference's dict; {threshold: dict} when ap_iou_thresh was a sequence"""
        if not self._scans:            # nothing to count, nothing to launch: the reference's nan, nan
            zero = np.zeros(1, np.int32)
            r = dict(nd=zero, npos=zero, ntp=np.zeros((len(self.thresholds), 1), np.int32))
        else:
            pack, C = self._pack()
            r = run_device(pack, self.thresholds, C, self.device)
        out = [self._metrics(r["nd"], r["npos"], r["ntp"][t]) for t in range(len(self.thresholds))]
        return out[0] if self.single else dict(zip(self.thresholds, out))

    def compute_curves(self):
        """-> (rec, prec, ap) as eval_det_multiprocessing returns them: dicts by class key of the
        cumulative recall and precision over the class's detections by descending score (equal
        scores by scan, then row) and the average precision; 0, 0, 0 for a class without
        predictions.  {threshold: (rec, prec, ap)} when ap_iou_thresh was a sequence."""
        if not self._scans:
            out = [({}, {}, {}) for _ in self.thresholds]
            return out[0] if self.single else dict(zip(self.thresholds, out))
        pack, C = self._pack()
        r = run_device(pack, self.thresholds, C, self.device, flags=True)
        host = lambda a: a.cpu().numpy() if isinstance(a, torch.Tensor) else a   # noqa: E731
        score, pcls = host(pack["score"]), host(pack["pred_cls"])
        order = np.argsort(-score, kind="stable")
        out = []
        for t in range(len(self.thresholds)):
            rec, prec, ap = {}, {}, {}
            for c in range(C):
                if not (r["nd"][c] or r["npos"][c]):
                    continue
                key = self._key(c, r["nd"][c] > 0)
                if not r["nd"][c]:
                    rec[key] = prec[key] = ap[key] = 0
                    continue
                sel = order[pcls[order] == c]
                tp = np.cumsum(r["tp"][t, sel].astype(np.float64))
                fp = np.cumsum(1.0 - r["tp"][t, sel].astype(np.float64))
                rec[key] = tp / np.maximum(float(r["npos"][c]), _EPS)
                prec[key] = tp / np.maximum(tp + fp, _EPS)
                ap[key] = voc_ap(rec[key], prec[key])
            out.append((rec, prec, ap))
        return out[0] if self.single else dict(zip(self.thresholds, out))


def _nyu40_to_class(ids, scan, what):
    v = np.asarray(ids)
    idx = np.searchsorted(NYU40IDS, v)
    ok = (idx < len(NYU40IDS)) & (NYU40IDS[np.minimum(idx, len(NYU40IDS) - 1)] == v)
    if not ok.all():
        raise ValueError(f"{scan}: {what} holds an id outside nyu40ids ({v[~ok][0]!r})")
    return idx


def compute_precision_recall(scan_names, box_dir, gt_dir, iou_thresh=0.25, class2type_map=SCANNET_CLASS2TYPE,
                             pred_ids="class", device="cuda"):
    """evaluate_box.py compute_precision_recall over files: box_dir/<scan>_bbox.npy (k, >= 7)
    pseudo boxes with the class index in column 6 (pred_ids="nyu40": the nyu40 id, the training
    format of lift_boxes.to_training_format), gt_dir/<scan>_bbox.npy (g, >= 7) with the nyu40 id
    in column 6.  A scan without pseudo boxes is skipped together with its GT, as the script
    does.  -> (metrics, avg_num, total_num); metrics as PRCalculator.compute_metrics."""
    if pred_ids not in ("class", "nyu40"):
        raise ValueError("pred_ids: 'class' or 'nyu40'")
    calc = PRCalculator(iou_thresh, class2type_map, device=device)
    all_p = []
    for scan in scan_names:
        prop = np.load(os.path.join(box_dir, scan + "_bbox.npy"), allow_pickle=False)
        if prop.shape[0] == 0:
            continue
        prop = _boxes(prop, scan + " pseudo boxes", 7)
        if pred_ids == "nyu40":
            prop = np.array(prop[:, :7])
            prop[:, 6] = _nyu40_to_class(prop[:, 6], scan, "the pseudo boxes' column 6")
        all_p.append(prop.shape[0])
        gt = _boxes(np.load(os.path.join(gt_dir, scan + "_bbox.npy"), allow_pickle=False), scan + " GT boxes", 7)
        calc.step_arrays(prop, gt, _nyu40_to_class(gt[:, 6], scan, "the GT boxes' column 6"))
    avg_num = np.mean(all_p) if all_p else np.float64(np.nan)
    return calc.compute_metrics(), avg_num, sum(all_p)


def print_metrics(metrics, avg_num, total_num, iou_thresh, file=None):
    """the lines evaluate_box.py prints"""
    print("-" * 10, f"prop: iou_thresh: {iou_thresh}", "-" * 10, file=file)
    print("avg num: %.2f total number: %d" % (avg_num, total_num), file=file)
    for key in metrics:
        print("eval %s: %f" % (key, metrics[key]), file=file)
