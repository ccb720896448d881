"""Writes tests/golden/box_eval.npz: the REFERENCE's own PRCalculator
(3DOVDet_tools/utils/evaluation/pr_helper.py, on eval_det.py's eval_det_multiprocessing, get_iou
and evaluation/box_util.py's calc_iou, imported unchanged) over box_eval_cases.py.  Run it in a
process of its own: the tools' `utils` directory goes on sys.path.

Two facts about the reference as published.  Neither evaluate_box.py can be imported:
utils/constants.py defines no DATASET_ROOT_DIR / BOX_ROOT.  So PRCalculator and eval_det are
what is recorded, and the loop of scannet/evaluate_box.py compute_precision_recall is restated
in run_loop below, step for step, on arrays instead of files.  The SUN RGB-D script passes
obb=True, with which eval_det_cls reads bb[7] of 7-element boxes and raises IndexError on the
first pair; the oriented mode is not recorded.

Recorded per case, mode (`step`: every scan; `loop`: the script's loop, which skips a scan
without predictions together with its GT) and threshold: the metric dict's keys in order, its
values and which of them are Python ints; the per-class TP totals, nd and npos; for "curve"
cases rec, prec and ap of every class; for `loop` avg num and total number.

Asserted per case, or the generator fails: every ovmax is equal to or at least 1e-9 from every
threshold; "curve" cases have pairwise distinct scores per class across scans; the closed-form
TP totals of the restatement (tests/box_eval_ref.py) equal the reference's; and the cases
together hold every situation listed in CHECKS."""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import box_eval_cases as BC  # noqa: E402
import box_eval_ref as R  # noqa: E402

TOOLS = os.path.join(os.environ.get("OV3D_REFERENCE", "/root/reference"), "3DOVDet_tools")
MARGIN = 1e-9
seen = set()


def reference():
    for p in (os.path.join(TOOLS, "utils"), TOOLS):
        if p not in sys.path:
            sys.path.insert(0, p)
    from evaluation.pr_helper import PRCalculator
    return PRCalculator


def run_loop(PRCalculator, scans, iou_thresh, class2type, skip_empty):
    """scannet/evaluate_box.py compute_precision_recall with the files' arrays handed in;
    skip_empty False: the `continue` is left out (step mode)"""
    calc = PRCalculator(iou_thresh, class2type)
    counts = []
    for pred, gt in scans:
        # the script's steps in its order: load the pseudo boxes; skip the scan if there are none;
        # predictions (column 6 as read, columns 0-5, np.prod of the size); count them; load the
        # GT; its column 6 -> index in nyu40ids; GT tuples; one step per scan (BC.lists builds
        # the two tuple lists that way)
        if skip_empty and pred.shape[0] == 0:
            continue
        counts.append(pred.shape[0])
        pred_list, gt_list = BC.lists(pred, gt)
        assert len(gt_list) == gt.shape[0]
        calc.step([pred_list], [gt_list])
    with warnings.catch_warnings():                        # np.mean([]) where nothing was predicted
        warnings.simplefilter("ignore")
        avg = np.mean(counts)
        metrics = calc.compute_metrics()
    return calc, metrics, avg, sum(counts)


def pack_of(scans):
    """the scans in the CSR form of include/ov3d_boxeval.h"""
    off = lambda i: np.concatenate([[0], np.cumsum([len(s[i]) for s in scans])]).astype(np.int32)   # noqa: E731
    cls = [np.searchsorted(BC.NYU40, g[:, 6]) for _, g in scans]
    return dict(pred=np.concatenate([p[:, :6].astype(np.float64) for p, _ in scans]).reshape(-1, 6),
                pred_cls=np.concatenate([p[:, 6] for p, _ in scans]).astype(np.int32),
                score=np.concatenate([np.prod(p[:, 3:6], 1).astype(np.float64) for p, _ in scans]),
                pred_off=off(0),
                gt=np.concatenate([g[:, :6].astype(np.float64) for _, g in scans]).reshape(-1, 6),
                gt_cls=np.concatenate(cls).astype(np.int32), gt_off=off(1))


def record(out, tag, PRCalculator, scans, class2type, kind, skip_empty):
    from evaluation.eval_det import eval_det_multiprocessing, get_iou
    used = [s for s in scans if not (skip_empty and s[0].shape[0] == 0)]
    pack = pack_of(used) if used else None
    for thr in BC.THRESHOLDS:
        calc, metrics, avg, total = run_loop(PRCalculator, scans, thr, class2type, skip_empty)
        rec, prec, ap = eval_det_multiprocessing(calc.pred_map_cls, calc.gt_map_cls, ovthresh=thr,
                                                 get_iou_func=get_iou)
        t = f"{tag}/{thr}"
        out[t + "/keys"] = np.array(list(metrics.keys()), dtype=str)
        out[t + "/values"] = np.array([float(v) for v in metrics.values()], np.float64)
        out[t + "/is_int"] = np.array([isinstance(v, int) for v in metrics.values()], np.uint8)
        if skip_empty:
            out[t + "/avg_total"] = np.array([avg, total], np.float64)
        C = 32
        nd, npos, tps = np.zeros(C, np.int32), np.zeros(C, np.int32), np.zeros(C, np.int32)
        if pack is not None:
            nd = np.bincount(pack["pred_cls"], minlength=C).astype(np.int32)
            npos = np.bincount(pack["gt_cls"], minlength=C).astype(np.int32)
        for key in ap:
            c = int(key)
            if isinstance(prec[key], int):
                assert prec[key] == 0 and rec[key] == 0 and ap[key] == 0 and nd[c] == 0, (t, key)
                seen.add("a GT-only class")
                continue
            assert len(prec[key]) == nd[c], (t, key)
            tps[c] = int(round(prec[key][-1] * nd[c]))
            assert prec[key][-1] == tps[c] / nd[c], (t, key)
            if npos[c] == 0:
                assert rec[key][-1] == 0.0
                seen.add("predictions of a class without GT")
            if kind == "curve":
                out[f"{t}/rec/{c}"], out[f"{t}/prec/{c}"], out[f"{t}/ap/{c}"] = rec[key], prec[key], np.float64(ap[key])
        out[t + "/nd"], out[t + "/npos"], out[t + "/tp"] = nd, npos, tps
        if pack is None:
            assert np.isnan(metrics["mPrecision"]) and np.isnan(metrics["AR"]) and len(metrics) == 2
            seen.add("no scan at all")
            continue
        # the closed form against the reference, and the margins
        m = R.match(pack["pred"], pack["pred_cls"], pack["score"], pack["pred_off"], pack["gt"],
                    pack["gt_cls"], pack["gt_off"], BC.THRESHOLDS)
        ntp = R.tally(pack["pred_cls"], pack["gt_cls"], m["best"], [thr], C)[2][0]
        assert np.array_equal(ntp, tps), (t, "closed-form TP totals", ntp, tps)
        ti = BC.THRESHOLDS.index(thr)
        assert np.array_equal(np.bincount(pack["pred_cls"], weights=m["tp"][ti], minlength=C).astype(np.int32), tps)
        ov = m["ovmax"][np.isfinite(m["ovmax"])]
        for th in BC.THRESHOLDS:
            assert ((ov == th) | (np.abs(ov - th) >= MARGIN)).all(), (t, "an ovmax within the margin of", th)
            if (ov == th).any():
                seen.add("an IoU equal to a threshold")
        if kind == "curve":
            for c in np.unique(pack["pred_cls"]):
                sc = pack["score"][pack["pred_cls"] == c]
                assert len(np.unique(sc)) == len(sc), (t, "equal scores in class", c)
        else:
            for s in range(len(used)):
                p0, p1 = pack["pred_off"][s], pack["pred_off"][s + 1]
                pairs = set()
                for c, v in zip(pack["pred_cls"][p0:p1], pack["score"][p0:p1]):
                    if (c, v) in pairs:
                        seen.add("equal volumes within a scan and class")
                    pairs.add((c, v))
        situations(m, pack, used, metrics)
    return metrics


def situations(m, pack, used, metrics):
    if np.isnan(metrics["mPrecision"]):
        seen.add("no predictions at all")
    if any(len(p) == 0 for p, _ in used):
        seen.add("a scan without predictions")
    if any(len(g) == 0 for _, g in used):
        seen.add("a scan without GT")
    if (m["ovmax"] == 1.0).any():
        seen.add("identical boxes")
    if (pack["pred"][:, 3:6] == 0).any():
        seen.add("a zero-size prediction")
    if len({p.dtype for p, _ in used}) > 1:
        seen.add("float32 and float64 files")
    for j in range(len(pack["gt"])):
        cl = np.nonzero(m["jmax"] == j)[0]
        if len(cl) > 1 and pack["score"][cl[np.argmax(m["ovmax"][cl])]] < pack["score"][cl].max():
            seen.add("several claimants, the best IoU not the best score")
    # two GT boxes at the same (largest) IoU, and boxes that touch
    for s in range(len(used)):
        p0, p1, g0, g1 = pack["pred_off"][s], pack["pred_off"][s + 1], pack["gt_off"][s], pack["gt_off"][s + 1]
        if p1 == p0 or g1 == g0:
            continue
        iou = R.ious(pack["pred"][p0:p1], pack["gt"][g0:g1])
        same = pack["pred_cls"][p0:p1, None] == pack["gt_cls"][None, g0:g1]
        top = np.where(same, iou, -1).max(1, keepdims=True)
        if ((np.where(same, iou, -1) == top) & (top > 0)).sum(1).max() > 1:
            seen.add("two GT boxes at equal IoU")
        hp, lp = pack["pred"][p0:p1, None, :3] + pack["pred"][p0:p1, None, 3:6] / 2, \
            pack["pred"][p0:p1, None, :3] - pack["pred"][p0:p1, None, 3:6] / 2
        hg, lg = pack["gt"][None, g0:g1, :3] + pack["gt"][None, g0:g1, 3:6] / 2, \
            pack["gt"][None, g0:g1, :3] - pack["gt"][None, g0:g1, 3:6] / 2
        m_, x_ = np.minimum(hp, hg), np.maximum(lp, lg)
        if ((m_ >= x_).all(-1) & (m_ == x_).any(-1) & same & (pack["pred"][p0:p1, None, 3:6] > 0).all(-1)).any():
            seen.add("touching boxes")


CHECKS = ("a scan without predictions", "a scan without GT", "predictions of a class without GT",
          "a GT-only class", "no predictions at all", "no scan at all",
          "several claimants, the best IoU not the best score", "two GT boxes at equal IoU",
          "an IoU equal to a threshold", "touching boxes", "identical boxes", "a zero-size prediction",
          "float32 and float64 files", "equal volumes within a scan and class")


def main():
    PRCalculator = reference()
    out = {}
    for name in BC.CASES:
        scans, class2type, kind = BC.case(name)
        for mode, skip in (("step", False), ("loop", True)):
            metrics = record(out, f"{name}/{mode}", PRCalculator, scans, class2type, kind, skip)
        print(name, len(scans), "scans,", sum(len(p) for p, _ in scans), "predictions,",
              sum(len(g) for _, g in scans), "GT boxes; last dict:", len(metrics), "keys")
    missing = [c for c in CHECKS if c not in seen]
    assert not missing, ("the cases do not hold", missing)
    assert any(k.endswith("Precision") and k[0].isalpha() and k != "mPrecision" for n in out if n.endswith("/keys")
               for k in out[n]) and any(k[0].isdigit() for n in out if n.endswith("/keys") for k in out[n])
    path = os.path.join(HERE, "box_eval.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
