"""numpy restatement of csrc/boxeval.hip (include/ov3d_boxeval.h): the same operation order in
float64, the same tie rules, the same outputs.  Also the reference's precision / recall curve
(eval_det_cls's cumulative sums and voc_ap) from the per-detection flags, for the tests."""
import numpy as np

FREE = 2 ** 31 - 1
EPS = np.finfo(np.float64).eps


def ious(pred, gt):
    """(p,g) calc_iou + get_iou of every pair; pred, gt (n,>=6) float64 centre, size"""
    hp, lp = pred[:, :3] + pred[:, 3:6] / 2, pred[:, :3] - pred[:, 3:6] / 2
    hg, lg = gt[:, :3] + gt[:, 3:6] / 2, gt[:, :3] - gt[:, 3:6] / 2
    vp, vg = (pred[:, 3] * pred[:, 4]) * pred[:, 5], (gt[:, 3] * gt[:, 4]) * gt[:, 5]
    m = np.minimum(hp[:, None], hg[None])
    x = np.maximum(lp[:, None], lg[None])
    d = m - x
    inter = (d[..., 0] * d[..., 1]) * d[..., 2]
    with np.errstate(all="ignore"):
        iou = np.where((m > x).all(-1), inter / ((vp[:, None] + vg[None]) - inter), 0.0)
    iou = np.where(iou < 0.0, 0.0, iou)
    return np.where(iou > 1.0, 1.0, iou)


def match(pred, pred_cls, score, pred_off, gt, gt_cls, gt_off, thr):
    """ov3d_boxeval_match -> dict rank, jmax, ovmax (P); best (G); owner (T,G); tp (T,P)"""
    pred, gt = np.asarray(pred, np.float64), np.asarray(gt, np.float64)     # (P,>=6), (G,>=6)
    thr = np.asarray(thr, np.float64)
    P, G, T = len(pred), len(gt), len(thr)
    rank, jmax = np.zeros(P, np.int32), np.full(P, -1, np.int32)
    ovmax, best = np.full(P, -np.inf), np.full(G, -np.inf)
    owner, tp = np.full((T, G), FREE, np.int32), np.zeros((T, P), np.uint8)
    for s in range(len(pred_off) - 1):
        p0, p1, g0, g1 = pred_off[s], pred_off[s + 1], gt_off[s], gt_off[s + 1]
        n = p1 - p0
        if n == 0:
            continue
        order = np.lexsort((np.arange(n), -score[p0:p1]))      # score descending, row ascending
        r = np.empty(n, np.int32)
        r[order] = np.arange(n, dtype=np.int32)
        rank[p0:p1] = r
        if g1 == g0:
            continue
        iou = ious(pred[p0:p1], gt[g0:g1])
        ok = (pred_cls[p0:p1, None] == gt_cls[None, g0:g1]) & ~np.isnan(iou)
        iou = np.where(ok, iou, -np.inf)
        jm = np.argmax(iou, 1)                                 # the first maximum
        has = ok.any(1)
        ov = np.where(has, iou[np.arange(n), jm], -np.inf)
        jm = np.where(has, g0 + jm, -1).astype(np.int32)
        jmax[p0:p1], ovmax[p0:p1] = jm, ov
        for i in np.nonzero(has)[0]:
            j = jm[i]
            best[j] = max(best[j], ov[i])
            hit = ov[i] > thr
            owner[hit, j] = np.minimum(owner[hit, j], r[i])
        for i in np.nonzero(has)[0]:
            tp[:, p0 + i] = (ov[i] > thr) & (owner[:, jm[i]] == r[i])
    return dict(rank=rank, jmax=jmax, ovmax=ovmax, best=best, owner=owner, tp=tp)


def tally(pred_cls, gt_cls, best, thr, C):
    """ov3d_boxeval_tally -> nd (C), npos (C), ntp (T,C) int32"""
    thr = np.asarray(thr, np.float64)
    inside = lambda c: c[(c >= 0) & (c < C)]                     # noqa: E731
    nd = np.bincount(inside(np.asarray(pred_cls, np.int64)), minlength=C).astype(np.int32)
    npos = np.bincount(inside(np.asarray(gt_cls, np.int64)), minlength=C).astype(np.int32)
    ntp = np.zeros((len(thr), C), np.int32)
    g = np.asarray(gt_cls, np.int64)
    for t, th in enumerate(thr):
        ntp[t] = np.bincount(inside(g[np.asarray(best) > th]), minlength=C)
    return nd, npos, ntp


def run(pack, thr, C, flags=False):
    """stands in for the two launches of ov3d_amd.box_eval.run_device on a host pack"""
    m = match(pack["pred"], pack["pred_cls"], pack["score"], pack["pred_off"], pack["gt"],
              pack["gt_cls"], pack["gt_off"], thr)
    nd, npos, ntp = tally(pack["pred_cls"], pack["gt_cls"], m["best"], thr, C)
    out = dict(nd=nd, npos=npos, ntp=ntp)
    if flags:
        out.update(tp=m["tp"], ovmax=m["ovmax"])
    return out


def voc_ap(rec, prec):
    """the area under the precision envelope (eval_det.voc_ap, use_07_metric False)"""
    mrec = np.concatenate(([0.0], rec, [1.0]))
    mpre = np.concatenate(([0.0], prec, [0.0]))
    for i in range(mpre.size - 1, 0, -1):
        mpre[i - 1] = np.maximum(mpre[i - 1], mpre[i])
    i = np.where(mrec[1:] != mrec[:-1])[0]
    return np.sum((mrec[i + 1] - mrec[i]) * mpre[i + 1])


def curve(score, tp, npos):
    """rec, prec, ap of one class from its detections in (scan, row) order: global descending
    score, equal scores in the given order"""
    order = np.argsort(-np.asarray(score, np.float64), kind="stable")
    t = np.cumsum(np.asarray(tp, np.float64)[order])
    f = np.cumsum(1.0 - np.asarray(tp, np.float64)[order])
    rec = t / np.maximum(float(npos), EPS)
    prec = t / np.maximum(t + f, EPS)
    return rec, prec, voc_ap(rec, prec)
