"""Device evaluation past the small kernels' caps (more than 512 boxes in the NMS, more than 256
proposals or 64 GT boxes in the AP match) and with the 2D NMS, against the REFERENCE
evaluation's own outputs (tests/golden/evaldet_large.npz, made by make_eval_large_golden.py).

Bars, those of test_evaldet_gpu.py: in-hull point counts, detection masks and per-class scores
bit-exact; per-class AP / recall <= 1e-12, mAP (float32) exact, AR <= 1e-12.  The TP / FP
flags of the large AP-match kernel are compared exactly: with a numpy restatement of
eval_det.py:104-131 on synthetic tensors, and with the small kernel at the shapes both take.
"""
import os

import numpy as np
import pytest
import torch

import eval_cases
from eval_large_cases import CONFIGS, make_batches
from ov3d_amd import _native as nat
from ov3d_amd import ap_calculator as apc
from ov3d_amd import nms

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = np.load(os.path.join(HERE, "golden", "evaldet_large.npz"))


class _Cfg:
    def __init__(self, c):
        self.num_semcls = c


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_parse_predictions_equals_reference(name):
    cfg = CONFIGS[name]
    conf = apc.get_ap_config_dict(dataset_config=_Cfg(cfg["data"]["num_classes"]), **cfg["ap"])
    for bi, bt in enumerate(make_batches(**cfg["data"])):
        if conf["remove_empty_box"]:
            cnt = apc.box_points_count(_t(bt["point_clouds"]), _t(bt["pred_corners"])).cpu().numpy()
            assert np.array_equal(cnt, GOLD[f"{name}/b{bi}/counts"]), (bi, np.argwhere(cnt != GOLD[f"{name}/b{bi}/counts"]))
        scores, _ = apc.parse_predictions_device(_t(bt["pred_corners"]), _t(bt["sem_cls_prob"]),
                                                 _t(bt["objectness_prob"]), _t(bt["point_clouds"]), conf)
        sc = scores.cpu().numpy()
        ref = GOLD[f"{name}/b{bi}/scores"]
        assert np.array_equal(np.isfinite(sc).any(-1), GOLD[f"{name}/b{bi}/valid"]), bi
        assert np.array_equal(sc.view(np.uint32), ref.view(np.uint32)), bi


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_compute_metrics_equals_reference(name):
    cfg = CONFIGS[name]
    conf = apc.get_ap_config_dict(dataset_config=_Cfg(cfg["data"]["num_classes"]), **cfg["ap"])
    calc = apc.APCalculator(_Cfg(cfg["data"]["num_classes"]), ap_iou_thresh=[0.25, 0.5],
                            class2type_map=None, ap_config_dict=conf)
    for bt in make_batches(**cfg["data"]):
        calc.step(_t(bt["pred_corners"]), _t(bt["sem_cls_prob"]), _t(bt["objectness_prob"]),
                  _t(bt["point_clouds"]), _t(bt["gt_box_corners"]), _t(bt["gt_box_sem_cls_label"]),
                  _t(bt["gt_box_present"]))
    met = calc.compute_metrics()
    for th, d in met.items():
        pre = f"{name}/metrics/{th}/"
        keys = [k[len(pre):] for k in GOLD.files if k.startswith(pre)]
        assert set(d.keys()) == set(keys)
        for k, v in d.items():
            ref = GOLD[pre + k]
            if k == "mAP":
                assert np.float32(v) == np.float32(ref), (th, v, ref)
            else:
                assert abs(float(v) - float(ref)) <= 1e-12, (th, k, v, ref)
    assert "mAP" in met[0.25] and met[0.25]["mAP"] > 0


# ---------------------------------------------------------------- the TP / FP walk on its own
def _walk(scores, iou, gt_cls, gvalid, thresh):
    """eval_det_cls's TP / FP walk (eval_det.py:104-131) per (scene, class): detections by
    descending confidence (equal ones: lower box index first), each matched to the first GT of
    the class with the largest IoU, a GT counted once"""
    S, K, C = scores.shape
    tp = np.zeros((S, K, C), np.uint8)
    for s in range(S):
        for c in range(C):
            gts = np.where(gvalid[s] & (gt_cls[s] == c))[0]
            ks = [k for k in range(K) if scores[s, k, c] > -np.inf]
            ks.sort(key=lambda k: (-scores[s, k, c], k))
            if not gts.size:
                continue                       # ovmax stays -inf: every detection an FP
            sub = iou[s][:, gts]
            first_max = sub.argmax(1)          # "if overlap > ovmax" scanning upwards: the first
            det = set()
            for k in ks:
                ovmax, jmax = sub[k, first_max[k]], first_max[k]
                if ovmax > thresh and jmax not in det:
                    tp[s, k, c] = 1
                    det.add(jmax)
    return tp


def _ap_match(scores, iou, gt_cls, gvalid, thresh):
    S, K, C = scores.shape
    G = gt_cls.shape[1]
    tp = torch.zeros((S, K, C), dtype=torch.uint8, device="cuda")
    nat.call("ov3d_ap_match", _t(iou), _t(scores), _t(gt_cls), _t(gvalid.astype(np.uint8)), S, K, G, C,
             float(thresh), tp, like=tp)
    return tp.cpu().numpy()


def _synthetic(K, G, seed, S=2, C=3):
    """scores with ties and non-detections, a sparse IoU table on a grid of 1/16 (equal IoUs to
    two GTs, several detections over one GT), class 2 without GT in scene 0, class 1 without a
    detection in scene 1, some GT slots absent"""
    rs = np.random.RandomState(seed)
    scores = (rs.randint(1, 40, (S, K, C)) / 40.0).astype(np.float32)
    scores[rs.rand(S, K, C) < 0.3] = -np.inf
    scores[1, :, 1] = -np.inf
    iou = rs.randint(0, 17, (S, K, G)) / 16.0
    iou[rs.rand(S, K, G) < 0.6] = 0.0
    gt_cls = rs.randint(0, C, (S, G)).astype(np.int64)
    gt_cls[0][gt_cls[0] == 2] = 0
    gvalid = rs.rand(S, G) < 0.8
    return scores, iou, gt_cls, gvalid


@pytest.mark.parametrize("K,G", [(257, 64), (256, 65), (300, 130), (2048, 1024)])
def test_ap_match_large_equals_walk(K, G):
    scores, iou, gt_cls, gvalid = _synthetic(K, G, seed=K + G)
    assert not ((gt_cls[0] == 2) & gvalid[0]).any() and np.isfinite(scores[0, :, 2]).any()
    assert ((gt_cls[1] == 1) & gvalid[1]).any() and not np.isfinite(scores[1, :, 1]).any()
    for th in (0.25, 0.5):
        got = _ap_match(scores, iou, gt_cls, gvalid, th)
        ref = _walk(scores, iou, gt_cls, gvalid, th)
        assert 0 < ref.sum() < np.isfinite(scores).sum()
        assert np.array_equal(got, ref), np.argwhere(got != ref)[:8]
        assert not got[~np.isfinite(scores)].any()


def test_ap_match_large_duplicates_and_equal_ious():
    """three detections of class 0 over GT 1 (the best-scoring is the TP, the others FPs, also
    the one whose IoU is larger); a detection with the same IoU to GT 0 and GT 2 takes GT 0, the
    next such one finds GT 0 taken and is an FP (it is not handed GT 2)"""
    K, G, C = 257, 65, 1
    scores = np.full((1, K, C), -np.inf, np.float32)
    iou = np.zeros((1, K, G))
    gt_cls = np.zeros((1, G), np.int64)
    gvalid = np.zeros((1, G), bool)
    gvalid[0, :3] = True
    scores[0, [10, 200, 256, 5, 6], 0] = [0.5, 0.9, 0.7, 0.4, 0.3]
    iou[0, 10, 1], iou[0, 200, 1], iou[0, 256, 1] = 0.9, 0.6, 0.8
    iou[0, 5, 0] = iou[0, 5, 2] = 0.75
    iou[0, 6, 0] = iou[0, 6, 2] = 0.75
    got = _ap_match(scores, iou, gt_cls, gvalid, 0.5)
    assert np.array_equal(got, _walk(scores, iou, gt_cls, gvalid, 0.5))
    assert got[0, [10, 200, 256, 5, 6], 0].tolist() == [0, 1, 0, 1, 0]
    # equal scores: the lower box index goes first
    scores[0, [10, 200, 256], 0] = 0.5
    got = _ap_match(scores, iou, gt_cls, gvalid, 0.5)
    assert got[0, [10, 200, 256], 0].tolist() == [1, 0, 0]


@pytest.mark.parametrize("name", sorted(eval_cases.CONFIGS))
def test_large_ap_match_equals_small_kernel(name):
    """the six configurations of test_evaldet_gpu.py (K = 64, G = 64): tp of both kernels equal
    byte for byte, from the scores and IoUs the evaluation itself computes"""
    cfg = eval_cases.CONFIGS[name]
    conf = apc.get_ap_config_dict(dataset_config=_Cfg(cfg["data"]["num_classes"]), **cfg["ap"])
    bts = eval_cases.make_batches(**cfg["data"])
    scores = torch.cat([apc.parse_predictions_device(
        _t(bt["pred_corners"]), _t(bt["sem_cls_prob"]), _t(bt["objectness_prob"]),
        _t(bt["point_clouds"]), conf)[0] for bt in bts])
    corners = torch.cat([_t(bt["pred_corners"]) for bt in bts])
    gtc = torch.cat([_t(bt["gt_box_corners"]) for bt in bts])
    gcls = torch.cat([_t(bt["gt_box_sem_cls_label"]) for bt in bts]).to(torch.int64).contiguous()
    gvalid = (torch.cat([_t(bt["gt_box_present"]) for bt in bts]) == 1).to(torch.uint8).contiguous()
    S, K, C = scores.shape
    G = gtc.shape[1]
    assert K <= 256 and G <= 64
    pvalid = torch.isfinite(scores).any(-1).to(torch.uint8).contiguous()
    iou = torch.empty((S, K, G), dtype=torch.float64, device="cuda")
    nat.call("ov3d_box3d_iou_eval", corners.contiguous(), pvalid, gtc.float().contiguous(), gvalid,
             S, K, G, iou, like=scores)
    prev = nms.large_kernels(-1)
    try:
        out = []
        for on in (0, 1):
            nms.large_kernels(on)
            for th in (0.25, 0.5):
                tp = torch.zeros((S, K, C), dtype=torch.uint8, device="cuda")
                nat.call("ov3d_ap_match", iou, scores, gcls, gvalid, S, K, G, C, th, tp, like=scores)
                out.append(tp)
    finally:
        nms.large_kernels(prev)
    assert int(out[0].sum()) > 0
    assert torch.equal(out[0], out[2]) and torch.equal(out[1], out[3])


def test_too_many_boxes_are_refused_in_step():
    """K = 2049 raises in step, before anything is stored, not after the pass in
    compute_metrics; so does G = 1025 (and eval_det_device itself)"""
    calc = apc.APCalculator(_Cfg(3), ap_iou_thresh=[0.25], class2type_map=None, exact_eval=False)

    def step(K, G):
        calc.step(torch.zeros((1, K, 8, 3), device="cuda"), torch.zeros((1, K, 4), device="cuda"),
                  torch.zeros((1, K), device="cuda"), torch.zeros((1, 16, 3), device="cuda"),
                  torch.zeros((1, G, 8, 3), device="cuda"),
                  torch.zeros((1, G), dtype=torch.int64, device="cuda"), torch.zeros((1, G), device="cuda"))
    with pytest.raises(ValueError):
        step(2049, 4)
    with pytest.raises(ValueError):
        step(8, 1025)
    assert calc.scan_cnt == 0 and not calc._scores
    with pytest.raises(ValueError):
        apc.eval_det_device(torch.zeros((1, 8, 3), device="cuda"), torch.zeros((1, 8, 8, 3), device="cuda"),
                            torch.zeros((1, 1025, 8, 3), device="cuda"),
                            torch.zeros((1, 1025), dtype=torch.int64, device="cuda"),
                            torch.zeros((1, 1025), device="cuda"), [0.25])
