"""Golden outputs of the REFERENCE evaluation at proposal counts past the small kernels' caps
and with the 2D NMS (utils/ap_calculator.py, utils/eval_det.py, utils/nms.py).  Run where the
reference exists:

    python tests/golden/make_eval_large_golden.py   # -> evaldet_large.npz, nms_large.npz

evaldet_large.npz: per config of eval_large_cases.CONFIGS the in-hull point counts (where the
config removes empty boxes), the parse_predictions detections (valid boxes, per-class scores)
and compute_metrics() at IoU 0.25 / 0.5, as make_eval_golden.py records them.
nms_large.npz: the reference's pick lists on the box tables of eval_large_cases (3D with
K = 513 / 1100 / 2048: nms_3d_faster_samecls and nms_3d_faster; 2D with K = 37 / 700:
nms_2d_faster), threshold 0.25, both old_type values.

Asserted while it runs, so that the comparison is well-defined from the reference alone: no two
boxes of a scene share a score; every overlap the reference compares with the threshold is
further than 1e-9 from it; every evaluation config keeps >= 20 and suppresses >= 20 boxes per
scene and has mAP@0.25 > 0.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

from ref_loader import load_reference  # noqa: E402
from eval_large_cases import (CONFIGS, MARGIN, NMS2D_K, NMS3D_K, NMS_THRESHOLD, make_batches,  # noqa: E402
                              nms2d_table, nms3d_table)
from make_eval_golden import detections_from_lists  # noqa: E402


def check_margin(table, picks, thr, old_type, samecls):
    """Replay the greedy loop along the reference's own pick list: every overlap it compares
    with thr is > MARGIN away from it, and the replay picks what the reference picked.
    table (n, 7|8) [x1,y1,z1,x2,y2,z2,score(,cls)]; -> number of suppressed rows."""
    score = table[:, 6]
    assert np.unique(score).size == score.size, "two boxes share a score"
    lo, hi = table[:, 0:3], table[:, 3:6]
    vol = (hi[:, 0] - lo[:, 0]) * (hi[:, 1] - lo[:, 1]) * (hi[:, 2] - lo[:, 2])
    left = list(np.argsort(score))
    mine = []
    while left:
        i = left.pop()
        mine.append(i)
        rest = np.array(left, dtype=np.int64)
        d = np.maximum(0, np.minimum(hi[i], hi[rest]) - np.maximum(lo[i], lo[rest]))
        inter = d[:, 0] * d[:, 1] * d[:, 2]
        o = inter / vol[rest] if old_type else inter / (vol[i] + vol[rest] - inter)
        if samecls:
            o = o * (table[i, 7] == table[rest, 7])
        assert np.isfinite(o).all()
        assert (np.abs(o - thr) > MARGIN).all(), ("an overlap within the margin of the threshold",
                                                  float(np.abs(o - thr).min()))
        left = [j for j, drop in zip(left, o > thr) if not drop]
    assert mine == [int(p) for p in picks], "the replay disagrees with the reference"
    return table.shape[0] - len(mine)


def lift2d(t):
    out = np.zeros((t.shape[0], 7))
    out[:, [0, 2, 3, 5, 6]] = t[:, [0, 1, 2, 3, 4]]
    out[:, 4] = 1.0
    return out


def gen_nms(nms):
    out = {}
    for i in range(len(NMS3D_K)):
        boxes = nms3d_table(i)
        out[f"boxes{i}"] = boxes
        for old in (False, True):
            same = nms.nms_3d_faster_samecls(boxes, NMS_THRESHOLD, old)
            anyc = nms.nms_3d_faster(boxes[:, :7], NMS_THRESHOLD, old)
            ns = check_margin(boxes, same, NMS_THRESHOLD, old, True)
            na = check_margin(boxes[:, :7], anyc, NMS_THRESHOLD, old, False)
            assert min(len(same), len(anyc), ns, na) >= 20, (len(same), len(anyc), ns, na)
            out[f"samecls{i}_{int(old)}"] = np.array(same, np.int32)
            out[f"any{i}_{int(old)}"] = np.array(anyc, np.int32)
            print(f"3D K={boxes.shape[0]} old={int(old)}: kept {len(same)} / {len(anyc)}, "
                  f"suppressed {ns} / {na}")
    for i in range(len(NMS2D_K)):
        boxes = nms2d_table(i)
        out[f"boxes2d{i}"] = boxes
        for old in (False, True):
            pick = nms.nms_2d_faster(boxes, NMS_THRESHOLD, old)
            n2 = check_margin(lift2d(boxes), pick, NMS_THRESHOLD, old, False)
            assert len(pick) >= 5 and n2 >= 5, (len(pick), n2)
            out[f"nms2d{i}_{int(old)}"] = np.array(pick, np.int32)
            print(f"2D K={boxes.shape[0]} old={int(old)}: kept {len(pick)}")
    np.savez_compressed(os.path.join(HERE, "nms_large.npz"), **out)
    print("wrote nms_large.npz", len(out))


def nms_table(corners, obj, cls, conf):
    """the table parse_predictions hands its NMS for one scene (ap_calculator.py:89-190)"""
    lo, hi = corners.min(1).astype(np.float64), corners.max(1).astype(np.float64)
    if not conf["use_3d_nms"]:
        return lift2d(np.stack([lo[:, 0], lo[:, 2], hi[:, 0], hi[:, 2], obj.astype(np.float64)], 1))
    return np.concatenate([lo, hi, obj[:, None].astype(np.float64), cls[:, None].astype(np.float64)], 1)


def gen_eval(apc, bu, ref_nms):
    import torch
    out = {}
    for name, cfg in CONFIGS.items():
        batches = make_batches(**cfg["data"])
        C = cfg["data"]["num_classes"]

        class Cfg:
            num_semcls = C
        conf = apc.get_ap_config_dict(dataset_config=Cfg(), **cfg["ap"])
        calc = apc.APCalculator(Cfg(), ap_iou_thresh=[0.25, 0.5], class2type_map=None,
                                ap_config_dict=conf)
        for bi, bt in enumerate(batches):
            corners = bt["pred_corners"]
            B, K = corners.shape[:2]
            nonempty = np.ones((B, K), bool)
            if conf["remove_empty_box"]:
                cnt = np.zeros((B, K), np.int32)
                for i in range(B):
                    for j in range(K):
                        box = apc.flip_axis_to_depth(corners[i, j])
                        cnt[i, j] = len(bu.extract_pc_in_box3d(bt["point_clouds"][i], box)[0])
                out[f"{name}/b{bi}/counts"] = cnt
                nonempty = cnt >= 5
                assert nonempty.any(1).all()
            args = [torch.from_numpy(bt[k]) for k in ("pred_corners", "sem_cls_prob", "objectness_prob",
                                                      "point_clouds")]
            # pred_mask is not returned: the NMS survivors are the boxes above the confidence
            # threshold that come back as detections, plus the picks below it (replayed)
            lists = apc.parse_predictions(*args, conf)
            valid, scores = detections_from_lists(lists, corners, C)
            out[f"{name}/b{bi}/valid"] = valid
            out[f"{name}/b{bi}/scores"] = scores
            cls = np.argmax(bt["sem_cls_prob"], -1)
            samecls = bool(conf["use_3d_nms"] and conf["cls_nms"])
            for i in range(B):
                idx = np.where(nonempty[i])[0]
                tab = nms_table(corners[i], bt["objectness_prob"][i], cls[i], conf)[idx]
                if not conf["use_3d_nms"]:
                    pick = ref_nms.nms_2d_faster(tab[:, [0, 2, 3, 5, 6]], conf["nms_iou"],
                                                 conf["use_old_type_nms"])
                elif samecls:
                    pick = ref_nms.nms_3d_faster_samecls(tab, conf["nms_iou"], conf["use_old_type_nms"])
                else:
                    pick = ref_nms.nms_3d_faster(tab[:, :7], conf["nms_iou"], conf["use_old_type_nms"])
                dropped = check_margin(tab, pick, conf["nms_iou"], conf["use_old_type_nms"], samecls)
                kept = np.zeros(K, bool)
                kept[idx[pick]] = True
                assert np.array_equal(kept & (bt["objectness_prob"][i] > conf["conf_thresh"]), valid[i])
                assert len(pick) >= 20 and dropped >= 20, (name, i, len(pick), dropped)
                print(f"{name} scene {i}: {idx.size} in, kept {len(pick)}, suppressed {dropped}")
            calc.step(*args, torch.from_numpy(bt["gt_box_corners"]),
                      torch.from_numpy(bt["gt_box_sem_cls_label"]), torch.from_numpy(bt["gt_box_present"]))
        met = calc.compute_metrics()
        assert met[0.25]["mAP"] > 0
        for th, d in met.items():
            for k, v in d.items():
                out[f"{name}/metrics/{th}/{k}"] = np.asarray(v)
        print(name, {th: (float(d["mAP"]), float(d["AR"])) for th, d in met.items()})
    np.savez_compressed(os.path.join(HERE, "evaldet_large.npz"), **out)
    print("wrote evaldet_large.npz", len(out))


if __name__ == "__main__":
    load_reference()
    import utils.ap_calculator as ref_apc
    import utils.box_util as ref_bu
    import utils.nms as ref_nms
    gen_nms(ref_nms)
    gen_eval(ref_apc, ref_bu, ref_nms)
