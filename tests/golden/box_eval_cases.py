"""Cases of the pseudo-box evaluation (tests/golden/box_eval.npz, make_box_eval_golden.py), as
plain numpy data.  A case is a list of scans; a scan is (pred, gt): pred (k,7) centre, size,
class index in the dtype of its file, gt (g,7) centre, size, nyu40 id.

`step` mode hands every scan to PRCalculator.step; `loop` mode is the script's file loop, which
skips a scan without predictions together with its GT."""
import os

import numpy as np

NYU40 = np.array([3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14, 16, 24, 28, 33, 34, 36, 39])
NAMES = ["cabinet", "bed", "chair", "sofa", "table", "door", "window", "bookshelf", "picture", "counter",
         "desk", "curtain", "refrigerator", "shower curtain", "toilet", "sink", "bathtub", "other furniture"]
CLASS2TYPE = dict(enumerate(NAMES))
THRESHOLDS = (0.25, 0.5)

# name -> (scans builder, class2type_map or None, kind): "metric" cases may hold equal scores
# within a class, "curve" cases have distinct scores per class and pin rec / prec / ap too
CASES = ("quirks", "quirks_named", "no_predictions", "ties_f32", "ties_f64", "curve", "curve_named")


def _pred(rows, dtype=np.float64):
    return np.array(rows, dtype=dtype).reshape(-1, 7)


def _gt(rows, dtype=np.float64):
    g = np.array(rows, dtype=np.float64).reshape(-1, 7)
    g[:, 6] = NYU40[g[:, 6].astype(int)]
    return g.astype(dtype)


def quirks():
    s0_gt = _gt([[0, 0, 0, 1, 1, 1, 2],          # A
                 [5, 0, 0, 1, 1, 1, 2],          # B
                 [0, 5, 0, 1, 1, 1, 4],          # C
                 [1, 5, 0, 1, 1, 1, 4],          # E: beside C
                 [9, 9, 9, 1, 2, 1, 7]])         # a class only GT has
    s0_pred = _pred([[0, 0, 0, 1, 1, 1, 2],      # identical to A: IoU 1.0 exactly
                     [0, 0, 1.5, 1, 1, 4, 2],    # contains A: 1 / 4 = 0.25 exactly, no TP at 0.25
                     [5.75, 0, 0, 2.5, 1, 1, 2],  # claims B at IoU 0.4 with the best score
                     [5.1, 0, 0, 1.2, 1, 1, 2],  # claims B at IoU 1 / 1.2 with a lower score
                     [0.5, 5, 0, 1, 1, 1, 4],    # C and E at IoU 1 / 3 each: the first wins
                     [1, 5, 0, 1, 1, 1, 4],      # identical to E
                     [2, 5, 0, 1, 1, 1, 4],      # touches E: 0
                     [0, 0, 0, 0, 1, 1, 2],      # zero size
                     [3, 3, 3, 1, 1, 2, 10],     # a class without GT anywhere
                     [0.125, 0, 0, 1, 1, 1, 2]])  # A again, same volume as the first row
    s1 = (_pred([]), _gt([[0, 0, 0, 1, 1, 1, 2], [2, 2, 2, 1, 1, 1, 7]]))          # no predictions
    s2 = (_pred([[0, 0, 0, 1, 1, 1, 2], [1, 1, 1, 2, 1, 1, 4]], np.float32), _gt([]))   # no GT
    s3_gt = _gt([[0, 0, 0, 2, 2, 2, 2], [4, 0, 0, 1, 1, 1, 14]], np.float32)
    s3_pred = _pred([[0.25, 0, 0, 2, 2, 2, 2],   # equal volumes within the class, both claim one box
                     [0, 0.125, 0, 2, 2, 2, 2],
                     [4, 0, 0.125, 1, 1, 1, 14],
                     [4.5, 0, 0, 1, 1, 1, 14]], np.float32)
    return [(s0_pred, s0_gt), s1, s2, (s3_pred, s3_gt)]


def no_predictions():
    return [(_pred([]), _gt([[0, 0, 0, 1, 1, 1, 2], [2, 2, 2, 1, 1, 1, 7]])),
            (_pred([], np.float32), _gt([[1, 0, 0, 1, 1, 1, 2]]))]


def random_scans(seed, dtype, distinct, n_scans=6, n_cls=5):
    """GT boxes on a 1/8 grid and predictions that are jittered copies of them, so that many
    claim one GT box and (unless distinct) many volumes are equal.  distinct: every size x gets
    its own multiple of 2^-10 added, which float32 holds exactly."""
    rng = np.random.Generator(np.random.PCG64(seed))
    scans, serial = [], 0
    for s in range(n_scans):
        g = int(rng.integers(1, 7))
        centre = rng.integers(-16, 17, (g, 3)) / 8.0 + np.arange(g)[:, None] * [3.0, 0, 0]
        size = rng.integers(4, 13, (g, 3)) / 8.0
        cls = rng.integers(0, n_cls, g)
        gt = np.concatenate([centre, size, cls[:, None]], 1)
        k = int(rng.integers(0 if s == 2 else 2, 12))
        src = rng.integers(0, g, k)
        pc = centre[src] + rng.integers(-2, 3, (k, 3)) / 8.0
        ps = size[src] + rng.integers(-1, 2, (k, 3)) / 8.0
        pcls = np.where(rng.random(k) < 0.8, cls[src], rng.integers(0, n_cls + 1, k))
        if distinct:
            ps[:, 0] += (serial + np.arange(k) + 1) * 2.0 ** -10
            serial += k
        scans.append((_pred(np.concatenate([pc, ps, pcls[:, None]], 1), dtype if s % 2 else np.float64),
                      _gt(gt, np.float64 if s % 3 else np.float32)))
    return scans


def case(name):
    """-> (scans, class2type_map, kind)"""
    if name.startswith("quirks"):
        return quirks(), CLASS2TYPE if name.endswith("named") else None, "metric"
    if name == "no_predictions":
        return no_predictions(), None, "metric"
    if name.startswith("ties"):
        return random_scans(11, np.float32 if name.endswith("f32") else np.float64, False), None, "metric"
    if name.startswith("curve"):
        return random_scans(23, np.float32, True), CLASS2TYPE if name.endswith("named") else None, "curve"
    raise KeyError(name)


def scan_name(i):
    return "scene%04d_00" % i


def write_tree(scans, root):
    """the two directories of <scan>_bbox.npy files -> (scan names, box_dir, gt_dir)"""
    box_dir, gt_dir = os.path.join(root, "pseudo"), os.path.join(root, "gt")
    os.makedirs(box_dir)
    os.makedirs(gt_dir)
    for i, (pred, gt) in enumerate(scans):
        np.save(os.path.join(box_dir, scan_name(i) + "_bbox.npy"), pred)
        np.save(os.path.join(gt_dir, scan_name(i) + "_bbox.npy"), gt)
    return [scan_name(i) for i in range(len(scans))], box_dir, gt_dir


def lists(pred, gt):
    """one scan as the tuple lists of evaluate_box.py's loop"""
    cls = [np.where(NYU40 == x)[0][0] for x in gt[:, 6]]
    return ([(pred[j, 6], pred[j, :6], np.prod(pred[j, 3:6])) for j in range(len(pred))],
            [(cls[j], gt[j, :6]) for j in range(len(gt))])
