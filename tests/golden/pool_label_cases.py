"""Deterministic cases for the pool labelling (assign_box_label_from_gt.py labeling) and the
pseudo-label assessment (assess_pseudo_label.py match).  make_pool_label_golden.py runs the
reference's own functions over them and asserts that each case decides what it is meant to;
the tests build the same arrays again and compare with what was recorded.

A labelling case is a scan of eight octants of 2 m, one ground-truth label each, with 12 % of
the vertices relabelled at random, a pool of random boxes, and hand-placed vertices and boxes
far from the octants, one group per property (every coordinate there is a small dyadic number,
so cs2vv's lo = c - s/2 and hi = s + lo are exact):
  x = 10  a tie between labels 4 and 5 (the smaller wins), and between 13 and 16
  x = 12  labels 0..2 in the majority: the vote from 3 up elects 7, a vote from 0 would elect 1
  x = 14  vertices exactly on the lower and on the upper bound (closed interval)
  x = 16  nothing but labels 0..2 (no vote), and an empty box
  x = 18  label 13 only (the mode is not in nyu40ids)
  x = 20  float32 vertices with a bound one float64 ulp outside and one inside, on either side
"""
import os

import numpy as np

NYU40 = np.array([3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14, 16, 24, 28, 33, 34, 36, 39])
LABEL_CASES = ("f32", "f64")           # every generator assertion holds for these
SHAPE_CASES = ("none", "one")          # the (0, 7) and the (1, 7) file
ASSESS_CASES = ("a", "b")
OCTANT_LABELS = {"f32": [3, 13, 5, 1, 39, 20, 8, 2], "f64": [36, 2, 21, 4, 0, 12, 40, 33]}
ULP_X = np.float32(20.3)               # not a dyadic number with few bits: a generic float32


def ulp_bounds():
    """the four bounds one float64 ulp from ULP_X: (above, below) of the vertex"""
    v = np.float64(ULP_X)
    return np.nextafter(v, np.inf), np.nextafter(v, -np.inf)


def _unit_box(lo, hi=None):
    """pool row whose cs2vv form has lower corner lo (size 1) or upper corner hi (size 1):
    exact where lo, lo + 0.5 and lo + 1 share a binade"""
    lo = np.asarray(lo if hi is None else np.asarray(hi, np.float64) - 1.0, np.float64)
    return np.concatenate([lo + 0.5, [1.0, 1.0, 1.0], [-1.0]])


def _special(dtype):
    """hand-placed vertices (xyz, label) and pool rows"""
    pts, lab, pool = [], [], []

    def put(xyz, label):
        pts.append(xyz)
        lab.append(label)

    def box(c, s):
        pool.append(list(c) + list(s) + [-1.0])

    # ties: 2 x label 5, 2 x label 4 -> 4; 1 x 16, 1 x 13 -> 13 (not a detection class: dropped)
    for k, l in enumerate((5, 4, 5, 4)):
        put((10.25 + 0.125 * k, 0.5, 0.5), l)
    box((10.5, 0.5, 0.5), (1.0, 0.5, 0.5))
    put((10.25, 4.5, 0.5), 16)
    put((10.5, 4.5, 0.5), 13)
    box((10.5, 4.5, 0.5), (1.0, 0.5, 0.5))
    # labels below 3 in the majority
    for k, l in enumerate((1, 1, 1, 1, 1, 7, 7, 9, 2, 0)):
        put((12.0 + 0.0625 * k, 0.25, 0.75), l)
    box((12.5, 0.25, 0.75), (1.5, 0.25, 0.25))
    # on the bounds: box [14, 15] x [1, 2] x [2, 3]; a vertex on each face, one just outside
    put((14.0, 1.5, 2.5), 6)
    put((15.0, 1.5, 2.5), 6)
    put((14.5, 1.0, 3.0), 6)
    put((15.125, 1.5, 2.5), 8)
    put((14.5, 0.875, 2.5), 8)
    box((14.5, 1.5, 2.5), (1.0, 1.0, 1.0))
    # no vote
    for k, l in enumerate((0, 1, 2, 2)):
        put((16.25 + 0.125 * k, 0.5, 0.5), l)
    box((16.5, 0.5, 0.5), (1.0, 0.5, 0.5))
    box((16.5, 6.5, 0.5), (0.5, 0.5, 0.5))                  # nothing inside
    # a label that is no detection class
    for k in range(3):
        put((18.25 + 0.125 * k, 0.5, 0.5), 13)
    put((18.5, 0.625, 0.5), 3)
    box((18.5, 0.5, 0.5), (1.0, 0.5, 0.5))
    # one float64 ulp from a float32 vertex, four boxes with one vertex each (y = 0, 2, 4, 6)
    above, below = ulp_bounds()
    for y, bound, side in ((0.0, above, "lo"), (2.0, below, "hi"), (4.0, below, "lo"), (6.0, above, "hi")):
        put((ULP_X, y + 20.5, 20.5), 10)
        corner = np.array([bound, y + 20.0, 20.0]) if side == "lo" else np.array([bound, y + 21.0, 21.0])
        pool.append(_unit_box(corner) if side == "lo" else _unit_box(None, corner))
    return np.array(pts, dtype), np.array(lab, np.int64), np.array(pool, np.float64)


def label_case(name):
    """-> dict(points (N, 3) float32 / float64, labels (N) int64, pool (P, 7) float64)"""
    if name in SHAPE_CASES:
        pts = np.array([[0.5, 0.5, 0.5], [0.25, 0.5, 0.5], [4.5, 0.5, 0.5]], np.float32)
        lab = np.array([7, 7, 13], np.int64)
        pool = np.array([[4.5, 0.5, 0.5, 0.5, 0.5, 0.5, -1.0], [9.0, 9.0, 9.0, 1.0, 1.0, 1.0, -1.0],
                         [0.5, 0.5, 0.5, 1.0, 1.0, 1.0, -1.0]], np.float64)
        if name == "none":
            pool = pool[:2]
        return dict(points=pts, labels=lab, pool=pool)
    dtype = np.float32 if name == "f32" else np.float64
    rng = np.random.Generator(np.random.PCG64(7 if name == "f32" else 8))
    n = 2500 if name == "f32" else 1800
    pts = rng.uniform(0.0, 4.0, (n, 3)).astype(dtype)
    octant = (pts[:, 0] >= 2) * 4 + (pts[:, 1] >= 2) * 2 + (pts[:, 2] >= 2) * 1
    lab = np.array(OCTANT_LABELS[name], np.int64)[octant]
    noise = rng.random(n) < 0.12
    lab[noise] = rng.integers(0, 41, int(noise.sum()))
    k = 44 if name == "f32" else 31
    centre = rng.uniform(0.3, 3.7, (k, 3))
    size = rng.uniform(0.2, 1.2, (k, 3))
    pool = np.concatenate([centre, size, np.full((k, 1), -1.0)], 1)
    spts, slab, spool = _special(dtype)
    order = rng.permutation(k + len(spool))                  # the hand-placed boxes among the others
    perm = rng.permutation(n + len(spts))
    return dict(points=np.concatenate([pts, spts])[perm], labels=np.concatenate([lab, slab])[perm],
                pool=np.concatenate([pool, spool])[order])


def assess_case(name):
    """-> dict(frame_ids [int], gt (F, H, W) float32 nyu40 ids as load_label returns them,
    pseudo (F, H, W) int16 LSeg indices: classes, values >= 18 and a few -100)"""
    rng = np.random.Generator(np.random.PCG64(21 if name == "a" else 22))
    F, H, W = (3, 24, 32) if name == "a" else (2, 15, 21)
    ids = [0, 20, 100][:F]
    bh, bw = -(-H // 3), -(-W // 4)

    def blocks(hi):
        """blocks of 3 x 4 pixels of one label, as a segmentation has runs; every label occurs"""
        vals = np.concatenate([np.arange(hi), rng.integers(0, hi, F * bh * bw - hi)])
        return np.kron(rng.permutation(vals).reshape(F, bh, bw), np.ones((1, 3, 4), np.int64))[:, :H, :W]
    gt = blocks(41)
    true_cls = np.full(41, 18)
    true_cls[NYU40] = np.arange(18)
    pseudo = np.where(rng.random((F, H, W)) < 0.6, true_cls[gt], blocks(22))             # 18 .. 21: ignored
    pseudo[:, 0, :5] = -100
    return dict(frame_ids=ids, gt=gt.astype(np.float32), pseudo=pseudo.astype(np.int16))


def write_label_tree(case, root, scan):
    """the files PoolLabeler (and the reference script) reads -> (vert_dir, label_dir, pool_dir)"""
    dirs = [os.path.join(root, d) for d in ("det", "det", "gss")]
    for d in dirs:
        os.makedirs(d, exist_ok=True)
    extra = np.full((len(case["points"]), 3), 127, case["points"].dtype)                 # the colour columns
    np.save(os.path.join(dirs[0], scan + "_vert.npy"), np.concatenate([case["points"], extra], 1))
    np.save(os.path.join(dirs[1], scan + "_sem_label.npy"), case["labels"])
    np.save(os.path.join(dirs[2], scan + "_prop.npy"), case["pool"])
    return dirs
