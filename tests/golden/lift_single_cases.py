"""Synthetic inputs of the single-view lifting tests (tests/golden/lift_single.npz is what the
reference's scannet/lift_boxes.py makes of them with VIEW = 'single';
make_lift_single_golden.py).

Four 240 x 320 frames (the size the reference hard-codes): label maps with rectangles of a
class on a background of ignored values (18 and up) and of class 4, which no box names; uint16
depth in millimetres, flat per rectangle plus noise; cameras looking at a common room.  A 2D
box lifts every pixel of its frame that carries its label, so the boxes below are told apart
by (frame, label) only; their rectangles are arbitrary.  Every decision of the chain is far
from its threshold for these inputs; the generator asserts the margins and that no stage is
trivial.
"""
import os

import numpy as np

import lift_cases as LC

H, W = 240, 320
NYU40 = np.array([3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14, 16, 24, 28, 33, 34, 36, 39])
BACKGROUND = (18, 19, 25, 40, 4)
BACKGROUND_NYU = {18: 1, 19: 2, 25: 13, 40: 40, 4: int(NYU40[4])}

# frame: camera (eye, target), rectangles (class, u0, u1, v0, v1 inclusive, depth range mm)
FRAMES = [
    (((-2.0, 0.0, 1.0), (0.0, 0.0, 1.0)), [(2, 60, 119, 80, 139, (1900, 2100)), (5, 200, 259, 60, 129, (2400, 2600))]),
    (((-2.0, 1.0, 1.1), (0.0, 0.5, 1.0)), [(2, 30, 99, 50, 119, (2000, 2300))]),
    (((-2.0, 0.05, 1.0), (0.0, 0.05, 1.0)), [(2, 125, 184, 80, 139, (1900, 2100)), (7, 230, 289, 150, 209, (3000, 3200))]),
    (((0.0, -3.0, 1.2), (0.0, 0.0, 1.0)), [(5, 100, 179, 70, 149, (2800, 3000)), (11, 220, 279, 40, 99, (1500, 1700))]),
]
ZERO_DEPTH = (3, slice(90, 94), slice(120, 126))           # depth 0 inside frame 3's class 5

# x, y, w, h, score, label per frame
BOXES = [
    [[55.5, 75.5, 70.0, 70.0, 0.91, 2.0],
     [50.25, 70.5, 80.5, 80.25, 0.83, 2.0],                 # the same (frame, label): the same lifted box
     [0.0, 20.5, 100.25, 80.5, 0.99, 2.0],                  # edge filter: x == 0
     [190.5, 50.5, 80.0, 90.0, 0.86, 5.0],
     [120.5, 150.5, 40.0, 40.0, 0.47, 9.0],                 # a label absent from the frame
     [10.5, 10.5, 300.0, 200.0, 0.3, -100.0]],              # lifts the ignored pixels
    [],                                                     # a frame without boxes
    [[120.5, 75.5, 70.0, 70.0, 0.72, 2.0],
     [225.5, 145.5, 70.0, 70.0, 0.61, 7.0]],
    [[95.5, 65.5, 90.0, 90.0, 0.66, 5.0],
     [215.5, 35.5, 70.0, 70.0, 0.55, 11.0],
     [100.5, 139.5, 50.0, 100.5, 0.97, 5.0]],               # edge filter: y + h == 240
]


def scene(seed=41):
    """-> depths (F,H,W) uint16, labels (F,H,W) int64, poses (F,4,4) float32"""
    rng = np.random.Generator(np.random.PCG64(seed))
    F = len(FRAMES)
    labels = rng.choice(BACKGROUND, (F, H, W)).astype(np.int64)
    depths = rng.integers(2500, 4000, (F, H, W)).astype(np.uint16)
    poses = []
    for f, ((eye, target), rects) in enumerate(FRAMES):
        poses.append(LC.look_at(eye, target))
        for cls, u0, u1, v0, v1, (d0, d1) in rects:
            labels[f, v0:v1 + 1, u0:u1 + 1] = cls
            depths[f, v0:v1 + 1, u0:u1 + 1] = rng.integers(d0, d1, (v1 - v0 + 1, u1 - u0 + 1))
    f, vs, us = ZERO_DEPTH
    depths[f, vs, us] = 0
    return depths, labels, np.stack(poses)


def cloud(depths, labels, poses, A, K, f, cls):
    """aligned points of the pixels of class cls in frame f (float64; only the pool is built
    from it, so the summation order does not matter)"""
    v, u = np.nonzero(labels[f] == cls)
    d = depths[f][v, u].astype(np.float32) / np.float32(1000.0)
    Kh = np.array(K, dtype=np.float64)
    Kh[:2] /= 2.0
    cam = (np.linalg.inv(Kh[:3, :3]) @ np.stack([u, v, np.ones_like(u)]).astype(np.float64) * d).T
    P = poses[f].astype(np.float64)
    world = cam @ P[:3, :3].T + P[:3, 3]
    return world @ A[:3, :3].T + A[:3, 3]


def case(name):
    """-> dict(depths (F,H,W) uint16, labels (F,H,W) int64 class maps (pseudo) or float32 nyu40
    maps, axis_align_matrix, intrinsic, poses (F,4,4) f32, boxes2d [F x (k,6) f64],
    gss_pool (P,7) f64, pseudo)"""
    depths, labels, poses = scene()
    A, K = LC.alignment(), LC.intrinsic()
    rng = np.random.Generator(np.random.PCG64(9))
    pts = lambda f, cls: cloud(depths, labels, poses, A, K, f, cls)   # noqa: E731
    pool = [LC.pool_box(pts(0, 2), (0.06, 0.3, 0.3)), LC.pool_box(pts(2, 2), (0.06, 0.3, 0.3)),
            LC.pool_box(pts(0, 5), (0.1, 0.08, 0.12)), LC.pool_box(pts(3, 5), (0.2, 0.3, 0.1)),
            LC.pool_box(pts(2, 7), (0.07, 0.09, 0.05))]
    for _ in range(9):                                     # far from everything
        c = rng.uniform([16, 16, 0], [19, 19, 2])
        pool.append(np.concatenate([c, rng.uniform(0.3, 0.9, 3), [0.0]]))
    pool = np.array(pool)
    pool = pool[rng.permutation(len(pool))]
    boxes2d = [np.array(b, dtype=np.float64).reshape(-1, 6) for b in BOXES]
    out = dict(depths=depths, labels=labels, axis_align_matrix=A, intrinsic=K, poses=poses,
               boxes2d=boxes2d, gss_pool=pool, pseudo=True)
    if name == "main":
        return out
    if name == "gt_labels":                                # nyu40 ids as the label-mapped PNGs hold them
        nyu = np.zeros_like(labels)
        for c in np.unique(labels):
            nyu[labels == c] = BACKGROUND_NYU[int(c)] if int(c) in BACKGROUND_NYU else NYU40[int(c)]
        return dict(out, labels=nyu.astype(np.float32), pseudo=False)
    if name == "nothing_lifted":                           # every box names a class no frame has
        out["boxes2d"] = [np.concatenate([b[:, :5], np.full((len(b), 1), 9.0)], 1) for b in boxes2d]
        return out
    if name == "nothing_matched":                          # the pool is elsewhere
        out["gss_pool"] = pool + np.array([40.0, 0, 0, 0, 0, 0, 0])
        return out
    raise KeyError(name)


CASES = ("main", "gt_labels", "nothing_lifted", "nothing_matched")


def write_tree(case, root, scan, with_labels=True):
    """the files the reference script and ScannetBoxLifter(view="single") read for one scan:
    lift_cases.write_scannet_tree's, with the per-frame dict in lseg/ (pseudo) and the PNGs
    frames/<scan>/depth/<id>.png and frames/<scan>/label-mapped/<id>.png (written and checked
    through PIL)"""
    from PIL import Image
    stub = dict(case, points=np.zeros((1, 3)), labels=np.zeros(1))
    LC.write_scannet_tree(stub, root, scan)
    frames = os.path.join(root, "frames", scan)
    for d in ("depth", "label-mapped"):
        os.makedirs(os.path.join(frames, d), exist_ok=True)
    if case["pseudo"] and with_labels:
        np.save(os.path.join(root, "lseg", scan + ".npy"),
                {i: np.ascontiguousarray(m, dtype=np.int16) for i, m in enumerate(case["labels"])})
    for i, depth in enumerate(case["depths"]):
        path = os.path.join(frames, "depth", "%d.png" % i)
        Image.fromarray(depth).save(path)
        assert np.array_equal(np.array(Image.open(path)), depth)
        if not case["pseudo"]:
            path = os.path.join(frames, "label-mapped", "%d.png" % i)
            Image.fromarray(case["labels"][i].astype(np.uint8)).save(path)
            assert np.array_equal(np.array(Image.open(path)), case["labels"][i])
