"""Synthetic inputs of the pseudo-box lifting tests (tests/golden/lift_boxes.npz is what the
reference's lift_boxes.py scripts make of them; make_lift_golden.py).

ScanNet cases: float32-rounded points held as float64, labelled blobs plus a sparse background
of ignored labels, cameras looking at one blob each, 2D boxes around the blob's projection.
SUN RGB-D cases: a small depth image with labelled rectangles.  Every decision of the chain
(frustum membership, both NMS passes, the match, every argsort) is far from its threshold for
these inputs; the generator asserts the margins and that no stage is trivial.
"""
import os

import numpy as np

FX, CX, CY = 577.870605, 319.5, 239.5          # the 640 x 480 depth intrinsic
SUN_IDS = (36, 4, 10, 29, 5, 12, 14, 8, 17, 35, 32, 18, 34, 6, 7, 25, 33)


def intrinsic():
    K = np.eye(4, dtype=np.float32)
    K[0, 0] = K[1, 1] = FX
    K[0, 2], K[1, 2] = CX, CY
    return K


def alignment(angle=0.35, shift=(1.25, -0.75, 0.125)):
    c, s = np.cos(angle), np.sin(angle)
    A = np.eye(4)
    A[:2, :2] = [[c, s], [-s, c]]
    A[:3, 3] = shift
    return A


def look_at(eye, target):
    """camera-to-world (4,4) float32: z forward to the target, y down"""
    eye, target = np.asarray(eye, float), np.asarray(target, float)
    z = (target - eye) / np.linalg.norm(target - eye)
    x = np.cross(z, [0.0, 0.0, 1.0])
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    P = np.eye(4)
    P[:3, 0], P[:3, 1], P[:3, 2], P[:3, 3] = x, y, z, eye
    return P.astype(np.float32)


def box_around(pose, pts, pad):
    """x, y, w, h of the projection of pts (original frame) into the 320 x 240 frame, padded
    and moved off the pixel grid"""
    P = pose.astype(np.float64)
    cam = (pts - P[:3, 3]) @ P[:3, :3]
    u = FX / 2 * cam[:, 0] / cam[:, 2] + CX / 2
    v = FX / 2 * cam[:, 1] / cam[:, 2] + CY / 2
    x, y = np.floor(u.min()) - pad + 0.37, np.floor(v.min()) - pad + 0.41
    return [x, y, np.ceil(u.max()) + pad + 0.23 - x, np.ceil(v.max()) + pad + 0.19 - y]


# blob: class, centre (original frame), half size
BLOBS = [(2, (1.0, 0.5, 0.6), 0.25), (2, (1.0, 1.3, 0.6), 0.25), (5, (-1.5, -1.0, 0.8), 0.3),
         (7, (-1.0, 2.2, 0.5), 0.2), (11, (2.2, -1.6, 1.0), 0.25)]


def scannet_scene(seed, n_blob=60, n_back=240):
    """-> aligned points (N,3) f64 (float32 values), labels (N) f64, A, the blobs' original and
    aligned points"""
    rng = np.random.Generator(np.random.PCG64(seed))
    A = alignment()
    orig, lab = [], []
    for cls, c, r in BLOBS:
        orig.append(np.asarray(c) + rng.uniform(-r, r, (n_blob, 3)))
        lab.append(np.full(n_blob, float(cls)))
    orig.append(rng.uniform([-3, -3, 0], [3, 3, 2.4], (n_back, 3)))
    lab.append(rng.choice([18.0, 19.0, 25.0, 40.0, 4.0], n_back))      # 4: a class no box names
    orig, lab = np.concatenate(orig), np.concatenate(lab)
    aligned = (orig @ A[:3, :3].T + A[:3, 3]).astype(np.float32).astype(np.float64)
    back = (aligned - A[:3, 3]) @ A[:3, :3]                            # original frame again
    blobs_o = [back[i * n_blob:(i + 1) * n_blob] for i in range(len(BLOBS))]
    blobs_a = [aligned[i * n_blob:(i + 1) * n_blob] for i in range(len(BLOBS))]
    return aligned, lab, A, blobs_o, blobs_a


def pool_box(pts, grow):
    lo, hi = pts.min(0), pts.max(0)
    return np.concatenate([(lo + hi) / 2, (hi - lo) + np.asarray(grow), [0.0]])


def scannet_case(name):
    """-> dict(points, labels, axis_align_matrix, intrinsic, poses (F,4,4) f32,
    boxes2d [F x (k,6) f64], gss_pool (P,7) f64)"""
    aligned, lab, A, bo, ba = scannet_scene(11)
    rng = np.random.Generator(np.random.PCG64(5))
    views = [((-1.5, 0.5, 0.6), 0), ((-1.5, 1.3, 0.7), 1), ((0.5, -1.0, 0.9), 2),
             ((-1.5, 1.2, 0.8), 2), None, ((-1.0, 0.2, 0.5), 3), ((2.2, 0.4, 1.0), 4)]
    scores = [0.91, 0.83, 0.86, 0.72, 0.66, 0.61, 0.55]
    poses, boxes2d = [], []
    for f, view in enumerate(views):
        if view is None:                                   # ScanNet's invalid pose
            poses.append(np.full((4, 4), -np.inf, np.float32))
            boxes2d.append(np.array([[40.5, 30.5, 60.0, 50.0, scores[f], 2.0]]))
            continue
        eye, b = view
        pose = look_at(eye, BLOBS[b][1])
        rows = [box_around(pose, bo[b], 4) + [scores[f], float(BLOBS[b][0])]]
        if f == 0:                                         # removed by the edge filter
            rows.append([0.0, 20.5, 100.25, 80.5, 0.99, 2.0])
            rows.append([100.5, 20.25, 219.5, 90.5, 0.98, 5.0])      # x + w == 320
        if f == 3:                                         # a class without points; a zero-width box
            rows.append(box_around(pose, bo[b], 6) + [0.47, 9.0])
            rows.append([150.5, 100.5, 0.0, 40.0, 0.45, 5.0])
        poses.append(pose)
        boxes2d.append(np.array(rows, dtype=np.float64))
    pool = [pool_box(ba[0], (0.06, 0.45, 0.06)), pool_box(ba[1], (0.06, 0.45, 0.06)),
            pool_box(ba[2], (0.1, 0.08, 0.12)), pool_box(ba[2], (0.5, 0.45, 0.4)),
            pool_box(ba[4], (0.07, 0.09, 0.05))]
    for _ in range(9):                                     # far from every blob
        c = rng.uniform([6, 6, 0], [9, 9, 2])
        pool.append(np.concatenate([c, rng.uniform(0.3, 0.9, 3), [0.0]]))
    pool = np.array(pool)
    pool = pool[rng.permutation(len(pool))]
    case = dict(points=aligned, labels=lab, axis_align_matrix=A, intrinsic=intrinsic(),
                poses=np.stack(poses), boxes2d=boxes2d, gss_pool=pool)
    if name == "main":
        return case
    if name == "nothing_lifted":                           # every box names a class without points
        case["boxes2d"] = [np.concatenate([b[:, :5], np.full((len(b), 1), 9.0)], 1) for b in boxes2d]
        return case
    if name == "nothing_matched":                          # the pool is elsewhere
        case["gss_pool"] = pool + np.array([20.0, 0, 0, 0, 0, 0, 0])
        return case
    raise KeyError(name)


SCANNET_CASES = ("main", "nothing_lifted", "nothing_matched")


def sun_case(name):
    """-> dict(depth (H,W) uint16, seg (H,W) int64 raw ids, Rtilt, K, boxes2d (k,6), gss_pool)"""
    H, W = 48, 64
    rng = np.random.Generator(np.random.PCG64(23))
    seg = rng.choice([0, 1, 2, 3, 9, 20], (H, W)).astype(np.int64)       # ids outside the table
    depth = rng.integers(18, 40, (H, W)).astype(np.uint16)
    # object: class index, u0, u1, v0, v1 (inclusive), depth range
    objs = [(1, 10, 22, 8, 20, (20, 24)), (1, 30, 41, 8, 20, (20, 24)), (4, 45, 58, 28, 40, (26, 30)),
            (13, 6, 18, 30, 42, (15, 19))]
    for cls, u0, u1, v0, v1, (d0, d1) in objs:
        seg[v0:v1 + 1, u0:u1 + 1] = SUN_IDS[cls]
        depth[v0:v1 + 1, u0:u1 + 1] = rng.integers(d0, d1, (v1 - v0 + 1, u1 - u0 + 1))
    depth[10:12, 31:34] = 0                                               # depth 0 takes part
    a = 0.12
    Rtilt = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    K = np.array([[57.5, 0, 31.25], [0, 58.25, 23.75], [0, 0, 1]])
    boxes = np.array([
        [10.0, 8.0, 12.0, 12.0, 0.93, 1.0],           # edges exactly on pixel coordinates
        [8.5, 6.5, 15.25, 15.5, 0.81, 1.0],           # the same object: suppressed by the first NMS
        [28.5, 6.25, 14.5, 15.5, 0.88, 1.0],
        [43.5, 26.5, 16.25, 15.75, 0.77, 4.0],        # no pool box near it
        [4.25, 28.5, 15.5, 15.25, 0.69, 13.0],
        [0.0, 5.5, 20.0, 20.0, 0.99, 1.0],            # edge filter: x == 0
        [40.5, 30.5, 23.5, 10.0, 0.97, 4.0],          # edge filter: x + w == W
        [20.5, 2.5, 5.25, 3.5, 0.52, 6.0],            # no pixel of its class
    ])

    def cloud(u0, u1, v0, v1):
        v, u = np.mgrid[v0:v1 + 1, u0:u1 + 1]
        d = depth[v0:v1 + 1, u0:u1 + 1].astype(float)
        p = np.stack([(u - K[0, 2]) * d / K[0, 0], d, -(v - K[1, 2]) * d / K[1, 1]], -1).reshape(-1, 3)
        return p @ Rtilt.T
    c0, c1, c3 = cloud(10, 22, 8, 20), cloud(30, 41, 8, 20), cloud(6, 18, 30, 42)
    pool = [pool_box(c0, (4.0, 0.5, 0.5)), pool_box(c1, (4.0, 0.5, 0.5)), pool_box(c3, (0.5, 0.4, 0.6)),
            pool_box(c3, (6.0, 5.0, 4.0))]
    for _ in range(6):
        c = rng.uniform([60, 60, 60], [90, 90, 90])
        pool.append(np.concatenate([c, rng.uniform(3, 9, 3), [0.0]]))
    pool = np.array(pool)[rng.permutation(10)]
    case = dict(depth=depth, seg=seg, Rtilt=Rtilt, K=K, boxes2d=boxes, gss_pool=pool)
    if name == "main":
        return case
    if name == "nothing_lifted":
        case["boxes2d"] = boxes[[5, 6, 7]]
        return case
    raise KeyError(name)


SUN_CASES = ("main", "nothing_lifted")


def _num(x):
    return repr(float(x))


def write_scannet_tree(case, root, scan):
    """the files the ScanNet script (and ScannetBoxLifter) reads for one scan, under root:
    lseg/, frames/<scan>/{color,pose,intrinsic_depth.txt}, boxes2d/<scan>/color/, gss/, scans/"""
    frames = os.path.join(root, "frames", scan)
    for d in ("lseg", "gss", "out", os.path.join("scans", scan), os.path.join("boxes2d", scan, "color"),
              os.path.join("frames", scan, "color"), os.path.join("frames", scan, "pose")):
        os.makedirs(os.path.join(root, d), exist_ok=True)
    np.save(os.path.join(root, "lseg", scan + ".npy"),
            np.concatenate([case["points"], case["labels"][:, None]], 1))
    np.save(os.path.join(root, "gss", scan + "_prop.npy"), case["gss_pool"])
    with open(os.path.join(root, "scans", scan, scan + ".txt"), "w") as f:
        f.write("numDepthFrames = %d\n" % len(case["poses"]))
        f.write("axisAlignment = " + " ".join(_num(x) for x in case["axis_align_matrix"].reshape(-1)) + "\n")
    with open(os.path.join(frames, "intrinsic_depth.txt"), "w") as f:
        f.write("\n".join(" ".join(_num(x) for x in row) for row in case["intrinsic"]) + "\n")
    for i, (pose, boxes) in enumerate(zip(case["poses"], case["boxes2d"])):
        open(os.path.join(frames, "color", "%d.jpg" % i), "w").close()
        with open(os.path.join(frames, "pose", "%d.txt" % i), "w") as f:
            f.write("\n".join(" ".join(_num(x) for x in row) for row in pose) + "\n")
        np.save(os.path.join(root, "boxes2d", scan, "color", "%d.npy" % i), boxes)
