"""Seeded synthetic scenes for the multiview back-projection (tests/golden/backproj.npz).

A scene is a room of axis-aligned rectangles (floor, ceiling, four walls, a table) with
vertices drawn on the surfaces, a share of them lifted off the surface or pushed behind a wall,
and frames whose 41 x 32 depth maps are ray-cast from look-at poses through the helper's
intrinsic, so depth agrees with geometry and a healthy share of the vertices map.

`evaluate` restates every decision in float64 and measures how far each decision quantity is
from its threshold: the reference ran in float32 with a summation order of its own, so a
recorded result is only a fair target where no quantity is within 32 * 2^-23 * S of its
threshold, S the sum of the absolute values of the terms the quantity is formed from:
  frustum      100 * sum_i (p_i - c_i) n_i + 0.5 against 0;  S = 100 * sum_i (|p_i| + |c_i|) |n_i| + 0.5
  pixel        x - (floor(x) + 0.5) against 0, x = cam_x fx / cam_z + cx;
               S = fx S_x / |cam_z| + |x - cx| S_z / |cam_z| + cx + 0.5, S_x and S_z the absolute
               row sums sum_j |b_ij p_j| + |b_i3| of the world-to-camera product (and y alike)
  depth        d - depth_min (S = |d| + depth_min), depth_max - d (S = depth_max + |d|),
               accuracy - |d - cam_z| (S = accuracy + |d| + S_z)
A quantity counts only where the decisions before it let the point through (a pixel is only
rounded for a point inside the frustum, a depth only read at a pixel inside the image).
Points that miss a margin in any frame are redrawn here, so no test drops a point."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (HERE, os.path.dirname(HERE)):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import backproj_ref as R  # noqa: E402
from lift_cases import look_at  # noqa: E402

IMAGE_DIMS = (41, 32)
MARGIN = 32 * 2.0 ** -23
CASES = ("main", "edges")
PLANES = ((3, 1, 0), (2, 5, 1), (3, 6, 2), (0, 7, 3), (1, 4, 0), (6, 4, 5))

# (axis, value, lo, hi of the two other axes in ascending axis order)
ROOM = (5.0, 4.0, 2.6)
RECTS = [(2, 0.0, (0, 0), (5, 4)), (2, 2.6, (0, 0), (5, 4)), (0, 0.0, (0, 0), (4, 2.6)),
         (0, 5.0, (0, 0), (4, 2.6)), (1, 0.0, (0, 0), (5, 2.6)), (1, 4.0, (0, 0), (5, 2.6)),
         (2, 0.8, (1.5, 1.0), (2.5, 2.0)), (0, 1.5, (1.0, 0), (2.0, 0.8)), (0, 2.5, (1.0, 0), (2.0, 0.8)),
         (1, 1.0, (1.5, 0), (2.5, 0.8)), (1, 2.0, (1.5, 0), (2.5, 0.8))]


def _others(axis):
    return [a for a in range(3) if a != axis]


def ray_cast(pose, par, image_dims=IMAGE_DIMS):
    """(H,W) float32 depth (camera z of the nearest rectangle along every pixel's ray; 0: none)"""
    W, H = image_dims
    fx, fy, cx, cy = (float(v) for v in par[:4])
    P = pose.astype(np.float64)
    u, v = np.meshgrid(np.arange(W), np.arange(H))
    d_cam = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u, dtype=float)], -1)
    d_world = d_cam @ P[:3, :3].T
    o = P[:3, 3]
    best = np.full((H, W), np.inf)
    with np.errstate(all="ignore"):
        for axis, value, lo, hi in RECTS:
            t = (value - o[axis]) / d_world[..., axis]
            hit = o + t[..., None] * d_world
            a, b = _others(axis)
            ok = (t > 0) & (hit[..., a] >= lo[0]) & (hit[..., a] <= hi[0]) & (hit[..., b] >= lo[1]) & (hit[..., b] <= hi[1])
            best = np.where(ok & (t < best), t, best)
    return np.where(np.isfinite(best), best, 0.0).astype(np.float32)


def draw_points(rng, n):
    """n float32 vertices: on a rectangle (70 %), up to 8 cm off it (15 %), anywhere in a box
    half a metre larger than the room (15 %)"""
    area = np.array([(hi[0] - lo[0]) * (hi[1] - lo[1]) for _, _, lo, hi in RECTS])
    which = rng.choice(len(RECTS), n, p=area / area.sum())
    kind = rng.random(n)
    pts = np.empty((n, 3))
    for i in range(n):
        axis, value, lo, hi = RECTS[which[i]]
        a, b = _others(axis)
        pts[i, axis] = value + (rng.uniform(-0.08, 0.08) if kind[i] > 0.7 else 0.0)
        pts[i, a], pts[i, b] = rng.uniform(lo[0], hi[0]), rng.uniform(lo[1], hi[1])
        if kind[i] > 0.85:
            pts[i] = rng.uniform([-0.5, -0.5, -0.5], np.array(ROOM) + 0.5)
    return pts.astype(np.float32)


def evaluate(pts, depth, poses, par, image_dims=IMAGE_DIMS):
    """float64 decisions of every (frame, point) -> dict: keep (F,N) bool and pixel (F,N); near
    (N) bool, a point with a decision quantity inside its margin in some frame; stats, per
    filter (accepted, rejected) counts over the pairs the filter is defined on"""
    W, H = image_dims
    p = np.asarray(pts, dtype=np.float32).astype(np.float64)
    par = np.asarray(par, dtype=np.float32).astype(np.float64)
    fx, fy, cx, cy, dmin, dmax, acc = par[:7]
    cp = par[8:32].reshape(8, 3)
    F, N = len(poses), len(p)
    keep, pixel, near = np.zeros((F, N), bool), np.zeros((F, N), np.int64), np.zeros(N, bool)
    stats = {k: [0, 0] for k in ("frustum", "pixel range", "depth range", "depth agreement")}

    def tally(name, mask, where):
        stats[name][0] += int((mask & where).sum())
        stats[name][1] += int((~mask & where).sum())

    with np.errstate(all="ignore"):
        for f in range(F):
            P = np.asarray(poses[f], dtype=np.float32).astype(np.float64)
            if not np.isfinite(P).all() or np.linalg.matrix_rank(P) < 4:
                continue
            B = np.linalg.inv(P)
            c = cp @ P[:3, :3].T + P[:3, 3]
            inside = np.ones(N, bool)
            for k, (pa, pb, po) in enumerate(PLANES):
                n = np.cross(c[pa] - c[po], c[pb] - c[po])
                cc = c[2] if k < 3 else c[4]
                q = 100.0 * ((p - cc) @ n) + 0.5
                S = 100.0 * ((np.abs(p) + np.abs(cc)) @ np.abs(n)) + 0.5
                near |= ~(np.abs(q) >= MARGIN * S)
                inside &= q < 0
            tally("frustum", inside, np.ones(N, bool))
            cam = p @ B[:3, :3].T + B[:3, 3]
            Sc = np.abs(p) @ np.abs(B[:3, :3]).T + np.abs(B[:3, 3])
            xy = np.stack([cam[:, 0] * fx / cam[:, 2] + cx, cam[:, 1] * fy / cam[:, 2] + cy], 1)
            for a, (fa, ca) in enumerate(((fx, cx), (fy, cy))):
                q = xy[:, a] - (np.floor(xy[:, a]) + 0.5)
                S = (fa * Sc[:, a] + np.abs(xy[:, a] - ca) * Sc[:, 2]) / np.abs(cam[:, 2]) + ca + 0.5
                near |= inside & ~(np.abs(q) >= MARGIN * S)
            r = np.rint(xy)
            defined = np.isfinite(xy).all(1)
            inrange = defined & (r[:, 0] >= 0) & (r[:, 0] < W) & (r[:, 1] >= 0) & (r[:, 1] < H)
            tally("pixel range", inrange, defined)
            pix = np.where(inrange, r[:, 1] * W + r[:, 0], 0).astype(np.int64)
            d = np.asarray(depth[f], dtype=np.float32).astype(np.float64).reshape(-1)[pix]
            gap = np.abs(d - cam[:, 2])
            for q, S in ((d - dmin, np.abs(d) + dmin), (dmax - d, dmax + np.abs(d)),
                         (acc - gap, acc + np.abs(d) + Sc[:, 2])):
                near |= inside & inrange & ~(np.abs(q) >= MARGIN * S)
            ranged, agree = (d >= dmin) & (d <= dmax), gap <= acc
            tally("depth range", ranged, inrange)
            tally("depth agreement", agree, inrange)
            keep[f] = inside & inrange & ranged & agree
            pixel[f] = np.where(keep[f], pix, 0)
    return {"keep": keep, "pixel": pixel, "near": near, "stats": stats}


def _settle(rng, pts, depth, poses, par):
    """redraw the points that sit inside a margin until none does"""
    for _ in range(50):
        near = evaluate(pts, depth, poses, par)["near"]
        if not near.any():
            return pts
        pts[near] = draw_points(rng, int(near.sum()))
    raise AssertionError("points kept landing inside a margin")


def case(name):
    """-> dict points (N,3) f32, depth (F,32,41) f32, poses (F,4,4) f32, features (F,3,32,41) f32"""
    par = R.params()
    W, H = IMAGE_DIMS
    if name == "main":
        rng = np.random.Generator(np.random.PCG64(20240))
        N = 4000
        views = [((0.8, 0.7, 1.5), (3.5, 3.0, 0.6)), ((4.3, 0.6, 1.6), (1.5, 3.2, 0.9)),
                 ((2.0, 3.5, 1.4), (2.0, 1.5, 0.8)), ((4.4, 3.4, 1.7), (0.5, 0.4, 0.3)),
                 ((2.6, 0.5, 1.2), (2.1, 1.4, 0.7)), ((0.6, 3.3, 1.8), (4.8, 1.0, 1.0))]
    elif name == "edges":
        rng = np.random.Generator(np.random.PCG64(20241))
        N = 400
        # 0 looks out through a wall from outside the room (nothing maps), 1 gets an all-zero depth
        # map, 3 is 2 moved by a few centimetres (most of its vertices map in both)
        views = [((-1.0, 2.0, 1.3), (-4.0, 2.1, 1.2)), ((0.8, 0.7, 1.5), (3.5, 3.0, 0.6)),
                 ((2.0, 3.5, 1.4), (2.0, 1.5, 0.8)), ((2.03, 3.52, 1.41), (2.0, 1.5, 0.8)),
                 ((4.3, 0.6, 1.6), (1.5, 3.2, 0.9))]
    else:
        raise KeyError(name)
    poses = np.stack([look_at(eye, target) for eye, target in views])
    depth = np.stack([ray_cast(P, par) for P in poses])
    holes = rng.random(depth.shape) < 0.04
    depth[holes] = 0.0
    if name == "edges":
        depth[1] = 0.0
    pts = _settle(rng, draw_points(rng, N), depth, poses, par)
    features = (rng.integers(-128, 128, (len(poses), 3, H, W)) / 16.0).astype(np.float32)
    return {"points": pts, "depth": depth, "poses": poses, "features": features}
