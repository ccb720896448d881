"""numpy restatement of the multiview back-projection (ov3d_amd.projection, csrc/backproj.hip):
the helper's constants, the frame table, the per-(frame, point) decision, the (F, N+1) index
tables, ProjectionHelper.project and the compose loop.  Elementwise float32 (the inverse pose in
float64, rounded) with every sum written out in the order include/ov3d_backproj.h states, so the
device results are expected bit for bit; tests/test_backproj_cpu.py holds it to the reference's
recorded results (tests/golden/backproj.npz)."""
import numpy as np

ROW, NPARAMS, BLOCK = 40, 32, 1024
PLANE_CORNERS = ((3, 1, 0), (2, 5, 1), (3, 6, 2), (0, 7, 3), (1, 4, 0), (6, 4, 5))
INTRINSICS = [[37.01983, 0, 20, 0], [0, 38.52470, 15.5, 0], [0, 0, 1, 0], [0, 0, 0, 1]]
F32 = np.float32


def params(intrinsic=INTRINSICS, depth_min=0.1, depth_max=4.0, image_dims=(41, 32), accuracy=0.05):
    """(32) float32: fx fy cx cy depth_min depth_max accuracy 0, then the eight corner points,
    each formed in Python floats and rounded once"""
    fx, fy, cx, cy = intrinsic[0][0], intrinsic[1][1], intrinsic[0][2], intrinsic[1][2]
    W, H = image_dims
    out = [fx, fy, cx, cy, depth_min, depth_max, accuracy, 0.0]
    for d in (depth_min, depth_max):
        for ux, uy in ((0, 0), (W - 1, 0), (W - 1, H - 1), (0, H - 1)):
            out += [d * ((ux - cx) / fx), d * ((uy - cy) / fy), d]
    return np.array(out, dtype=F32)


def inverse_rows(P):
    """(4,4) float32 -> (4,4) float32: the float64 adjugate over the determinant, rounded"""
    a = np.asarray(P, dtype=F32).astype(np.float64)
    (a00, a01, a02, a03), (a10, a11, a12, a13), (a20, a21, a22, a23), (a30, a31, a32, a33) = a
    s0, s1, s2 = a00 * a11 - a10 * a01, a00 * a12 - a10 * a02, a00 * a13 - a10 * a03
    s3, s4, s5 = a01 * a12 - a11 * a02, a01 * a13 - a11 * a03, a02 * a13 - a12 * a03
    c5, c4, c3 = a22 * a33 - a32 * a23, a21 * a33 - a31 * a23, a21 * a32 - a31 * a22
    c2, c1, c0 = a20 * a33 - a30 * a23, a20 * a32 - a30 * a22, a20 * a31 - a30 * a21
    det = ((((s0 * c5 - s1 * c4) + s2 * c3) + s3 * c2) - s4 * c1) + s5 * c0
    b = np.array([
        ((a11 * c5 - a12 * c4) + a13 * c3) / det, ((-a01 * c5 + a02 * c4) - a03 * c3) / det,
        ((a31 * s5 - a32 * s4) + a33 * s3) / det, ((-a21 * s5 + a22 * s4) - a23 * s3) / det,
        ((-a10 * c5 + a12 * c2) - a13 * c1) / det, ((a00 * c5 - a02 * c2) + a03 * c1) / det,
        ((-a30 * s5 + a32 * s2) - a33 * s1) / det, ((a20 * s5 - a22 * s2) + a23 * s1) / det,
        ((a10 * c4 - a11 * c2) + a13 * c0) / det, ((-a00 * c4 + a01 * c2) - a03 * c0) / det,
        ((a30 * s4 - a31 * s2) + a33 * s0) / det, ((-a20 * s4 + a21 * s2) - a23 * s0) / det,
        ((-a10 * c3 + a11 * c1) - a12 * c0) / det, ((a00 * c3 - a01 * c1) + a02 * c0) / det,
        ((-a30 * s3 + a31 * s1) - a32 * s0) / det, ((a20 * s3 - a21 * s1) + a22 * s0) / det])
    return b.astype(F32).reshape(4, 4)


def frame_table(poses, par):
    """(F,4,4) float32 -> (F, ROW) float32"""
    poses = np.asarray(poses, dtype=F32)
    table = np.zeros((len(poses), ROW), F32)
    corner_points = par[8:32].reshape(8, 3)
    with np.errstate(all="ignore"):
        for f, P in enumerate(poses):
            b = inverse_rows(P)
            c = np.empty((8, 3), F32)
            for k, (x, y, z) in enumerate(corner_points):
                for i in range(3):
                    c[k, i] = ((P[i, 0] * x + P[i, 1] * y) + P[i, 2] * z) + P[i, 3]
            table[f, :12] = b[:3].reshape(-1)
            table[f, 12:15], table[f, 15:18] = c[2], c[4]
            for k, (pa, pb, po) in enumerate(PLANE_CORNERS):
                u, v = c[pa] - c[po], c[pb] - c[po]
                table[f, 18 + 3 * k: 21 + 3 * k] = (u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2],
                                                    u[0] * v[1] - u[1] * v[0])
            table[f, 36] = 1.0
            if not (np.isfinite(P).all() and np.isfinite(b).all()):
                table[f] = 0.0                                  # an empty frame: the whole row
    return table


def decide(row, par, image_dims, depth, pts):
    """one frame: row (ROW), depth (H,W) float32, pts (N,3) float32 -> (keep (N) bool, pixel (N)
    int64, valid where keep)"""
    W, H = image_dims
    pts = np.asarray(pts, dtype=F32)
    N = len(pts)
    if row[36] == 0.0:
        return np.zeros(N, bool), np.zeros(N, np.int64)
    x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
    fx, fy, cx, cy, dmin, dmax, acc = par[:7]
    hundred = F32(100.0)
    with np.errstate(all="ignore"):
        inside = np.ones(N, bool)
        for k in range(6):
            c = row[12:15] if k < 3 else row[15:18]
            n = row[18 + 3 * k: 21 + 3 * k]
            dot = ((x - c[0]) * n[0] + (y - c[1]) * n[1]) + (z - c[2]) * n[2]
            inside &= np.rint(dot * hundred) / hundred < 0
        cam = [((row[4 * i] * x + row[4 * i + 1] * y) + row[4 * i + 2] * z) + row[4 * i + 3] for i in range(3)]
        rx = np.rint((cam[0] * fx) / cam[2] + cx)
        ry = np.rint((cam[1] * fy) / cam[2] + cy)
        assert rx.dtype == F32 and cam[2].dtype == F32
        ok = inside & (rx >= 0) & (rx < W) & (ry >= 0) & (ry < H)
        pix = np.where(ok, ry.astype(np.float64) * W + rx.astype(np.float64), 0).astype(np.int64)
        d = np.asarray(depth, dtype=F32).reshape(-1)[pix]
        keep = ok & (d >= dmin) & (d <= dmax) & (np.abs(d - cam[2]) <= acc)
    return keep, pix


def tables(pts, depth, poses, par, image_dims=(41, 32)):
    """-> idx3d, idx2d (F, N+1) int64"""
    F, N = len(poses), len(pts)
    table = frame_table(poses, par)
    i3, i2 = np.zeros((F, N + 1), np.int64), np.zeros((F, N + 1), np.int64)
    for f in range(F):
        keep, pix = decide(table[f], par, image_dims, depth[f], pts)
        idx = np.nonzero(keep)[0]
        i3[f, 0] = i2[f, 0] = len(idx)
        i3[f, 1:1 + len(idx)], i2[f, 1:1 + len(idx)] = idx, pix[idx]
    return i3, i2


def project(label, i3, i2, num_points):
    """ProjectionHelper.project: label (C,H,W) or (H,W) -> (C, num_points)"""
    label = np.asarray(label)
    C = 1 if label.ndim == 2 else label.shape[0]
    out = np.zeros((C, num_points), label.dtype)
    n = int(i3[0])
    if n > 0:
        out[:, i3[1:1 + n]] = label.reshape(C, -1)[:, i2[1:1 + n]]
    return out


def compose_loop(features, i3, i2, num_points, project_fn=project):
    """the definition of compose_features over tables: later frames overwrite earlier ones
    -> (out (C, N), frame (N) int32)"""
    features = np.asarray(features)
    out = np.zeros((features.shape[1], num_points), features.dtype)
    frame = np.full(num_points, -1, np.int32)
    for i in range(len(features)):
        p = project_fn(features[i], i3[i], i2[i], num_points)
        idx = i3[i][1:1 + int(i3[i][0])]
        out[:, idx] = p[:, idx]
        frame[idx] = i
    return out, frame


def compose(pts, depth, poses, features, par, image_dims=(41, 32)):
    i3, i2 = tables(pts, depth, poses, par, image_dims)
    return compose_loop(features, i3, i2, len(pts))
