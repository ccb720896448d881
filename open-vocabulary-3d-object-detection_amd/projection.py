"""Multiview back-projection on the device: which pixel of which frame's feature map does every
scan vertex land on, and the features it takes from there.

Replaces ``utils/projection.py`` ``ProjectionHelper.compute_projection`` / ``.project`` and, with
``ov3d_amd.image_util.image_processor``, the per-frame loop of ``utils/image_util.py``.  The
kernels are csrc/backproj.hip behind include/ov3d_backproj.h, which pins the arithmetic: the
frustum test on the rounded, unnormalised plane products, the world-to-camera transform, pixel
rounding half to even and the depth-consistency test, all in float32.

  ProjectionHelper.compute_projection   one frame, the reference's return values (syncs once to
                                        decide ``None``, as the reference does)
  ProjectionHelper.compute_projections  all frames at once -> two (F, N+1) int64 tables; three
                                        launches, no synchronisation, capturable in a hipGraph
  ProjectionHelper.project              one table row -> (C, num_points) features, one launch
  compose_features                      the fused path: every vertex takes the features of the
                                        last frame that maps it; two launches, no tables

``Projection.backward`` of the reference reads tensors its forward never saved
(``ctx.saved_variables`` with ``save_for_backward`` commented out); it cannot run and is not
ported.  A frame whose pose (or its inverse) has a non-finite entry maps nothing, where the
reference's ``torch.inverse`` raises or returns NaN: ScanNet ships ``-inf`` poses.
"""
import numpy as np
import torch

from . import _native as nat

ROW, NPARAMS, BLOCK = 40, 32, 1024       # OV3D_BACKPROJ_ROW, _PARAMS, _BLOCK
INTRINSICS = [[37.01983, 0, 20, 0], [0, 38.52470, 15.5, 0], [0, 0, 1, 0], [0, 0, 0, 1]]


def _device_f32(x, device, name, shape):
    """numpy or torch, host or device, float64 or float32 -> contiguous float32 device tensor"""
    if not isinstance(x, torch.Tensor):
        x = torch.from_numpy(np.ascontiguousarray(np.asarray(x), dtype=np.float32))
    x = x.detach().to(device=device, dtype=torch.float32).contiguous()
    if x.dim() != len(shape) or any(w is not None and w != g for w, g in zip(shape, x.shape)):
        raise ValueError(f"{name}: expected shape {shape}, got {tuple(x.shape)}")
    return x


class ProjectionHelper:
    def __init__(self, intrinsic, depth_min, depth_max, image_dims, accuracy, cuda=True):
        if not cuda:
            raise nat.NativeError("ProjectionHelper: the kernels run on the ROCm device only (cuda=False)")
        self.intrinsic = intrinsic
        self.depth_min = depth_min
        self.depth_max = depth_max
        self.image_dims = image_dims
        self.accuracy = accuracy
        self.cuda = cuda
        W, H = int(image_dims[0]), int(image_dims[1])
        if W < 1 or H < 1 or W * H >= 2 ** 31:
            raise ValueError(f"image_dims: expected [W, H] with 1 <= W * H < 2^31, got {image_dims}")
        self._params = {}
        self._compute_corner_points()

    def depth_to_skeleton(self, ux, uy, depth):
        x = (ux - self.intrinsic[0][2]) / self.intrinsic[0][0]
        y = (uy - self.intrinsic[1][2]) / self.intrinsic[1][1]
        return torch.tensor([depth * x, depth * y, depth], dtype=torch.float32)

    def _compute_corner_points(self):
        """(8, 4) float32 on the host: the image corners at depth_min, then at depth_max"""
        W, H = self.image_dims[0], self.image_dims[1]
        corner_points = torch.ones(8, 4)
        for k, d in enumerate((self.depth_min, self.depth_max)):
            for j, (ux, uy) in enumerate(((0, 0), (W - 1, 0), (W - 1, H - 1), (0, H - 1))):
                corner_points[4 * k + j][:3] = self.depth_to_skeleton(ux, uy, d)
        self.corner_points = corner_points

    def host_params(self):
        """(32) float32, the constants of include/ov3d_backproj.h"""
        k = self.intrinsic
        head = torch.tensor([k[0][0], k[1][1], k[0][2], k[1][2], self.depth_min, self.depth_max,
                             self.accuracy, 0.0], dtype=torch.float32)
        return torch.cat([head, self.corner_points[:, :3].reshape(-1)])

    def params(self, device):
        """the constants on `device` (uploaded once per device; do the first call outside a
        graph capture)"""
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if device not in self._params:
            self._params[device] = nat.check_device(self.host_params().to(device), "params")
        return self._params[device]

    def _device(self, *xs):
        for x in xs:
            if isinstance(x, torch.Tensor) and x.is_cuda:
                return x.device
        return torch.device("cuda", torch.cuda.current_device())

    def frame_table(self, camera_to_world):
        """(F,4,4) poses -> (F, 40) float32 rows (world-to-camera, corners 2 and 4, six normals,
        usable flag); one launch"""
        dev = self._device(camera_to_world)
        poses = _device_f32(camera_to_world, dev, "camera_to_world", (None, 4, 4))
        F = poses.shape[0]
        if F < 1:
            raise ValueError("camera_to_world: at least one frame")
        table = torch.empty((F, ROW), dtype=torch.float32, device=dev)
        nat.call("ov3d_backproj_frames", poses, F, self.params(dev), table, like=poses)
        return table

    def compute_projections(self, points, depth, camera_to_world):
        """points (N,3), depth (F,H,W), camera_to_world (F,4,4) -> (indices_3d, indices_2d), each
        (F, N+1) int64: per frame the count, the mapped point indices ascending / their pixel
        indices, zeros.  A frame that maps nothing (the reference's ``None``) is a zero row."""
        dev = self._device(points, depth, camera_to_world)
        W, H = int(self.image_dims[0]), int(self.image_dims[1])
        pts = _device_f32(points, dev, "points", (None, 3))
        poses = _device_f32(camera_to_world, dev, "camera_to_world", (None, 4, 4))
        F, N = poses.shape[0], pts.shape[0]
        dep = _device_f32(depth, dev, "depth", (F, H, W))
        if N < 1 or F < 1 or N + 1 >= 2 ** 31:
            raise ValueError(f"expected 1 <= N < 2^31 - 1 points and F >= 1 frames, got N = {N}, F = {F}")
        table = torch.empty((F, ROW), dtype=torch.float32, device=dev)
        counts = torch.empty((F, -(-N // BLOCK)), dtype=torch.int32, device=dev)
        i3 = torch.empty((F, N + 1), dtype=torch.int64, device=dev)
        i2 = torch.empty((F, N + 1), dtype=torch.int64, device=dev)
        nat.call("ov3d_backproj_tables", pts, N, dep, poses, F, self.params(dev), W, H, table, counts,
                 i3, i2, like=pts)
        return i3, i2

    def compute_projection(self, points, depth, camera_to_world):
        """one frame: depth (H,W), camera_to_world (4,4) -> None when nothing maps, else
        (indices_3d, indices_2d), each (N+1) int64"""
        dev = self._device(points, depth, camera_to_world)
        W, H = int(self.image_dims[0]), int(self.image_dims[1])
        dep = _device_f32(depth, dev, "depth", (H, W))
        pose = _device_f32(camera_to_world, dev, "camera_to_world", (4, 4))
        i3, i2 = self.compute_projections(points, dep[None], pose[None])
        if int(i3[0, 0]) == 0:
            return None
        return i3[0], i2[0]

    @torch.no_grad()
    def project(self, label, lin_indices_3d, lin_indices_2d, num_points):
        """label (C,H,W) or (H,W), float32 or bfloat16 -> (C, num_points): column
        lin_indices_3d[k] takes label[:, lin_indices_2d[k]], every other column is zero.  The
        indices are a row of compute_projection's tables (point indices ascending)."""
        dev = self._device(label, lin_indices_3d)
        if not isinstance(label, torch.Tensor):
            label = torch.from_numpy(np.ascontiguousarray(label))
        label = label.detach().to(dev)
        if label.dtype not in (torch.float32, torch.bfloat16):
            label = label.to(torch.float32)
        label = label.contiguous()
        if label.dim() not in (2, 3):
            raise ValueError(f"label: expected (C,H,W) or (H,W), got {tuple(label.shape)}")
        C = 1 if label.dim() == 2 else label.shape[0]
        HW = label.numel() // max(C, 1)
        N = int(num_points)
        i3, i2 = (torch.as_tensor(t).to(device=dev, dtype=torch.int64).contiguous()
                  for t in (lin_indices_3d, lin_indices_2d))
        if i3.shape != (N + 1,) or i2.shape != (N + 1,) or N < 1 or C < 1 or HW < 1:
            raise ValueError(f"indices: expected two ({N + 1},) rows, got {tuple(i3.shape)}, {tuple(i2.shape)}")
        out = torch.empty((C, N), dtype=label.dtype, device=dev)
        nat.call("ov3d_backproj_gather", label, int(label.dtype == torch.bfloat16), C, HW, i3, i2, N,
                 out, like=label)
        return out


_DEFAULT = None


def default_projector():
    """the helper of image_processor: the 41 x 32 feature map, depths 0.1 .. 4.0, accuracy 0.05"""
    global _DEFAULT
    if _DEFAULT is None:
        _DEFAULT = ProjectionHelper(INTRINSICS, 0.1, 4.0, [41, 32], 0.05)
    return _DEFAULT


def compose_features(points, depths, poses, features, rows=False, out=None, projector=None):
    """points (N,3), depths (F,H,W), poses (F,4,4), features (F,C,H,W) float32 or bfloat16
    -> (out, frame): out (C,N), or (N,C) with rows=True (the layout ScanStore(features=...)
    takes), of the features' dtype; frame (N) int32, the frame every vertex took its features
    from, -1 (and a zero column) where no frame maps it.  Equal to

        out = zeros(C, N)
        for i in range(F):
            p = project(features[i], i3d[i], i2d[i], N); idx = i3d[i][1:1 + n_i]; out[:, idx] = p[:, idx]

    over compute_projections' tables (later frames overwrite earlier ones) without forming them:
    two launches, no synchronisation.  projector: a ProjectionHelper (default: image_processor's)."""
    helper = default_projector() if projector is None else projector
    dev = helper._device(points, depths, poses, features)
    W, H = int(helper.image_dims[0]), int(helper.image_dims[1])
    pts = _device_f32(points, dev, "points", (None, 3))
    pose = _device_f32(poses, dev, "poses", (None, 4, 4))
    F, N = pose.shape[0], pts.shape[0]
    dep = _device_f32(depths, dev, "depths", (F, H, W))
    if not isinstance(features, torch.Tensor):
        features = torch.from_numpy(np.ascontiguousarray(features))
    feat = features.detach().to(dev)
    if feat.dtype not in (torch.float32, torch.bfloat16):
        feat = feat.to(torch.float32)
    feat = feat.contiguous()
    if feat.dim() != 4 or feat.shape[0] != F or tuple(feat.shape[2:]) != (H, W):
        raise ValueError(f"features: expected ({F}, C, {H}, {W}), got {tuple(feat.shape)}")
    C = feat.shape[1]
    if N < 1 or F < 1 or C < 1 or N + 1 >= 2 ** 31:
        raise ValueError(f"expected N, F, C >= 1 and N < 2^31 - 1, got N = {N}, F = {F}, C = {C}")
    shape = (N, C) if rows else (C, N)
    if out is None:
        out = torch.empty(shape, dtype=feat.dtype, device=dev)
    nat.check(out, "out", feat.dtype, 2)
    if tuple(out.shape) != shape or out.device != dev:
        raise ValueError(f"out: expected {shape} on {dev}, got {tuple(out.shape)} on {out.device}")
    table = torch.empty((F, ROW), dtype=torch.float32, device=dev)
    frame = torch.empty(N, dtype=torch.int32, device=dev)
    nat.call("ov3d_backproj_compose", pts, N, dep, pose, F, helper.params(dev), W, H, feat,
             int(feat.dtype == torch.bfloat16), C, int(bool(rows)), table, out, frame, like=pts)
    return out, frame
