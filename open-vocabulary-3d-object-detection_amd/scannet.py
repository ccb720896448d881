"""ScanNet training / evaluation batches built on the device.

Drop-in for datasets/scannet.py:172 ``ScannetDetectionDataset`` (same leading constructor
arguments): the raw scans are loaded once (np.load of ``{scan}_vert.npy`` / ``{scan}_bbox.npy``
as the reference does, scannet.py:256-270) and kept resident in HBM; ``get_batch(indices)``
returns the collated batch dict of the reference's ``__getitem__`` (scannet.py:256-417) as
device tensors, built by the HIP kernels of csrc/scanaug.hip: one launch samples, augments and
writes the points and colours, one builds every label tensor, and with ``use_2d_feature`` one
gathers the feature rows.

Random draws: the reference's numpy calls, in the reference's order, on ``rng`` (the global
``np.random`` by default, as the reference's workers use), so the same seed gives the
reference's batch bit for bit:
  per scene   choice(n, num_points, replace=n < num_points)   (sampling comes first, :319-321)
              and with augment: random() (x flip), random() (y flip), random() (rotation).
There is no RandomCuboid (commented out in the reference, :309-317: ``use_random_cuboid`` and
``random_cuboid_min_points`` are accepted and unused), so the whole plan is known on the host
before the first launch and ``get_batch`` never reads anything back from the device.

Scope: ``use_image`` (the multiview frame loader; needs imageio and torchvision) and
``use_height`` (never passed by build_dataset) raise NotImplementedError; the per-vertex
features themselves come from ``ov3d_amd.projection.compose_features``.  ``use_pbox`` reads the
boxes from ``pseudo_box_dir`` instead (scannet.py:264-267).  ``pcl_color`` holds the raw colours,
or with ``use_color`` the normalised ones (in the reference it is a view of the normalised array).

Memory: the vertices take S x n_max x 6 elements (1201 training scans of 50000 float32 vertices:
1.4 GB).  With ``use_2d_feature`` the per-vertex features ``feature_2d[pre_subsample_inds]``
(scannet.py:333) are composed once on the host at load, so a batch needs a single-level row
gather; resident they take S x n_max x D elements: 1201 scans x 50000 vertices x 512 fp16 is
61 GB of the 288 GB HBM (the uncomposed per-scan files are smaller by the factor
len(feature_2d) / len(pre_subsample_inds)).
"""
import os

import numpy as np
import torch

from . import _native as nat

# the reference's defaults for arguments left None (scannet.py:26-32, 194-204)
DATASET_ROOT_DIR = "/share/suzhengyuan/code/ScanRefer-3DVG/votenet/scannet/scannet_train_detection_data"
DATASET_METADATA_DIR = "/share/suzhengyuan/code/ScanRefer-3DVG/votenet/scannet/meta_data"
FEATURE_2D_PATH = "/data/suzhengyuan/ScanRefer/LSeg_data"
PSEUDO_BOX_PATH = ""


class ScanStore:
    """Raw scans resident on `device`: vertices (S, n_max, 6) of the scans' dtype, boxes
    (S, k_max, 7) float64, per-scan counts, and optionally per-vertex features (S, n_max, D)."""

    def __init__(self, scans, device, features=None):
        verts, boxes = [np.asarray(s[0]) for s in scans], [np.asarray(s[1]) for s in scans]
        dt = verts[0].dtype
        if any(v.dtype != dt for v in verts) or dt not in (np.float32, np.float64):
            raise TypeError("scans must share one float32 / float64 vertex dtype")
        if any(v.ndim != 2 or v.shape[1] < 6 for v in verts):
            raise ValueError("vertices must be (n, 6+): xyz + rgb")
        self.pc_f64 = int(dt == np.float64)
        self.n = np.array([v.shape[0] for v in verts], np.int32)
        self.k = np.array([b.shape[0] for b in boxes], np.int32)
        self.n_max = int(self.n.max())
        self.k_max = max(int(self.k.max()), 1)
        S = len(verts)
        vt = np.zeros((S, self.n_max, 6), dt)
        bx = np.zeros((S, self.k_max, 7), np.float64)
        for i, (v, b) in enumerate(zip(verts, boxes)):
            vt[i, : v.shape[0]] = v[:, 0:6]
            if b.shape[0]:
                bx[i, : b.shape[0], 0:6] = b[:, 0:6]
                bx[i, : b.shape[0], 6] = b[:, -1]
        self.device = torch.device(device)
        self.verts = torch.as_tensor(vt).to(self.device)
        self.boxes = torch.as_tensor(bx).to(self.device)
        self.n_dev = torch.as_tensor(self.n).to(self.device)
        self.k_dev = torch.as_tensor(self.k).to(self.device)
        self.features = None
        if features is not None:
            f0 = features[0]
            if any(f.dtype != f0.dtype or f.shape[1:] != f0.shape[1:] or f.ndim != 2 for f in features):
                raise ValueError("feature_2d arrays must share one dtype and row length")
            ft = torch.zeros((S, self.n_max, f0.shape[1]), dtype=torch.from_numpy(
                np.zeros(0, f0.dtype)).dtype, device=self.device)
            for i, f in enumerate(features):
                if f.shape[0] != self.n[i]:
                    raise ValueError("feature_2d[pre_subsample_inds] must have one row per vertex")
                ft[i, : f.shape[0]].copy_(torch.from_numpy(np.ascontiguousarray(f)))
            self.features = ft


class ScannetDetectionDataset:
    """datasets/scannet.py:172-251 constructor; scans resident on `device`.

    `scans` (list of (vertices (n, 6), bboxes (k, 7)) arrays) replaces reading ``root_dir``
    (synthetic data, tests); `extras` then holds per scan {"feature_2d": (m, D) array and
    optionally "pre_subsample_inds": (n,) indices into it}.  Batches:
    ``get_batch(indices, rng=np.random)``."""

    def __init__(self, dataset_config, split_set="train", root_dir=None, meta_data_dir=None,
                 pseudo_box_dir=None, feature_2d_dir=None, num_points=40000, use_color=False,
                 use_image=False, use_height=False, augment=False, use_random_cuboid=True,
                 random_cuboid_min_points=30000, use_pbox=False, use_2d_feature=False,
                 device="cuda", scans=None, extras=None):
        assert split_set in ["train", "val"]
        if use_image:
            raise NotImplementedError("use_image: the multiview frame loader (imageio, "
                                      "torchvision) is not part of the point-cloud path")
        if use_height:
            raise NotImplementedError("use_height is never enabled by build_dataset")
        self.dataset_config = dataset_config
        self.num_points = num_points
        self.use_color = use_color
        self.augment = augment
        self.use_pbox = use_pbox
        self.use_2d_feature = use_2d_feature
        self.use_random_cuboid = use_random_cuboid           # accepted, unused (scannet.py:309-317)
        self.random_cuboid_min_points = random_cuboid_min_points
        self.max_num_obj = 64                                 # MAX_NUM_PSEUDO_BOX too (:33, :251)
        if scans is None:
            scans, extras, self.scan_names = self._read(
                DATASET_ROOT_DIR if root_dir is None else root_dir,
                DATASET_METADATA_DIR if meta_data_dir is None else meta_data_dir, split_set, use_pbox,
                PSEUDO_BOX_PATH if pseudo_box_dir is None else pseudo_box_dir, use_2d_feature,
                FEATURE_2D_PATH if feature_2d_dir is None else feature_2d_dir)
        else:
            self.scan_names = [f"scene{i:04d}_00" for i in range(len(scans))]
        if not scans:
            raise ValueError("no scans")
        features = None
        if use_2d_feature:
            if not extras or any("feature_2d" not in e for e in extras):
                raise ValueError("use_2d_feature: no features (extras=)")
            features = [np.asarray(e["feature_2d"])[np.asarray(e["pre_subsample_inds"])]
                        if "pre_subsample_inds" in e else np.asarray(e["feature_2d"]) for e in extras]
        self._id2class = self._validate(scans, dataset_config, self.max_num_obj, self.scan_names)
        self.store = ScanStore(scans, device, features)
        self._id2class_dev = torch.as_tensor(self._id2class).to(self.store.device)

    @staticmethod
    def _validate(scans, cfg, max_num_obj, names):
        """host checks of what the reference fails on per item: a class id outside
        nyu40id2class (KeyError at scannet.py:402-405) and more boxes than MAX_NUM_OBJ (the
        broadcast at :335-336).  -> the id -> class table the label kernel reads."""
        table = np.full(int(max(cfg.nyu40id2class)) + 1, -1, np.int32)
        for i, c in cfg.nyu40id2class.items():
            table[int(i)] = c
        for name, s in zip(names, scans):
            bb = np.asarray(s[1])
            if bb.ndim != 2 or (bb.shape[0] and bb.shape[1] < 7):
                raise ValueError(f"{name}: boxes must be (k, 7)")
            if bb.shape[0] > max_num_obj:
                raise ValueError(f"{name}: {bb.shape[0]} boxes, more than max_num_obj = {max_num_obj}")
            for x in (bb[:, -1] if bb.shape[0] else ()):
                if int(x) not in cfg.nyu40id2class:
                    raise ValueError(f"{name}: box class id {x!r} is not in nyu40id2class")
        return table

    @staticmethod
    def _read(root_dir, meta_data_dir, split_set, use_pbox, pseudo_box_dir, use_2d_feature,
              feature_2d_dir):
        """the reference's file reads (scannet.py:209-229, 256-270); allow_pickle stays off"""
        present = set(os.path.basename(x)[0:12] for x in os.listdir(root_dir) if x.startswith("scene"))
        with open(os.path.join(meta_data_dir, f"scannetv2_{split_set}.txt")) as f:
            listed = f.read().splitlines()
        names = [n for n in listed if n in present]
        scans, extras = [], []
        for n in names:
            p = os.path.join(root_dir, n)
            vert = np.load(p + "_vert.npy")
            box_dir = pseudo_box_dir if use_pbox else root_dir
            scans.append((vert, np.load(os.path.join(box_dir, n) + "_bbox.npy")))
            if use_2d_feature:
                extras.append({"pre_subsample_inds": np.load(p + "_inds.npy"),
                               "feature_2d": np.load(os.path.join(feature_2d_dir, n) + ".npy")})
        return scans, extras, names

    def __len__(self):
        return len(self.scan_names)

    def _draw(self, rng, n, choices_row, params_row):
        """one scene's draws, in the reference's order (scannet.py:319-321, 341-352)"""
        choices_row[:] = rng.choice(n, self.num_points, replace=n < self.num_points)
        if self.augment:
            flip_x = rng.random() > 0.5
            flip_y = rng.random() > 0.5
            rot_angle = (rng.random() * np.pi / 18) - np.pi / 36
            params_row[0:4] = [float(flip_x), float(flip_y), np.cos(rot_angle), np.sin(rot_angle)]

    def get_batch(self, indices, rng=None, rngs=None):
        """Collated reference batch for scans `indices` (device tensors).

        rng: one numpy RandomState-like generator drawn scene after scene (the reference's
        per-worker np.random); rngs: one generator per scene instead.  Three launches (two
        without use_2d_feature) behind three host -> device copies; nothing is read back."""
        st = self.store
        dev = st.device
        B, N, G = len(indices), self.num_points, self.max_num_obj
        if rngs is None:
            rngs = [rng if rng is not None else np.random] * B
        assert len(rngs) == B
        ind = np.asarray(indices, np.int64)
        if B == 0 or ind.min() < 0 or ind.max() >= len(self):
            raise IndexError("scan index out of range")
        choices = np.empty((B, N), np.int64)
        params = np.zeros((B, 8))
        for b in range(B):
            self._draw(rngs[b], int(st.n[ind[b]]), choices[b], params[b])
        idx = torch.as_tensor(ind).to(dev)
        ch = torch.as_tensor(choices).to(dev)
        par = torch.as_tensor(params).to(dev)
        T = torch.float64 if st.pc_f64 else torch.float32
        S = int(st.verts.shape[0])
        C = 6 if self.use_color else 3
        nparts = nat.load().ov3d_scan_parts(N)
        f32 = dict(dtype=torch.float32, device=dev)
        i64 = dict(dtype=torch.int64, device=dev)
        dpart = torch.empty((B, nparts, 6), dtype=T, device=dev)
        out = {
            "point_clouds": torch.empty((B, N, C), **f32),
            "gt_box_corners": torch.empty((B, G, 8, 3), **f32),
            "gt_box_centers": torch.empty((B, G, 3), **f32),
            "gt_box_centers_normalized": torch.empty((B, G, 3), **f32),
            "gt_angle_class_label": torch.empty((B, G), **i64),
            "gt_angle_residual_label": torch.empty((B, G), **f32),
            "gt_box_sem_cls_label": torch.empty((B, G), **i64),
            "gt_box_present": torch.empty((B, G), **f32),
            "scan_idx": idx,
            "pcl_color": torch.empty((B, N, 3), dtype=T, device=dev),
        }
        if self.use_2d_feature:
            out["feature_2d"] = torch.empty((B, N, st.features.shape[2]), dtype=st.features.dtype,
                                            device=dev)
        out.update({
            "gt_box_sizes": torch.empty((B, G, 3), **f32),
            "gt_box_sizes_normalized": torch.empty((B, G, 3), **f32),
            "gt_box_angles": torch.empty((B, G), **f32),
            "point_cloud_dims_min": torch.empty((B, 3), **f32),
            "point_cloud_dims_max": torch.empty((B, 3), **f32),
        })
        nat.call("ov3d_scan_sample_aug", st.verts, st.pc_f64, st.n_max, S, idx, st.n_dev, ch, B, N,
                 par, int(self.augment), int(self.use_color), out["point_clouds"], out["pcl_color"],
                 dpart, like=st.verts)
        args = nat.ScanLabelsArgs(
            B=B, S=S, max_num_obj=G, k_stride=st.k_max, augment=int(self.augment), n_dims_part=nparts,
            n_id2class=int(self._id2class_dev.numel()), pc_f64=st.pc_f64, boxes=st.boxes.data_ptr(),
            nbox=st.k_dev.data_ptr(), scene_idx=idx.data_ptr(), params=par.data_ptr(),
            dims_part=dpart.data_ptr(), id2class=self._id2class_dev.data_ptr(),
            dims_min=out["point_cloud_dims_min"].data_ptr(),
            dims_max=out["point_cloud_dims_max"].data_ptr(),
            corners=out["gt_box_corners"].data_ptr(), centers=out["gt_box_centers"].data_ptr(),
            centers_normalized=out["gt_box_centers_normalized"].data_ptr(),
            sem_cls=out["gt_box_sem_cls_label"].data_ptr(), present=out["gt_box_present"].data_ptr(),
            sizes=out["gt_box_sizes"].data_ptr(),
            sizes_normalized=out["gt_box_sizes_normalized"].data_ptr(),
            angles=out["gt_box_angles"].data_ptr(), angle_cls=out["gt_angle_class_label"].data_ptr(),
            angle_res=out["gt_angle_residual_label"].data_ptr())
        nat.call("ov3d_scan_labels", nat.byref(args), like=st.verts)
        if self.use_2d_feature:
            rows_gather(st.features, idx, ch, out=out["feature_2d"])
        return out

    def __getitem__(self, idx):
        """one scene through the device path, as the reference's numpy dict"""
        return {k: v[0].cpu().numpy() for k, v in self.get_batch([idx]).items()}


def rows_gather(feat, scene_idx, choices, out=None, vec_bytes=0):
    """out[b, j, :] = feat[scene_idx[b], choices[b, j], :] in one launch (ov3d_rows_gather).

    feat (S, R, D) of any dtype whose rows are an even number of bytes, scene_idx (B) and
    choices (B, N) int64, all on the device; vec_bytes 16 / 4 / 2 forces the access width
    (0: the widest the row size and the base pointers allow)."""
    nat.check_device(feat, "feat")
    nat.check(scene_idx, "scene_idx", torch.int64, 1)
    nat.check(choices, "choices", torch.int64, 2)
    if feat.dim() != 3 or feat.stride(2) != 1 or feat.stride(1) != feat.shape[2] or \
            feat.stride(0) != feat.shape[1] * feat.shape[2]:
        raise ValueError("feat: expected a dense (S, R, D) tensor")
    B, N = choices.shape
    if scene_idx.shape[0] != B:
        raise ValueError("scene_idx and choices disagree on the batch size")
    if out is None:
        out = torch.empty((B, N, feat.shape[2]), dtype=feat.dtype, device=feat.device)
    elif out.shape != (B, N, feat.shape[2]) or out.dtype != feat.dtype or out.stride() != (
            N * feat.shape[2], feat.shape[2], 1):
        raise ValueError("out: expected a dense (B, N, D) tensor of feat's dtype")
    nat.call("ov3d_rows_gather", feat, int(feat.shape[1]), int(feat.shape[2]) * feat.element_size(),
             int(feat.shape[0]), scene_idx, choices, B, N, int(vec_bytes), out, like=feat)
    return out
