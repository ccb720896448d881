"""The ScanNet device loader's host side (no GPU): the file reads laid out as
datasets/scannet.py:209-229, 256-270 reads them, the load-time validation, the additive
ScannetDatasetConfig members, and the new C entries' argument checks."""
import ctypes
import os

import numpy as np
import pytest

from helpers import GOLDEN, ov3d  # noqa: F401  (registers the ov3d_amd package)
from ov3d_amd import scannet
from ov3d_amd.dataset_config import ScannetDatasetConfig
from scannet_aug_cases import CASES, NYU40IDS, features, pseudo_boxes, raw_scans, scan_name

GOLD = np.load(os.path.join(GOLDEN, "scannet_aug.npz"))


@pytest.fixture()
def tree(tmp_path):
    root, meta, pdir, fdir = (tmp_path / x for x in ("data", "meta", "pbox", "feat"))
    for x in (root, meta, pdir, fdir):
        x.mkdir()
    scans = raw_scans()[:4]
    for i, (vert, bb) in enumerate(scans):
        np.save(root / (scan_name(i) + "_vert.npy"), vert)
        np.save(root / (scan_name(i) + "_bbox.npy"), bb)
        np.save(pdir / (scan_name(i) + "_bbox.npy"), pseudo_boxes(i))
        feat, inds = features(i, "h16")
        np.save(root / (scan_name(i) + "_inds.npy"), inds)
        np.save(fdir / (scan_name(i) + ".npy"), feat)
    (root / "notes.txt").write_text("not a scan\n")
    # the split lists two scans the directory does not hold, and in its own order
    (meta / "scannetv2_train.txt").write_text("\n".join(
        ["scene0777_00", scan_name(2), scan_name(0), scan_name(3), "scene0999_01", scan_name(1)]) + "\n")
    return dict(root=str(root), meta=str(meta), pdir=str(pdir), fdir=str(fdir), scans=scans)


def test_disk_read_split_filter_features(tree):
    ds = scannet.ScannetDetectionDataset(
        ScannetDatasetConfig(), split_set="train", root_dir=tree["root"], meta_data_dir=tree["meta"],
        feature_2d_dir=tree["fdir"], num_points=256, use_2d_feature=True, device="cpu")
    order = [2, 0, 3, 1]
    assert ds.scan_names == [scan_name(i) for i in order] and len(ds) == 4
    st = ds.store
    assert st.verts.shape == (4, 3000, 6) and st.boxes.shape == (4, 12, 7)
    for s, i in enumerate(order):
        vert, bb = tree["scans"][i]
        assert st.n[s] == vert.shape[0] and st.k[s] == bb.shape[0]
        np.testing.assert_array_equal(st.verts[s, : st.n[s]].numpy(), vert)
        assert float(st.verts[s, st.n[s]:].abs().sum()) == 0
        np.testing.assert_array_equal(st.boxes[s, : st.k[s]].numpy(), bb)
        feat, inds = features(i, "h16")
        np.testing.assert_array_equal(st.features[s, : st.n[s]].numpy(), feat[inds])


def test_disk_read_pbox_replaces_boxes(tree):
    ds = scannet.ScannetDetectionDataset(
        ScannetDatasetConfig(), split_set="train", root_dir=tree["root"], meta_data_dir=tree["meta"],
        pseudo_box_dir=tree["pdir"], use_pbox=True, device="cpu")
    assert ds.max_num_obj == 64 and ds.store.features is None
    for s, i in enumerate([2, 0, 3, 1]):
        pb = pseudo_boxes(i)
        assert ds.store.k[s] == pb.shape[0]
        np.testing.assert_array_equal(ds.store.boxes[s, : pb.shape[0]].numpy(), pb)


def test_refusals():
    scans = raw_scans()[:2]
    cfg = ScannetDatasetConfig()
    with pytest.raises(NotImplementedError):
        scannet.ScannetDetectionDataset(cfg, scans=scans, use_image=True, device="cpu")
    with pytest.raises(NotImplementedError):
        scannet.ScannetDetectionDataset(cfg, scans=scans, use_height=True, device="cpu")
    bad = scans[1][1].copy()
    bad[0, 6] = 13.0                                 # NYU40 id 13 is none of the 18 classes
    assert 13 not in NYU40IDS
    with pytest.raises(ValueError, match="nyu40id2class"):
        scannet.ScannetDetectionDataset(cfg, scans=[scans[0], (scans[1][0], bad)], device="cpu")
    many = np.repeat(scans[1][1], 65, axis=0)[:65]
    with pytest.raises(ValueError, match="max_num_obj"):
        scannet.ScannetDetectionDataset(cfg, scans=[(scans[1][0], many)], device="cpu")
    with pytest.raises(ValueError, match="features"):
        scannet.ScannetDetectionDataset(cfg, scans=scans, use_2d_feature=True, device="cpu")
    # everything else is accepted: the unused RandomCuboid arguments included
    ds = scannet.ScannetDetectionDataset(cfg, scans=scans, use_random_cuboid=False,
                                         random_cuboid_min_points=5, use_color=True, device="cpu")
    assert len(ds) == 2


def test_config_members():
    cfg = ScannetDatasetConfig()
    assert cfg.max_num_obj == 64
    assert list(cfg.nyu40ids) == list(NYU40IDS)
    assert cfg.nyu40id2class == {int(i): c for c, i in enumerate(NYU40IDS)}
    assert len(cfg.nyu40id2class) == cfg.num_semcls


def test_rotate_aligned_boxes_against_golden():
    """the float32 targets are rebuilt from the raw boxes and the case's replayed draws (flips,
    angle); rotating them must give the golden's gt_box_centers / gt_box_sizes bit for bit,
    padded zero rows included"""
    name = "train_xyz"
    case = CASES[name]
    scans = raw_scans()
    rng = np.random.RandomState(case["seed"])
    for j, i in enumerate(case["inds"]):
        n = scans[i][0].shape[0]
        rng.choice(n, 1000, replace=n < 1000)
        fx, fy = rng.random() > 0.5, rng.random() > 0.5
        ang = (rng.random() * np.pi / 18) - np.pi / 36
        c, s = np.cos(ang), np.sin(ang)
        target = np.zeros((64, 6), np.float32)
        target[: len(scans[i][1])] = scans[i][1][:, 0:6]
        if fx:
            target[:, 0] = -1 * target[:, 0]
        if fy:
            target[:, 1] = -1 * target[:, 1]
        got = ScannetDatasetConfig.rotate_aligned_boxes(target, np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]]))
        assert got.dtype == np.float64 and got.shape == (64, 6)
        got = got.astype(np.float32)
        assert np.array_equal(got[:, 0:3].view(np.uint8), GOLD[f"{name}/gt_box_centers"][j].view(np.uint8))
        assert np.array_equal(got[:, 3:6].view(np.uint8), GOLD[f"{name}/gt_box_sizes"][j].view(np.uint8))


def test_box_parametrization_to_corners_np_against_golden():
    name = "val_color"
    cor = ScannetDatasetConfig().box_parametrization_to_corners_np(
        GOLD[f"{name}/gt_box_centers"], GOLD[f"{name}/gt_box_sizes"], GOLD[f"{name}/gt_box_angles"])
    assert np.array_equal(cor.astype(np.float32), GOLD[f"{name}/gt_box_corners"])


def test_scan_entries_reject_bad_arguments():
    """ov3d_scan_sample_aug / ov3d_scan_labels / ov3d_rows_gather validate on the host and
    return -1 before any launch (the fake pointers are never dereferenced)."""
    from ov3d_amd import _native
    lib = _native.load()
    p = ctypes.c_void_p(256)       # 16-byte aligned
    p4 = ctypes.c_void_p(260)      # 4-byte aligned only
    p2 = ctypes.c_void_p(258)      # 2-byte aligned only
    odd = ctypes.c_void_p(257)
    assert lib.ov3d_scan_parts(1000) == 4 and lib.ov3d_scan_parts(1024) == 4

    def sa(**kw):
        a = dict(raw=p, f64=0, n_stride=100, S=2, idx=p, nv=p, ch=p, B=2, N=64, par=p, aug=1, col=1,
                 pc=p, color=p, part=p)
        a.update(kw)
        return lib.ov3d_scan_sample_aug(a["raw"], a["f64"], a["n_stride"], a["S"], a["idx"], a["nv"],
                                        a["ch"], a["B"], a["N"], a["par"], a["aug"], a["col"], a["pc"],
                                        a["color"], a["part"], None)
    for k in ("raw", "idx", "nv", "ch", "par", "pc", "color", "part"):
        assert sa(**{k: None}) == -1, k
    for k in ("n_stride", "S", "B", "N"):
        assert sa(**{k: 0}) == -1, k
    assert sa(B=1 << 16) == -1

    def rg(**kw):
        a = dict(feat=p, rows=100, rb=32, S=2, idx=p, ch=p, B=2, N=64, vec=0, out=p)
        a.update(kw)
        return lib.ov3d_rows_gather(a["feat"], a["rows"], a["rb"], a["S"], a["idx"], a["ch"], a["B"],
                                    a["N"], a["vec"], a["out"], None)
    for k in ("feat", "idx", "ch", "out"):
        assert rg(**{k: None}) == -1, k
    for k in ("rows", "rb", "S", "B", "N"):
        assert rg(**{k: 0}) == -1, k
    assert rg(rb=31) == -1                       # odd row byte count
    assert rg(feat=odd) == -1 and rg(out=odd) == -1
    assert rg(vec=8) == -1                       # no such path
    assert rg(vec=16, rb=28) == -1               # row size against the width asked for
    assert rg(vec=16, feat=p4) == -1 and rg(vec=16, out=p2) == -1
    assert rg(vec=4, rb=10) == -1 and rg(vec=4, feat=p2) == -1

    args = _native.ScanLabelsArgs()              # all zero: null pointers, zero sizes
    assert lib.ov3d_scan_labels(None, None) == -1
    assert lib.ov3d_scan_labels(_native.byref(args), None) == -1
    for n in ("B", "S", "max_num_obj", "k_stride", "n_dims_part", "n_id2class"):
        setattr(args, n, 4)
    assert lib.ov3d_scan_labels(_native.byref(args), None) == -1          # pointers still null
    for n, _ in _native.ScanLabelsArgs._fields_[8:]:
        setattr(args, n, 256)
    args.max_num_obj = 257
    assert lib.ov3d_scan_labels(_native.byref(args), None) == -1
    args.max_num_obj, args.angle_res = 64, None
    assert lib.ov3d_scan_labels(_native.byref(args), None) == -1
