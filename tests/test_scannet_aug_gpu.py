"""Device ScanNet batches (ov3d_amd.scannet, csrc/scanaug.hip) against the REFERENCE loader's own
outputs (tests/golden/scannet_aug.npz, made by tests/golden/make_scannet_aug_golden.py from
datasets/scannet.py:256-417 with the same numpy seeds).

Bar: identical key set, dtypes and shapes; every array bit-exact as bytes, except
gt_box_corners, compared by value (np.array_equal): its products with sin = 0 can differ in the
sign of an exact zero.  No ulp allowance anywhere: at angle 0 nothing evaluates cos / sin.

Not covered: a row gather whose element offsets pass 2^31.  With 2-byte elements that needs a
4 GB table, far above what a quick test may allocate; the kernel computes every offset in 64 bits
and in units of the access width (csrc/scanaug.hip rows_gather_kernel).
"""
import os

import numpy as np
import pytest
import torch

from helpers import GOLDEN, ov3d  # noqa: F401  (registers the ov3d_amd package)
from ov3d_amd import scannet
from ov3d_amd.dataset_config import ScannetDatasetConfig
from scannet_aug_cases import CASES, NUM_POINTS, NYU40IDS, features, pseudo_boxes, raw_scans
from scannet_aug_ref import scannet_item

pytestmark = pytest.mark.gpu
GOLD = np.load(os.path.join(GOLDEN, "scannet_aug.npz"))


def _dataset(case):
    scans = raw_scans()
    if case["use_pbox"]:
        scans = [(v, pseudo_boxes(i)) for i, (v, _) in enumerate(scans)]
    extras = None
    if case["feat"]:
        extras = []
        for i in range(len(scans)):
            feat, inds = features(i, case["feat"])
            extras.append({"feature_2d": feat, "pre_subsample_inds": inds})
    return scannet.ScannetDetectionDataset(
        ScannetDatasetConfig(), split_set=case["split"], num_points=NUM_POINTS,
        use_color=case["use_color"], augment=case["augment"], use_pbox=case["use_pbox"],
        use_2d_feature=bool(case["feat"]), device="cuda", scans=scans, extras=extras)


def _same_bytes(got, ref):
    return np.array_equal(np.ascontiguousarray(got).view(np.uint8), np.ascontiguousarray(ref).view(np.uint8))


@pytest.mark.parametrize("name", sorted(CASES))
def test_device_batch_equals_reference_loader(name):
    case = CASES[name]
    ds = _dataset(case)
    inds = case["inds"]
    if case["per_scene"]:
        out = ds.get_batch(inds, rngs=[np.random.RandomState(case["seed"] * 100 + j)
                                       for j in range(len(inds))])
    else:
        out = ds.get_batch(inds, rng=np.random.RandomState(case["seed"]))
    torch.cuda.synchronize()
    keys = [k.split("/", 1)[1] for k in GOLD.files if k.startswith(name + "/")]
    assert set(keys) == set(out), sorted(set(keys) ^ set(out))
    for k in keys:
        ref = GOLD[f"{name}/{k}"]
        got = out[k].cpu().numpy()
        assert got.shape == ref.shape, (k, got.shape, ref.shape)
        assert got.dtype == ref.dtype, (k, got.dtype, ref.dtype)
        if k == "gt_box_corners":
            assert np.array_equal(got, ref), (k, np.argwhere(got != ref)[:5])
        else:
            assert _same_bytes(got, ref), (k, np.argwhere(got != ref)[:5], got[got != ref][:5],
                                           ref[got != ref][:5])


def test_shared_rng_state_after_batch_matches_reference_draw_count():
    """after a batch, the generator sits exactly where the reference's per-scene draws leave it:
    two half batches from one generator equal the full batch from a fresh one"""
    case = CASES["train_color"]
    ds = _dataset(case)
    inds = case["inds"]
    r1 = np.random.RandomState(case["seed"])
    a = ds.get_batch(inds[:2], rng=r1)
    b = ds.get_batch(inds[2:], rng=r1)
    r2 = np.random.RandomState(case["seed"])
    full = ds.get_batch(inds, rng=r2)
    for k in full:
        assert torch.equal(torch.cat([a[k], b[k]]), full[k]), k
    assert r1.get_state()[2] == r2.get_state()[2]
    assert np.array_equal(r1.get_state()[1], r2.get_state()[1])


def test_getitem_is_one_scene_as_numpy():
    case = CASES["val_color"]
    ds = _dataset(case)
    saved = np.random.get_state()
    np.random.seed(case["seed"])                 # the default generator is the global one
    try:
        item = ds[case["inds"][0]]
    finally:
        np.random.set_state(saved)
    for k, v in item.items():
        assert isinstance(v, np.ndarray)
        assert _same_bytes(v, GOLD[f"val_color/{k}"][0]) or k == "gt_box_corners", k
    assert np.array_equal(item["gt_box_corners"], GOLD["val_color/gt_box_corners"][0])


# ---- ov3d_rows_gather directly, against torch indexing ----
def _gather_case(dtype, D, S=3, R=700, B=2, N=1000, vec=0, shift=0, seed=0):
    """feat (S, R, D) of dtype, with its base pointer moved `shift` elements into a larger
    allocation; choices drawn with replacement (duplicates)"""
    g = torch.Generator().manual_seed(seed)
    flat = torch.randn(S * R * D + 8, generator=g).to(dtype).cuda()
    feat = flat[shift: shift + S * R * D].view(S, R, D)
    idx = torch.randint(0, S, (B,), generator=g).cuda()
    ch = torch.randint(0, R, (B, N), generator=g).cuda()
    if N > 1:
        ch[:, 1] = ch[:, 0]                      # duplicate rows in any case
    ch[:, -1] = R - 1
    out = scannet.rows_gather(feat, idx, ch, vec_bytes=vec)
    torch.cuda.synchronize()
    ref = feat[idx[:, None], ch]
    assert out.shape == (B, N, D) and out.dtype == dtype
    assert torch.equal(out.view(torch.uint8), ref.contiguous().view(torch.uint8))


@pytest.mark.parametrize("dtype,D,vec", [
    (torch.float16, 16, 0),      # 32-byte rows: 16-byte path
    (torch.float32, 7, 0),       # 28-byte rows: 4-byte path
    (torch.float16, 5, 0),       # 10-byte rows: 2-byte path
    (torch.float16, 512, 0),     # 1 KB rows: a wave per row, 16-byte path
    (torch.float16, 200, 0),     # 400-byte rows: 25 units of 16 B, no power of two
    (torch.float16, 16, 4),      # narrower paths forced on an aligned table
    (torch.float16, 16, 2),
    (torch.float32, 130, 4),     # rows longer than 64 units on the 4-byte path
])
def test_rows_gather_paths(dtype, D, vec):
    _gather_case(dtype, D, vec=vec)


def test_rows_gather_shifted_base_pointer_takes_narrow_path():
    _gather_case(torch.float16, 16, shift=1)     # base 2 bytes past a 16-byte boundary
    _gather_case(torch.float16, 16, shift=2)     # 4 bytes past: the 4-byte path
    from ov3d_amd import _native
    flat = torch.zeros(3 * 8 * 16 + 8, dtype=torch.float16, device="cuda")
    feat = flat[1: 1 + 3 * 8 * 16].view(3, 8, 16)
    idx = torch.zeros(1, dtype=torch.int64, device="cuda")
    ch = torch.zeros((1, 4), dtype=torch.int64, device="cuda")
    with pytest.raises(_native.NativeError):     # the wide path asked for on that pointer
        scannet.rows_gather(feat, idx, ch, vec_bytes=16)


def test_rows_gather_single_scene_single_row():
    _gather_case(torch.float16, 64, S=1, R=5, B=1, N=1)
    _gather_case(torch.float32, 3, S=2, R=9, B=1, N=257)


def test_full_size_batch_equals_restatement():
    """the real shape: 8 scans of 50000 vertices -> 40000 points with colour, augmentation and
    fp16 D=64 features, against the numpy restatement (tests/scannet_aug_ref.py, pinned to the
    reference by tests/test_scannet_aug_ref_cpu.py)"""
    cfg = ScannetDatasetConfig()
    scans, extras = [], []
    for i in range(8):
        g = np.random.Generator(np.random.PCG64(300 + i))
        n, k = 50000, [0, 3, 64, 9, 1, 17, 30, 5][i]
        xyz = np.stack([g.uniform(-4, 4, n), g.uniform(-3, 3, n), g.uniform(0, 2.7, n)], 1)
        vert = np.concatenate([xyz, g.integers(0, 256, (n, 3)).astype(np.float64)], 1).astype(np.float32)
        bb = np.concatenate([g.uniform(-2.5, 2.5, (k, 3)), g.uniform(0.2, 2.0, (k, 3)),
                             NYU40IDS[g.integers(0, 18, k)].astype(np.float64)[:, None]], 1)
        scans.append((vert, bb))
        extras.append({"feature_2d": g.standard_normal((n, 64)).astype(np.float16)})
    ds = scannet.ScannetDetectionDataset(cfg, split_set="train", use_color=True, augment=True,
                                         use_2d_feature=True, device="cuda", scans=scans, extras=extras)
    inds = [5, 2, 7, 0, 1, 6, 3, 4]
    out = ds.get_batch(inds, rng=np.random.RandomState(123))
    rng = np.random.RandomState(123)
    ref = [scannet_item(*scans[i], rng, cfg.nyu40id2class, num_points=40000, use_color=True,
                        augment=True, feature=extras[i]["feature_2d"]) for i in inds]
    assert set(out) == set(ref[0]) | {"scan_idx"}
    assert out["scan_idx"].cpu().tolist() == inds
    for k in ref[0]:
        r = np.stack([x[k] for x in ref])
        g = out[k].cpu().numpy()
        assert g.shape == r.shape and g.dtype == r.dtype, k
        if k == "gt_box_corners":
            assert np.array_equal(g, r), k
        else:
            assert _same_bytes(g, r), (k, np.argwhere(g != r)[:5])


def test_float64_vertices_keep_numpy_dtypes():
    """float64 scan files: pcl_color stays float64, the rest is float32 as the reference casts
    it; against the restatement on the same float64 scans"""
    cfg = ScannetDatasetConfig()
    scans = raw_scans(np.float64)
    ds = scannet.ScannetDetectionDataset(cfg, split_set="train", num_points=NUM_POINTS, use_color=True,
                                         augment=True, device="cuda", scans=scans)
    inds = [2, 4, 0, 7]
    out = ds.get_batch(inds, rng=np.random.RandomState(9))
    rng = np.random.RandomState(9)
    ref = [scannet_item(*scans[i], rng, cfg.nyu40id2class, num_points=NUM_POINTS, use_color=True,
                        augment=True) for i in inds]
    assert out["pcl_color"].dtype == torch.float64
    for k in ref[0]:
        r = np.stack([x[k] for x in ref])
        g = out[k].cpu().numpy()
        assert g.dtype == r.dtype, (k, g.dtype, r.dtype)
        assert np.array_equal(g, r) if k == "gt_box_corners" else _same_bytes(g, r), k


def test_refusals_on_device():
    scans = raw_scans()[:2]
    cfg = ScannetDatasetConfig()
    with pytest.raises(NotImplementedError):
        scannet.ScannetDetectionDataset(cfg, scans=scans, use_image=True)
    with pytest.raises(NotImplementedError):
        scannet.ScannetDetectionDataset(cfg, scans=scans, use_height=True)
    bad = scans[1][1].copy()
    bad[0, 6] = 13.0
    with pytest.raises(ValueError):
        scannet.ScannetDetectionDataset(cfg, scans=[scans[0], (scans[1][0], bad)])
    with pytest.raises(ValueError):
        scannet.ScannetDetectionDataset(cfg, scans=[(scans[1][0], np.repeat(scans[1][1], 65, axis=0))])
