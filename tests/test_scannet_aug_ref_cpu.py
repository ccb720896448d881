"""tests/scannet_aug_ref.py (the numpy restatement the full-size GPU test compares against) is
pinned bit for bit to the REFERENCE loader's own outputs (tests/golden/scannet_aug.npz) on
every case, gt_box_corners included.  No GPU."""
import os

import numpy as np
import pytest

from helpers import GOLDEN, ov3d  # noqa: F401  (registers the ov3d_amd package)
from ov3d_amd.dataset_config import ScannetDatasetConfig
from scannet_aug_cases import CASES, NUM_POINTS, features, pseudo_boxes, raw_scans
from scannet_aug_ref import scannet_item

GOLD = np.load(os.path.join(GOLDEN, "scannet_aug.npz"))


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_equals_reference_loader(name):
    case = CASES[name]
    scans = raw_scans()
    id2class = ScannetDatasetConfig().nyu40id2class
    rng = np.random.RandomState(case["seed"])
    items = []
    for j, i in enumerate(case["inds"]):
        if case["per_scene"]:
            rng = np.random.RandomState(case["seed"] * 100 + j)
        feat = None
        if case["feat"]:
            table, inds = features(i, case["feat"])
            feat = table[inds]
        boxes = pseudo_boxes(i) if case["use_pbox"] else scans[i][1]
        items.append(scannet_item(scans[i][0], boxes, rng, id2class, num_points=NUM_POINTS,
                                  use_color=case["use_color"], augment=case["augment"], feature=feat))
        items[-1]["scan_idx"] = np.array(i).astype(np.int64)
    keys = [k.split("/", 1)[1] for k in GOLD.files if k.startswith(name + "/")]
    assert set(keys) == set(items[0]), sorted(set(keys) ^ set(items[0]))
    for k in keys:
        ref = GOLD[f"{name}/{k}"]
        got = np.stack([it[k] for it in items])
        assert got.shape == ref.shape and got.dtype == ref.dtype, (k, got.shape, got.dtype, ref.dtype)
        assert np.array_equal(np.ascontiguousarray(got).view(np.uint8), ref.view(np.uint8)), (
            k, np.argwhere(got != ref)[:5])
