"""Golden batches of the REFERENCE ScanNet loader (datasets/scannet.py:256-417) for the device
pipeline (ov3d_amd.scannet, csrc/scanaug.hip).  Run where the reference checkout exists:

    python tests/golden/make_scannet_aug_golden.py      # -> tests/golden/scannet_aug.npz

Raw scans come from scannet_aug_cases.py (numpy PCG64 seeds, regenerated bit-identically by the
tests), written as the reference's ``{scan}_vert.npy`` / ``{scan}_bbox.npy`` / ``{scan}_inds.npy``,
feature and split files into a temporary directory and read by the reference's own
ScannetDetectionDataset.  Each case seeds numpy's global generator (np.random.seed) exactly as the
test seeds the RandomState it passes.
"""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from ref_loader import load_reference  # noqa: E402
from scannet_aug_cases import (CASES, NSCAN, NUM_POINTS, NVERT, features, pseudo_boxes,  # noqa: E402
                               raw_scans, scan_name)


def _plan(case):
    """replay of the case's draws -> per scene (flip_x, flip_y), for the input conditions below"""
    flips = []
    rng = np.random.RandomState(case["seed"])
    for j, i in enumerate(case["inds"]):
        if case["per_scene"]:
            rng = np.random.RandomState(case["seed"] * 100 + j)
        rng.choice(NVERT[i], NUM_POINTS, replace=NVERT[i] < NUM_POINTS)
        if case["augment"]:
            flips.append((bool(rng.random() > 0.5), bool(rng.random() > 0.5)))
            rng.random()
    return flips


def main():
    load_reference()
    import datasets.scannet as scannet
    res = {}
    flips, replaced = set(), False
    with tempfile.TemporaryDirectory() as tmp:
        for name, case in CASES.items():
            root, meta, pdir, fdir = (os.path.join(tmp, name, x) for x in ("data", "meta", "pbox", "feat"))
            for x in (root, meta, pdir, fdir):
                os.makedirs(x)
            for i, (vert, bb) in enumerate(raw_scans()):
                p = os.path.join(root, scan_name(i))
                np.save(p + "_vert.npy", vert)
                np.save(p + "_bbox.npy", bb)
                np.save(os.path.join(pdir, scan_name(i)) + "_bbox.npy", pseudo_boxes(i))
                if case["feat"]:
                    feat, inds = features(i, case["feat"])
                    np.save(p + "_inds.npy", inds)
                    np.save(os.path.join(fdir, scan_name(i)) + ".npy", feat)
            with open(os.path.join(meta, "scannetv2_%s.txt" % case["split"]), "w") as f:
                # two listed scans are absent from the directory (scannet.py:224-228 drops them)
                f.write("\n".join(["scene9998_00"] + [scan_name(i) for i in range(NSCAN)]
                                  + ["scene9999_00"]) + "\n")
            ds = scannet.ScannetDetectionDataset(
                scannet.ScannetDatasetConfig(), split_set=case["split"], root_dir=root,
                meta_data_dir=meta, pseudo_box_dir=pdir, feature_2d_dir=fdir, num_points=NUM_POINTS,
                use_color=case["use_color"], augment=case["augment"], use_pbox=case["use_pbox"],
                use_2d_feature=bool(case["feat"]))
            assert ds.scan_names == [scan_name(i) for i in range(NSCAN)]
            np.random.seed(case["seed"])
            items = []
            for j, i in enumerate(case["inds"]):
                if case["per_scene"]:
                    np.random.seed(case["seed"] * 100 + j)
                items.append(ds[i])
            for k in items[0]:
                res[f"{name}/{k}"] = np.stack([it[k] for it in items])
            flips.update(_plan(case))
            replaced |= any(NVERT[i] < NUM_POINTS for i in case["inds"])
    # conditions on the inputs (not tolerances): every flip combination and the replacement path
    assert flips == {(False, False), (False, True), (True, False), (True, True)}, sorted(flips)
    assert replaced
    out = os.path.join(HERE, "scannet_aug.npz")
    np.savez_compressed(out, **res)
    print("wrote", out, len(res), "arrays,", os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
