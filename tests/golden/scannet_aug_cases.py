"""Cases of tests/golden/scannet_aug.npz (shared by make_scannet_aug_golden.py and the tests):
raw scans, pseudo boxes and 2D features are regenerated bit-identically from numpy PCG64 seeds."""
import numpy as np

NYU40IDS = np.array([3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14, 16, 24, 28, 33, 34, 36, 39])
NSCAN = 8
NVERT = [3000, 1500, 700, 3000, 1500, 700, 3000, 1500]     # 700 < 1000: sampling with replacement
NBOX = [0, 1, 5, 12, 64, 3, 7, 2]                          # none, and exactly max_num_obj
NPBOX = [2, 0, 64, 5, 1, 9, 3, 4]
NFEAT = 400                                                # rows of a scan's feature file
NUM_POINTS = 1000                                          # no multiple of 64 or 256: tail wave / block

# feature variants: fp16 D=16 rows of 32 B (16-byte path), fp32 D=7 rows of 28 B (4-byte path),
# fp16 D=5 rows of 10 B (2-byte path)
FEATS = {"h16": (np.float16, 16), "f7": (np.float32, 7), "h5": (np.float16, 5)}

# case: split, augment, use_color, seed, scan indices, one generator per scene, use_pbox, feature
CASES = {
    "train_xyz": dict(split="train", augment=True, use_color=False, seed=11, inds=[0, 2, 4, 7],
                      per_scene=False, use_pbox=False, feat=None),
    "train_color": dict(split="train", augment=True, use_color=True, seed=3, inds=[3, 5, 4, 1],
                        per_scene=False, use_pbox=False, feat=None),
    "val_color": dict(split="val", augment=False, use_color=True, seed=5, inds=[6, 2, 0],
                      per_scene=False, use_pbox=False, feat=None),
    "train_per_scene": dict(split="train", augment=True, use_color=False, seed=29, inds=[4, 5, 1],
                            per_scene=True, use_pbox=False, feat=None),
    "train_pbox": dict(split="train", augment=True, use_color=False, seed=31, inds=[2, 1, 6],
                       per_scene=False, use_pbox=True, feat=None),
    "train_color_h16": dict(split="train", augment=True, use_color=True, seed=37, inds=[7, 2],
                            per_scene=False, use_pbox=False, feat="h16"),
    "val_f7": dict(split="val", augment=False, use_color=False, seed=41, inds=[5, 3],
                   per_scene=False, use_pbox=False, feat="f7"),
    "train_h5": dict(split="train", augment=True, use_color=False, seed=43, inds=[1, 5, 0],
                     per_scene=False, use_pbox=False, feat="h5"),
}


def scan_name(i):
    return "scene%04d_00" % i


def _boxes(rng, k):
    ctr = np.stack([rng.uniform(-3.5, 3.5, k), rng.uniform(-2.5, 2.5, k), rng.uniform(0.2, 2.2, k)], 1)
    length = rng.uniform(0.2, 2.0, size=(k, 3))
    cls = NYU40IDS[rng.integers(0, len(NYU40IDS), k)].astype(np.float64)
    return np.concatenate([ctr, length, cls[:, None]], 1)


def raw_scan(i, dtype=np.float32):
    """scan i: vertices (n, 6) (xyz in a room-sized box, integer colours 0..255), boxes (k, 7)"""
    rng = np.random.Generator(np.random.PCG64(5000 + i))
    n = NVERT[i]
    xyz = np.stack([rng.uniform(-4.0, 4.0, n), rng.uniform(-3.0, 3.0, n), rng.uniform(0.0, 2.7, n)], 1)
    rgb = rng.integers(0, 256, (n, 3)).astype(np.float64)
    return np.concatenate([xyz, rgb], 1).astype(dtype), _boxes(rng, NBOX[i])


def raw_scans(dtype=np.float32):
    return [raw_scan(i, dtype) for i in range(NSCAN)]


def pseudo_boxes(i):
    """the use_pbox file of scan i (k, 7)"""
    return _boxes(np.random.Generator(np.random.PCG64(6000 + i)), NPBOX[i])


def features(i, kind):
    """-> (feature file (NFEAT, D), pre_subsample_inds (n,)) of scan i"""
    dt, d = FEATS[kind]
    rng = np.random.Generator(np.random.PCG64(7000 + i))
    feat = rng.standard_normal((NFEAT, d)).astype(dt)
    return feat, rng.integers(0, NFEAT, NVERT[i])
