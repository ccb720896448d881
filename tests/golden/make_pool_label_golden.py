"""Writes tests/golden/pool_label.npz: the REFERENCE's own `labeling`
(3DOVDet_tools/scannet/assign_box_label_from_gt.py) and `match`
(3DOVDet_tools/scannet/assess_pseudo_label.py), loaded by file path, unchanged, run over
pool_label_cases.py on a temporary file tree.  Run it in a process of its own: the tools'
`utils` package collides with the one ref_loader.py loads.

Both scripts import plyfile and imageio through utils.io_utils and the first makes a hard-coded
directory at import: empty stand-in modules go into sys.modules, os.makedirs is a no-op during
the import, and the scripts' path globals are re-pointed at the temporary tree.  For `match`,
load_label (frame decoding, out of scope) returns the case's array for the frame it is asked
for, and the pseudo labels are stored as the pickled dict the script reads.

Recorded: the `_bbox.npy` file of every labelling case and the (count, total) of every
assessment case.  Asserted, or the generator fails (conditions on the inputs, evaluated with
the reference's own cs2vv and numpy only):
  per labelling case of LABEL_CASES: at least a quarter of the pool kept and a quarter dropped;
  a box dropped without a vote and one dropped for a mode outside nyu40ids; a tied mode decided
  towards the smaller label; a mode that changes when labels 0..2 vote; a vertex exactly on a
  bound; a float32 vertex with a bound one float64 ulp above it and one below it, where a
  float32 comparison decides differently and the file would differ.  The two SHAPE_CASES exist
  for the (0, 7) and the (1, 7) file and are asserted to give them.
  per assessment case: all 18 classes and ignored pixels in both inputs, the ignored-ignored
  cell non-zero."""
import importlib.util
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import pool_label_cases as PC  # noqa: E402

TOOLS = os.path.join(os.environ.get("OV3D_REFERENCE", "/root/reference"), "3DOVDet_tools")
SCAN = "scene0000_00"


def load_script(rel, name):
    if TOOLS not in sys.path:
        sys.path.insert(0, TOOLS)
    for mod in ("plyfile", "imageio", "imageio.v2"):
        if mod not in sys.modules:
            sys.modules[mod] = types.ModuleType(mod)
    sys.modules["plyfile"].PlyData = sys.modules["plyfile"].PlyElement = None
    sys.modules["imageio.v2"].imread = None
    sys.modules["imageio"].v2 = sys.modules["imageio.v2"]
    spec = importlib.util.spec_from_file_location(name, os.path.join(TOOLS, rel))
    mod = importlib.util.module_from_spec(spec)
    real = os.makedirs
    os.makedirs = lambda *a, **k: None
    try:
        spec.loader.exec_module(mod)
    finally:
        os.makedirs = real
    return mod


def elect(lab, floor):
    """(the smallest most frequent label >= floor, whether the maximum is shared); (None, False)
    without a vote"""
    lab = lab[lab >= floor]
    if len(lab) == 0:
        return None, False
    count = np.bincount(lab)
    return int(count.argmax()), int((count == count.max()).sum()) > 1


def check_label_case(tag, mod, case, saved):
    pts, lab = case["points"], case["labels"]
    vv = mod.cs2vv(np.array(case["pool"], np.float64))
    nyu = set(mod.nyu40ids.tolist())
    seen = dict(no_vote=0, not_nyu=0, tie=0, low=0, bound=0)
    kept, kept32 = [], []
    for b in vv:
        on = (pts >= b[:3]) & (pts <= b[3:6])                           # float64, as the script compares
        mask = on.all(1)
        got, tie = elect(lab[mask], 3)
        seen["no_vote"] += got is None
        seen["not_nyu"] += got is not None and got not in nyu
        seen["tie"] += bool(tie and got in nyu)
        seen["low"] += got is not None and elect(lab[mask], 0)[0] != got
        seen["bound"] += bool((mask[:, None] & ((pts == b[:3]) | (pts == b[3:6]))).any())
        kept.append(got if got in nyu else None)
        b32 = b.astype(np.float32)                                      # what a float32 comparison would do
        got32 = elect(lab[((pts.astype(np.float32) >= b32[:3]) & (pts.astype(np.float32) <= b32[3:6])).all(1)], 3)[0]
        kept32.append(got32 if got32 in nyu else None)
    n_kept, P = sum(k is not None for k in kept), len(vv)
    assert saved.shape == (n_kept, 7) and saved.dtype == np.float64, (tag, saved.shape)
    assert np.array_equal(saved[:, 6], [k for k in kept if k is not None]), tag
    assert 4 * n_kept >= P and 4 * (P - n_kept) >= P, (tag, n_kept, P)
    assert all(v >= 1 for v in seen.values()), (tag, seen)
    # one float64 ulp from a float32 vertex, on each side
    v = np.float64(PC.ULP_X)
    assert (pts[:, 0] == v).any() and np.float32(v) == v
    for bound in PC.ulp_bounds():
        assert abs(bound - v) == np.spacing(v) or abs(bound - v) == np.spacing(bound), tag
        assert np.float32(bound) == PC.ULP_X and ((vv[:, 0] == bound) | (vv[:, 3] == bound)).any(), tag
    differ = [i for i in range(P) if kept[i] != kept32[i]]
    above, below = PC.ulp_bounds()
    assert any(vv[i, 0] == above for i in differ) and any(vv[i, 3] == below for i in differ), (tag, differ)
    return f"kept {n_kept} of {P}, {seen}, {len(differ)} boxes decided differently in float32"


def run_labeling(out):
    mod = load_script(os.path.join("scannet", "assign_box_label_from_gt.py"), "ref_assign_box_label")
    for name in PC.LABEL_CASES + PC.SHAPE_CASES:
        case = PC.label_case(name)
        with tempfile.TemporaryDirectory() as tmp:
            vert_dir, label_dir, pool_dir = PC.write_label_tree(case, tmp, SCAN)
            os.makedirs(os.path.join(tmp, "out"))
            mod.DATASET_ROOT_DIR = vert_dir
            mod.SCANNET_LABEL_PATH = os.path.join(label_dir, "{}_sem_label.npy")
            mod.GSS_PATH = os.path.join(pool_dir, "{}_prop.npy")
            mod.SCANNET_3DBOX_PATH = os.path.join(tmp, "out", "{}_bbox.npy")
            n = mod.labeling(SCAN)
            saved = np.load(os.path.join(tmp, "out", SCAN + "_bbox.npy"))
            assert mod.labeling(SCAN, replace=False) == n == saved.shape[0]
        tag = "label/" + name
        if name in PC.LABEL_CASES:
            print(f"{tag}: {check_label_case(tag, mod, case, saved)}")
        else:
            assert saved.shape == ({"none": 0, "one": 1}[name], 7) and saved.dtype == np.float64, (tag, saved.shape)
            print(f"{tag}: file {saved.shape}")
        out[tag] = saved


def run_match(out):
    mod = load_script(os.path.join("scannet", "assess_pseudo_label.py"), "ref_assess_pseudo_label")
    nyu = mod.PROJECTOR.nyu40ids
    for name in PC.ASSESS_CASES:
        case = PC.assess_case(name)
        by_id = dict(zip(case["frame_ids"], case["gt"]))
        with tempfile.TemporaryDirectory() as tmp:
            os.makedirs(os.path.join(tmp, "frames", SCAN, "color"))
            os.makedirs(os.path.join(tmp, "lseg"))
            for i in case["frame_ids"]:
                open(os.path.join(tmp, "frames", SCAN, "color", f"{i}.jpg"), "w").close()
            np.save(os.path.join(tmp, "lseg", SCAN + ".npy"),
                    {i: p for i, p in zip(case["frame_ids"], case["pseudo"])}, allow_pickle=True)
            mod.SCANNET_FRAMES = os.path.join(tmp, "frames", "{}", "{}")
            mod.SCANNET_FRAME_PATH = os.path.join(mod.SCANNET_FRAMES, "{}")
            mod.PSEUDO_LABEL_PATH = os.path.join(tmp, "lseg", "{}.npy")
            mod.load_label = lambda path: by_id[int(os.path.basename(path).split(".")[0])].copy()
            count, total = mod.match(SCAN)
        tag = "assess/" + name
        gt, ps = case["gt"], case["pseudo"]
        assert all((gt == c).any() for c in nyu) and all((ps == c).any() for c in range(18)), tag
        gt_ignored = ~np.isin(gt, nyu)
        ps_ignored = (ps >= 18) | (ps == -100)
        assert gt_ignored.any() and (ps >= 18).any() and (ps == -100).any() and (gt_ignored & ps_ignored).any(), tag
        assert total == gt.size and 0 < count < total, tag
        out[tag] = np.array([count, total], np.int64)
        print(f"{tag}: count {count} of {total}, {int((gt_ignored & ps_ignored).sum())} pixels ignored by both")


def main():
    out = {}
    run_labeling(out)
    run_match(out)
    path = os.path.join(HERE, "pool_label.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
