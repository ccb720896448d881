"""Writes tests/golden/lift_single.npz: the REFERENCE's own `lifting`
(3DOVDet_tools/scannet/lift_boxes.py, loaded by file path, unchanged) with VIEW = 'single', run
end to end over lift_single_cases.py on a temporary file tree.  Run it in a process of its own
(see make_lift_golden.py, whose loader and probes it uses).

The script's path globals are re-pointed at the temporary tree; the stand-in imageio's imread
decodes the depth and label PNGs through PIL, so the script's own load_depth and load_label
run.  PSEUDO_FLAG is set per case.

Recorded per case: the lifted boxes before the first NMS and the file written.  Asserted per
case, or the generator fails: the margins of make_lift_golden.py's Probe.check (every overlap
of both NMS passes and every iou.max() of the match at least 1e-9 from its threshold, best and
second-best IoU at least 1e-9 apart, distinct scores, size-NMS intersections 0 or at least
1e-9); and in "main" and "gt_labels" that the edge filter, both NMS passes and the match each
decide something, that two boxes of one (frame, label) lifted identical rows, that the box
labelled -100 and a class holding depth 0 were lifted and that one box found no pixel."""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import lift_single_cases as SC  # noqa: E402
import make_lift_golden as G  # noqa: E402


def run(out):
    from PIL import Image
    mod = G.load_script(os.path.join("scannet", "lift_boxes.py"), "ref_scannet_lift_single")
    sys.modules["utils.io_utils"].imread = lambda path: np.array(Image.open(path))
    proj = mod.PROJECTOR
    edge = proj.get_edge_mask
    state = {}

    def edge_probe(box):
        kept = edge(box)
        state["edge"] += len(box) - len(kept)
        return kept
    proj.get_edge_mask = edge_probe
    mod.VIEW = "single"
    assert mod.USE_GSS is True and tuple(proj.image_dims) == (SC.H, SC.W)
    for name in SC.CASES:
        case, scan = SC.case(name), "scene0000_00"
        with tempfile.TemporaryDirectory() as tmp:
            SC.write_tree(case, tmp, scan)
            os.makedirs(os.path.join(tmp, "det"))
            np.save(os.path.join(tmp, "det", scan + "_vert.npy"), np.zeros((1, 6), np.float32))
            mod.DATASET_ROOT_DIR = os.path.join(tmp, "det")
            mod.SCANNET_LABEL_PATH = os.path.join(tmp, "lseg", "{}.npy")
            mod.SCANNET_FRAMES = os.path.join(tmp, "frames", "{}", "{}")
            mod.SCANNET_FRAME_PATH = os.path.join(mod.SCANNET_FRAMES, "{}")
            mod.SCANNET_META_PATH = os.path.join(tmp, "scans", "{}", "{}.txt")
            mod.SCANNET_2DBOX_PATH = os.path.join(tmp, "boxes2d", "{}", "{}")
            mod.SCANNET_3DBOXS = os.path.join(tmp, "out")
            mod.SCANNET_3DBOX_PATH = os.path.join(tmp, "out", "{}_bbox.npy")
            mod.GSS_PATH = os.path.join(tmp, "gss", "{}_prop.npy")
            mod.PSEUDO_FLAG = bool(case["pseudo"])
            state.update(edge=0)
            probe = G.Probe(mod)
            mod.lifting(scan)
            final = np.load(os.path.join(tmp, "out", scan + "_bbox.npy"))
        tag = "single/" + name
        full = name in ("main", "gt_labels")
        report = probe.check(tag, mod.MATCH_THRESH, full)
        lifted = probe.lifted()
        if full:
            boxes = sum(len(b) for b in case["boxes2d"])
            assert state["edge"] == 2 and len(final) >= 2, tag
            assert len(lifted) == boxes - state["edge"] - 1, (tag, "exactly one box finds no pixel")
            twins = [(i, j) for i in range(len(lifted)) for j in range(i) if
                     lifted[i, :6].tobytes() == lifted[j, :6].tobytes()]
            assert len(twins) == 1 and lifted[twins[0][0], 7] == lifted[twins[0][1], 7] == 2.0, (tag, twins)
            assert (lifted[:, 7] == -100.0).sum() == 1, tag
            f, vs, us = SC.ZERO_DEPTH
            assert (case["depths"][f, vs, us] == 0).all() and len(np.unique(case["labels"][f, vs, us])) == 1
            ignored = case["labels"] >= 18 if case["pseudo"] else ~np.isin(case["labels"], SC.NYU40)
            assert ignored.any(), tag
        elif name == "nothing_lifted":
            assert final.shape == (0, 7) and len(lifted) == 0, tag
        else:
            assert final.shape == (0, 10) and len(lifted) > 0, tag
        out[tag + "/lifted"], out[tag + "/final"] = lifted, final
        print(f"{tag}: edge filter removed {state['edge']}, lifted {lifted.shape}, {report}, file {final.shape}")


def main():
    out = {}
    run(out)
    path = os.path.join(HERE, "lift_single.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
