"""Writes tests/golden/lift_boxes.npz: the REFERENCE's own `lifting` functions
(3DOVDet_tools/scannet/lift_boxes.py and sunrgbd/lift_boxes.py, loaded by file path, unchanged)
run end to end over lift_cases.py on a temporary file tree.  Run it in a process of its own:
the tools' `utils` package collides with the one ref_loader.py loads.

The ScanNet script imports plyfile and imageio and makes a hard-coded directory at import:
empty stand-in modules go into sys.modules, os.makedirs is a no-op during the import, the
script's path globals are re-pointed at the temporary tree and load_depth (unused in the
multi-view mode) is a stub.

Recorded per case: the lifted boxes before the first NMS (the script's nms_3d_faster wrapped)
and the file written.  Asserted per case, or the generator fails: every frustum test, every
overlap of both NMS passes and every iou.max() of the match is at least 1e-9 from its
threshold; an intersection of the size NMS is 0 or at least 1e-9; best and second-best IoU of
a match differ by at least 1e-9; scores entering an argsort are distinct; and in the "main"
cases the edge filter, the first NMS, the match (both ways) and the size NMS each decide
something.

The SUN RGB-D script as published fails on the first image that lifts a box (its cat_box
flattens the rows); the generator keeps the rows as rows (see run_sun) and changes nothing else."""
import argparse
import importlib.util
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import lift_cases as LC  # noqa: E402

TOOLS = os.path.join(os.environ.get("OV3D_REFERENCE", "/root/reference"), "3DOVDet_tools")
MARGIN = 1e-9


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


class Probe:
    """wraps the script's nms_3d_faster and box_3d_iou; keeps what the margins need"""

    def __init__(self, mod):
        self.nms_in, self.nms_out, self.ious = [], [], []
        if not hasattr(mod, "_own"):
            mod._own = (mod.nms_3d_faster, mod.box_3d_iou)
        nms, iou = mod._own

        def nms_probe(boxes, thresh, **kw):
            self.nms_in.append((np.array(boxes), thresh, kw))
            out = nms(boxes, thresh, **kw)
            self.nms_out.append(np.array(out))
            return out

        def iou_probe(q, k, **kw):
            out = iou(q, k, **kw)
            self.ious.append(np.array(out))
            return out
        mod.nms_3d_faster, mod.box_3d_iou = nms_probe, iou_probe

    def check(self, tag, match, main):
        for n, (boxes, thresh, kw) in enumerate(self.nms_in):
            size_pass = bool(kw.get("use_size_score"))
            score = boxes[:, 6] * boxes[:, 8] if size_pass else boxes[:, 6]
            assert len(np.unique(score)) == len(score), (tag, "equal scores in NMS pass", n)
            vol = np.prod(boxes[:, 3:6] - boxes[:, :3], -1) + 1e-8
            for i in range(len(boxes)):
                side = np.maximum(0, np.minimum(boxes[i, 3:6], boxes[:, 3:6]) - np.maximum(boxes[i, :3], boxes[:, :3]))
                inter = np.prod(side, -1)
                o = inter / (vol[i] + vol - inter) * (boxes[i, 7] == boxes[:, 7])
                o[i] = 1.0
                # an overlap that is exactly 0 (no intersection, or another class) decides exactly
                assert ((np.abs(o - thresh) >= MARGIN) | (o == 0)).all(), (tag, "overlap at the threshold", n, i)
                if size_pass:
                    assert ((inter == 0) | (inter >= MARGIN)).all(), (tag, "tiny intersection", n, i)
        unmatched = 0
        for iou in self.ious:
            top = np.sort(iou)[::-1]
            assert abs(top[0] - match) >= MARGIN, (tag, "iou.max() at the threshold")
            if top[0] < match:
                unmatched += 1
            elif len(top) > 1:
                assert top[0] - top[1] >= MARGIN, (tag, "argmax tie")
        if main:
            assert len(self.nms_in) == 2, (tag, "the chain stopped early")
            assert len(self.nms_out[0]) < len(self.nms_in[0][0]), (tag, "first NMS suppressed nothing")
            assert unmatched >= 1, (tag, "every lifted box matched")
            assert len(self.nms_in[1][0]) >= 2, (tag, "fewer than two pool boxes labelled")
            assert len(self.nms_out[1]) < len(self.nms_in[1][0]), (tag, "size NMS suppressed nothing")
        return (f"NMS {[(len(i[0]), len(o)) for i, o in zip(self.nms_in, self.nms_out)]}, "
                f"{len(self.ious)} matched against the pool, {unmatched} below the threshold")

    def lifted(self, width=8):
        return self.nms_in[0][0] if self.nms_in else np.zeros((0, width))


def run_scannet(out):
    mod = load_script(os.path.join("scannet", "lift_boxes.py"), "ref_scannet_lift")
    mod.load_depth = lambda path: None
    proj = mod.PROJECTOR
    in_frustum, edge = proj.points_in_frustum, proj.get_edge_mask
    state = {}

    def frustum_probe(corners, normals, pts, return_mask=False):
        with np.errstate(all="ignore"):
            for c, ns in ((corners[2][:3].reshape(-1), normals[:3]), (corners[4][:3].reshape(-1), normals[3:])):
                a = pts - c
                a = a / np.sum(a ** 2, -1, keepdims=True)
                for nrm in ns:
                    rel = np.abs(a @ nrm) / (np.linalg.norm(a, axis=-1) * np.linalg.norm(nrm))
                    if np.isfinite(rel).any():
                        state["margin"] = min(state["margin"], np.nanmin(rel))
        return in_frustum(corners, normals, pts, return_mask=return_mask)

    def edge_probe(box):
        kept = edge(box)
        state["edge"] += len(box) - len(kept)
        return kept
    proj.points_in_frustum, proj.get_edge_mask = frustum_probe, edge_probe
    for name in LC.SCANNET_CASES:
        case, scan = LC.scannet_case(name), "scene0000_00"
        with tempfile.TemporaryDirectory() as tmp:
            LC.write_scannet_tree(case, tmp, scan)
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
            assert (mod.VIEW, mod.PSEUDO_FLAG, mod.USE_GSS) == ("multi", True, True)
            state.update(margin=np.inf, edge=0)
            probe = Probe(mod)
            with np.errstate(all="ignore"):
                mod.lifting(scan)
            final = np.load(os.path.join(tmp, "out", scan + "_bbox.npy"))
        tag = "scannet/" + name
        assert state["margin"] >= MARGIN, (tag, "a point within the margin of a plane", state["margin"])
        report = probe.check(tag, mod.MATCH_THRESH, name == "main")
        if name == "main":
            assert state["edge"] >= 1 and len(final) >= 1, tag
        else:
            assert len(final) == 0, tag
        out[tag + "/lifted"], out[tag + "/final"] = probe.lifted(), final
        print(f"{tag}: edge filter removed {state['edge']}, plane margin {state['margin']:.2e}, {report}, "
              f"file {final.shape}")


def run_sun(out):
    from PIL import Image
    mod = load_script(os.path.join("sunrgbd", "lift_boxes.py"), "ref_sun_lift")
    const = mod.const_sunrgbd
    edge = mod.get_edge_mask
    state = {}

    def edge_probe(box, dims):
        kept = edge(box, dims)
        state["edge"] = len(box) - len(kept)
        return kept
    mod.get_edge_mask = edge_probe
    # The script's compute_box collects one (8,) row per 2D box and its cat_box concatenates
    # them into one flat vector, which nms_3d_faster cannot index: as published, `lifting` only
    # gets through an image that lifts nothing.  The rows are kept as rows here, the only change.
    cat = mod.cat_box
    mod.cat_box = lambda rows, l=8: np.reshape(cat(rows, l), (-1, l))
    for name in LC.SUN_CASES:
        case, scan = LC.sun_case(name), "000001"
        with tempfile.TemporaryDirectory() as tmp:
            for d in ("lseg", "calib", "depth", os.path.join("boxes", "2D"), os.path.join("boxes", "3D"),
                      os.path.join("gss", "gss_prop")):
                os.makedirs(os.path.join(tmp, d))
            np.save(os.path.join(tmp, "lseg", scan + ".npy"), case["seg"] - 1)
            with open(os.path.join(tmp, "calib", scan + ".txt"), "w") as f:
                for m in (case["Rtilt"], case["K"]):
                    f.write(" ".join(repr(float(x)) for x in m.reshape(-1, order="F")) + "\n")
            Image.fromarray(case["depth"]).save(os.path.join(tmp, "depth", scan + ".png"))
            assert np.array_equal(np.array(Image.open(os.path.join(tmp, "depth", scan + ".png"))), case["depth"])
            np.save(os.path.join(tmp, "boxes", "2D", scan + ".npy"), case["boxes2d"])
            np.save(os.path.join(tmp, "gss", "gss_prop", scan + "_prop.npy"), case["gss_pool"])
            mod.PSEUDO_LABEL_PATH = os.path.join(tmp, "lseg", "{}.npy")
            mod.CALIB_PATH = os.path.join(tmp, "calib", "{}.txt")
            mod.DEPTH_PATH = os.path.join(tmp, "depth", "{}.png")
            const.box_root, const.gss_root = os.path.join(tmp, "boxes"), os.path.join(tmp, "gss")
            opts = argparse.Namespace(input="2D", output="3D", use_gt=False, thresh_nms=0.7,
                                      thresh_size=0, thresh_match=0.3)
            probe = Probe(mod)
            mod.lifting(scan, debug=True, opts=opts)
            final = np.load(os.path.join(tmp, "boxes", "3D", scan + "_bbox.npy"))
        tag = "sun/" + name
        b = case["boxes2d"]
        for e in np.concatenate([b[:, 0], b[:, 1], b[:, 0] + b[:, 2], b[:, 1] + b[:, 3]]):
            assert e == np.round(e) or abs(e - np.round(e)) >= MARGIN, (tag, "edge near a pixel", e)
        report = probe.check(tag, 0.3, name == "main")
        if name == "main":
            assert state["edge"] >= 1 and len(final) >= 1, tag
            assert ((b[:, :4] == np.round(b[:, :4])).all(1) & (b[:, 0] != 0)).any(), (tag, "no box on the pixel grid")
        else:
            assert len(final) == 0, tag
        out[tag + "/lifted"], out[tag + "/final"] = probe.lifted(), final
        print(f"{tag}: edge filter removed {state['edge']}, {report}, file {final.shape}")


def main():
    out = {}
    run_scannet(out)
    run_sun(out)
    path = os.path.join(HERE, "lift_boxes.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
