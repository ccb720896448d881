"""Times of the single-view pseudo-box lift on one synthetic ScanNet-sized scan (100 frames of
240 x 320, 8 boxes each, a pool of 1 000 proposals), on the GPU:

  lift    ov3d_liftview_frames (both launches) on resident tensors, device events, median and
          spread over repeated runs after a warm-up, for uint16 and for float32 depth
  scan    lift_scannet_scan_single end to end (host plan, uploads, the device chain, the single
          read-back): host clock around calls that end in the read-back
  numpy   the restatement's lift of the same slots (tests/lift_single_ref.py, one core) on this
          machine's host, and whether device and restatement agree byte for byte

  python tools/lift_single_time.py [--out FILE.json] [--reps 30]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")]

import ov3d_import  # noqa: E402

ov3d_import.load()
import lift_cases as LC  # noqa: E402
import lift_single_ref as SR  # noqa: E402
from ov3d_amd import lift_boxes as LB  # noqa: E402

FRAMES, PER_FRAME, P, H, W, CLASSES = 100, 8, 1000, 240, 320, 18


def scan(seed=5):
    """every frame: a 4 x 5 grid of 60 x 64 tiles, each of one class 0..19 (18, 19 ignored) at
    its own depth; 8 boxes naming 6 distinct classes (two labels repeat, as detections do)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    labels = np.empty((FRAMES, H, W), np.int64)
    depths = np.empty((FRAMES, H, W), np.uint16)
    poses, boxes2d = [], []
    for f in range(FRAMES):
        tiles = rng.integers(0, 20, (4, 5))
        labels[f] = np.kron(tiles, np.ones((60, 64), np.int64))
        depths[f] = np.kron(rng.integers(1000, 4000, (4, 5)), np.ones((60, 64), np.int64)) + rng.integers(0, 50, (H, W))
        ang = rng.uniform(0, 2 * np.pi)
        poses.append(LC.look_at([3 * np.cos(ang), 3 * np.sin(ang), 1.2], [0.0, 0.0, 1.0]))
        cls = rng.choice(CLASSES, 6, replace=False)
        cls = np.concatenate([cls, cls[:2]])
        boxes2d.append(np.stack([rng.uniform(1, 100, 8), rng.uniform(1, 100, 8), rng.uniform(10, 200, 8),
                                 rng.uniform(10, 130, 8), rng.uniform(0.05, 1.0, 8), cls.astype(float)], 1))
    pool = np.concatenate([rng.uniform([-6, -6, 0], [6, 6, 2], (P, 3)), rng.uniform(0.3, 2.5, (P, 3)),
                           np.zeros((P, 1))], 1)
    return dict(depths=depths, labels=labels, axis_align_matrix=LC.alignment(), intrinsic=LC.intrinsic(),
                poses=np.stack(poses), boxes2d=boxes2d, gss_pool=pool)


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "runs": len(xs)}


def lift_times(dev, case, reps):
    plan = LB.single_host_plan(case["intrinsic"], case["poses"], case["boxes2d"])
    M, S = len(plan["box_slot"]), len(plan["slot_frame"])
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
    seg = up(case["labels"].astype(np.int32))
    fixed = [up(plan[k]) for k in ("kinv", "pose")] + [up(case["axis_align_matrix"])] + \
        [up(plan[k]) for k in ("slot_frame", "slot_label", "box_slot")]
    rows = torch.zeros(M, 8, dtype=torch.float64, device=dev)
    count = torch.empty(M, dtype=torch.int32, device=dev)
    out = {"boxes": M, "slots": S}
    got = {}
    for kind, depth in (("uint16", up(case["depths"])), ("float32", up(SR.metres(case["depths"])))):
        ms = []
        for it in range(reps + 5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            LB.lift_views(depth, seg, None, LB.PSEUDO_IGNORE_FROM, *fixed, rows, count)
            e1.record()
            e1.synchronize()
            if it >= 5:                                    # the first five warm up
                ms.append(e0.elapsed_time(e1))
        out["lift_ms_" + kind] = spread(ms)
        got[kind] = (rows[:, :6].cpu().numpy(), count.cpu().numpy())
    out["lifted"] = int((got["uint16"][1] > 0).sum())
    t0 = time.perf_counter()
    lohi, n = SR.lift_slots(SR.metres(case["depths"]), SR.classes(case["labels"], ignore_from=SR.IGNORE_FROM),
                            plan["kinv"], plan["pose"], case["axis_align_matrix"], plan["slot_frame"],
                            plan["slot_label"])
    out["numpy_lift_ms"] = (time.perf_counter() - t0) * 1e3
    bs = plan["box_slot"]
    out["same_bytes_as_numpy"] = all(r.tobytes() == lohi[bs].tobytes() and np.array_equal(c, n[bs])
                                     for r, c in got.values())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=30)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs the GPU: a time taken anywhere else says nothing")
    dev = torch.device("cuda", 0)
    case = scan()
    res = {"shape": {"frames": FRAMES, "H": H, "W": W, "boxes_per_frame": PER_FRAME, "P": P},
           "device": torch.cuda.get_device_name(0)}
    for _ in range(3):
        final = LB.lift_scannet_scan_single(**case, device=dev)
    ts = []
    for _ in range(args.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        final = LB.lift_scannet_scan_single(**case, device=dev)
        ts.append((time.perf_counter() - t0) * 1e3)
    res["scan_ms"], res["rows_out"] = spread(ts), int(final.shape[0])
    res.update(lift_times(dev, case, args.reps))
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    if not res["same_bytes_as_numpy"]:
        raise SystemExit("device and restatement disagree")


if __name__ == "__main__":
    main()
