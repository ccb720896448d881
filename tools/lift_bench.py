"""Times of pseudo-box lifting on one ScanNet-sized synthetic scan (50 000 vertices, 100 frames
of 8 boxes, a pool of 1 000 proposals), on the GPU:

  scan    lift_scannet_scan end to end (host planes, uploads, the device chain, the single
          read-back, compaction): host clock around calls that end in the read-back, median
          and spread over repeated runs after a warm-up
  host    the host part alone (edge filter, planes of all 800 boxes, the matrix inverse)
  stages  the device chain on resident tensors, device events around each stage (lift, first
          NMS, match, size NMS) and around the whole chain, median / min / max
  numpy   the restatement of the same scan (tests/lift_ref.py: one numpy pass over all
          vertices per 2D box, one core) on this machine's host, and whether the two arrays
          are the same bytes

  python tools/lift_bench.py [--out FILE.json] [--reps 20]
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
import lift_ref as R  # noqa: E402
from ov3d_amd import lift_boxes as LB  # noqa: E402

N, FRAMES, PER_FRAME, P, CLASSES = 50000, 100, 8, 1000, 18


def scan(seed=3):
    """18 labelled blobs on a 6 x 3 grid (70 % of the vertices) in a room of ignored background;
    every frame looks at one blob from 2.5 m and carries boxes around 8 blobs' projections
    (those behind the camera or off the frame give degenerate or empty frusta, as real
    detections do); the pool holds a grown box per blob among random ones"""
    rng = np.random.Generator(np.random.PCG64(seed))
    A = LC.alignment()
    centres = np.array([[(c % 6) * 1.5 - 3.75, (c // 6) * 1.8 - 1.8, 0.7] for c in range(CLASSES)])
    cls = rng.integers(0, CLASSES, N)
    orig = centres[cls] + rng.uniform(-0.3, 0.3, (N, 3))
    lab = cls.astype(np.float64)
    back = rng.random(N) < 0.3
    orig[back] = rng.uniform([-5, -3.5, 0], [5, 3.5, 2.5], (int(back.sum()), 3))
    lab[back] = rng.choice([18.0, 19.0, 39.0], int(back.sum()))
    aligned = (orig @ A[:3, :3].T + A[:3, 3]).astype(np.float32).astype(np.float64)
    poses, boxes2d = [], []
    for f in range(FRAMES):
        target = f % CLASSES
        ang = rng.uniform(0, 2 * np.pi)
        eye = centres[target] + [2.5 * np.cos(ang), 2.5 * np.sin(ang), rng.uniform(0.2, 0.8)]
        pose = LC.look_at(eye, centres[target])
        rows = []
        for b in [target] + list(rng.choice(CLASSES, PER_FRAME - 1, replace=False)):
            pts = orig[(cls == b) & ~back][:200]
            cam = (pts - pose[:3, 3].astype(float)) @ pose[:3, :3].astype(float)
            if (cam[:, 2] < 0.3).any():                    # behind the camera: a small box in the corner
                box = [5.5 + b, 7.5, 20.0, 15.0]
            else:
                box = LC.box_around(pose, pts, 3)
                box[0], box[1] = max(box[0], 0.5), max(box[1], 0.5)
                box[2], box[3] = min(box[2], 318.0 - box[0]), min(box[3], 238.0 - box[1])
            rows.append(box + [rng.uniform(0.05, 1.0), float(b)])
        poses.append(pose)
        boxes2d.append(np.array(rows))
    pool = [LC.pool_box(aligned[(cls == b) & ~back], rng.uniform(0.0, 0.15, 3)) for b in range(CLASSES)]
    while len(pool) < P:
        pool.append(np.concatenate([rng.uniform([-5, -4, 0], [6, 4, 2]), rng.uniform(0.2, 1.5, 3), [0.0]]))
    pool = np.array(pool)[rng.permutation(P)]
    return dict(points=aligned, labels=lab, axis_align_matrix=A, intrinsic=LC.intrinsic(),
                poses=np.stack(poses), boxes2d=boxes2d, gss_pool=pool)


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "runs": len(xs)}


def stage_times(dev, case, reps):
    planes, sl, plabel = LB.scannet_host_plan(case["intrinsic"], case["poses"], case["boxes2d"])
    M = len(planes)
    A = case["axis_align_matrix"]
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
    rows_h = np.zeros((M, 8))
    rows_h[:, 6:] = sl
    pts, lab = up(case["points"]), up(LB._int_labels(R.scannet_labels(case["labels"]), LB._NEVER_POINT))
    Ad, Ai, pl, pb, rows, pool = up(A), up(np.linalg.inv(A)), up(planes), up(plabel), up(rows_h), up(case["gss_pool"])
    packed, out, count, rank2 = LB.result_buffer(M, dev)
    names = ("lift", "nms", "match", "size_nms", "chain")
    ms = {n: [] for n in names}
    for it in range(reps + 3):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
        ev[0].record()
        LB.lift_frusta(pts, lab, Ad, Ai, pl, pb, rows, count)
        ev[1].record()
        rank1, _ = LB.nms_boxes(rows, 0.7, valid=count)
        ev[2].record()
        m = LB.match_pool(rows, rank1, pool, 0.3, out=out)
        ev[3].record()
        LB.nms_boxes(m["rows"], 0.0, valid=m["win"], use_size_score=True, rank=rank2)
        ev[4].record()
        ev[4].synchronize()
        if it >= 3:                                        # the first three warm up
            for i, n in enumerate(names[:4]):
                ms[n].append(ev[i].elapsed_time(ev[i + 1]))
            ms["chain"].append(ev[0].elapsed_time(ev[4]))
    return {"boxes": M, "lifted": int((count > 0).sum()), "first_nms_kept": int((rank1 >= 0).sum()),
            "pool_labelled": int(m["win"].sum()), "ms": {n: spread(v) for n, v in ms.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs the GPU: a time taken anywhere else says nothing")
    dev = torch.device("cuda", 0)
    case = scan()
    res = {"shape": {"N": N, "frames": FRAMES, "boxes_per_frame": PER_FRAME, "P": P},
           "device": torch.cuda.get_device_name(0)}
    for _ in range(2):
        final = LB.lift_scannet_scan(**case, device=dev)
    ts, th = [], []
    for _ in range(args.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        final = LB.lift_scannet_scan(**case, device=dev)
        ts.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        LB.scannet_host_plan(case["intrinsic"], case["poses"], case["boxes2d"])
        th.append((time.perf_counter() - t0) * 1e3)
    res["scan_ms"], res["host_plan_ms"] = spread(ts), spread(th)
    res["stages"] = stage_times(dev, case, args.reps)
    tn = []
    for _ in range(2):
        t0 = time.perf_counter()
        want, _ = R.scannet_scan(**case)
        tn.append((time.perf_counter() - t0) * 1e3)
    res["numpy_ms"] = spread(tn)
    res["rows_out"] = int(final.shape[0])
    res["same_bytes_as_numpy"] = bool(final.shape == want.shape and final.tobytes() == want.tobytes())
    res["speedup_vs_numpy"] = res["numpy_ms"]["median"] / res["scan_ms"]["median"]
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    if res["scan_ms"]["median"] > res["numpy_ms"]["median"]:
        raise SystemExit("the device chain is slower than the numpy restatement on this scan")


if __name__ == "__main__":
    main()
