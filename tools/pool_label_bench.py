"""Times of the pool labelling and the pseudo-label assessment on one ScanNet-sized synthetic
scan (50 000 float32 vertices, a pool of 1 000 and of 4 000 boxes, 100 frames of 240 x 320
labels), on the GPU:

  scan       label_pool end to end (validation, cs2vv, uploads, the launch, the read-back of the
             modes, filter and vv2cs): host clock around calls that end in the read-back,
             median and spread after a warm-up; against the numpy restatement
             (tests/pool_label_ref.py: one numpy pass over all vertices per box, one core) on
             this machine's host, and whether the two arrays are the same bytes
  vote       the vote kernel alone on resident tensors against the existing box_label_votes
             (ov3d_box_points_count kind 1) at a shape both accept: float32 vertices, 32 bins,
             float32-exact bounds.  Device events around `--inner` back-to-back launches,
             `--rounds` rounds, the two kernels alternating; per-launch median / min / max, and
             whether the counts are the same
  confusion  the confusion entry (its clear and its kernel) on resident tensors, the same way:
             the 100 frames of one scan (15 MB: served from cache after the first launch) and a
             group of 8 scans of 500 frames (614 MB, more than the Infinity Cache: a stream
             from HBM); the achieved bytes per second count the two bytes per pixel the
             algorithm reads

  python tools/pool_label_bench.py [--out FILE.json] [--lib LIBRARY.so]

--lib times a library built with another OV3D_POOLLABEL_TILE / OV3D_POOLLABEL_CULL.
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
import pool_label_ref as R  # noqa: E402
from ov3d_amd import _native, label_assess as LA, label_formatter as LF, pool_label as PL  # noqa: E402

N, H, W, FRAMES = 50000, 240, 320, 100
HBM_PEAK, HBM_COPY = 8.0e12, 6.29e12          # MI355X_MICROARCH.md: spec, measured float4 copy
OBJECT_IDS = np.array([3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14, 16, 24, 28, 33, 34, 36, 39, 13, 21, 40])


def scan(P, seed=5):
    """21 labelled blobs on a 7 x 3 grid (70 % of the vertices: the 18 detection classes and
    three other nyu40 ids) in a room of wall and floor (labels 1 and 2); the pool holds random
    boxes of 0.2 .. 1.5 m.  Everything is a multiple of 1/64: exact in float32."""
    rng = np.random.Generator(np.random.PCG64(seed))
    centres = np.array([[(c % 7) * 1.5 - 4.5, (c // 7) * 1.8 - 1.8, 0.7] for c in range(len(OBJECT_IDS))])
    obj = rng.integers(0, len(OBJECT_IDS), N)
    pts = centres[obj] + rng.uniform(-0.4, 0.4, (N, 3))
    lab = OBJECT_IDS[obj]
    back = rng.random(N) < 0.3
    pts[back] = rng.uniform([-6, -3.5, 0], [6, 3.5, 2.5], (int(back.sum()), 3))
    lab[back] = rng.choice([1, 2], int(back.sum()))
    grid = lambda a: np.round(a * 64) / 64                                           # noqa: E731
    pool = np.concatenate([grid(rng.uniform([-6, -3.5, 0], [6, 3.5, 2.5], (P, 3))),
                           grid(rng.uniform(0.2, 1.5, (P, 3))), np.zeros((P, 1))], 1)
    return dict(points=grid(pts).astype(np.float32), sem_labels=lab.astype(np.int64), pool=pool)


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "runs": len(xs)}


def per_launch_ms(fns, inner, rounds):
    """{name: per-launch times}: device events around `inner` back-to-back launches of each
    function in turn, `rounds` rounds after two warm-up rounds"""
    ms = {n: [] for n in fns}
    for it in range(rounds + 2):
        for name, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                fn()
            e1.record()
            e1.synchronize()
            if it >= 2:
                ms[name].append(e0.elapsed_time(e1) / inner)
    return {n: spread(v) for n, v in ms.items()}


def end_to_end(dev, P, reps):
    case = scan(P)
    for _ in range(2):
        got = PL.label_pool(**case, device=dev)
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = PL.label_pool(**case, device=dev)
        ts.append((time.perf_counter() - t0) * 1e3)
    t0 = time.perf_counter()
    scan_ = PL._scan(case["points"], case["sem_labels"], case["pool"], "bench")
    want = PL._finish(scan_[2], R.vote_group([scan_])[0])
    numpy_ms = (time.perf_counter() - t0) * 1e3
    return {"P": P, "scan_ms": spread(ts), "numpy_ms": numpy_ms, "rows_out": int(got.shape[0]),
            "same_bytes_as_numpy": bool(got.shape == want.shape and got.tobytes() == want.tobytes()),
            "speedup_vs_numpy": numpy_ms / statistics.median(ts)}


def vote_alone(dev, P, inner, rounds):
    case = scan(P)
    pts, lab, boxes = PL._scan(case["points"], np.minimum(case["sem_labels"], 31), case["pool"], "bench")
    assert np.array_equal(boxes[:, :6], boxes[:, :6].astype(np.float32))             # float32-exact bounds
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)                 # noqa: E731
    t_pts, t_lab, t_box = up(pts), up(lab), up(boxes[:, :6])
    pt_off, box_off = up(np.array([0, N], np.int32)), up(np.array([0, P], np.int32))
    lo32, hi32 = (up(boxes[None, :, c:c + 3].astype(np.float32)) for c in (0, 3))
    new = lambda: PL.vote(t_pts, t_lab, pt_off, t_box, box_off, 0, 32)               # noqa: E731
    old = lambda: LF.box_label_votes(t_pts[None], t_lab[None], lo32, hi32, 32)       # noqa: E731
    same = bool(torch.equal(new()[0], old()[0][0]) and torch.equal(new()[1], old()[1][0]))
    res = per_launch_ms({"poollabel_vote": new, "box_label_votes": old}, inner, rounds)
    return {"P": P, "C": 32, "same_counts_and_modes": same, "ms": res,
            "ratio_new_over_old": res["poollabel_vote"]["median"] / res["box_label_votes"]["median"]}


def confusion_alone(dev, scans, frames, inner, rounds):
    """runs of 8 equal labels, made on the device"""
    F = scans * frames
    g = torch.Generator(device=dev).manual_seed(F)
    runs = lambda hi: torch.randint(0, hi, (F * H * W // 8,), device=dev, generator=g,      # noqa: E731
                                    dtype=torch.uint8).repeat_interleave(8).view(F, H * W)
    gt, pseudo = runs(41), runs(20)
    off = torch.arange(0, F + 1, frames, dtype=torch.int32, device=dev)
    gt_map = torch.from_numpy(LA.GT_MAP).to(dev)
    conf = LA.confusion(gt, pseudo, off, gt_map)
    total = int(conf.sum())
    res = per_launch_ms({"confusion": lambda: LA.confusion(gt, pseudo, off, gt_map)}, inner, rounds)["confusion"]
    nbytes = 2 * F * H * W
    rate = nbytes / (res["median"] * 1e-3)
    return {"scans": scans, "frames_per_scan": frames, "bytes_read": nbytes, "pixels_counted": total,
            "all_pixels_counted": total == F * H * W, "ms": res, "bytes_per_s": rate,
            "share_of_hbm_peak": rate / HBM_PEAK, "share_of_measured_copy": rate / HBM_COPY}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--skip-numpy", action="store_true", help="vote and confusion only")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs the GPU: a time taken anywhere else says nothing")
    if args.lib:
        _native.LIB_PATH = os.path.abspath(args.lib)
    dev = torch.device("cuda", 0)
    res = {"shape": {"N": N, "frames": FRAMES, "H": H, "W": W}, "device": torch.cuda.get_device_name(0),
           "lib": os.path.relpath(_native.LIB_PATH, ROOT), "inner": args.inner, "rounds": args.rounds}
    res["vote"] = [vote_alone(dev, P, args.inner, args.rounds) for P in (1000, 4000)]
    res["confusion"] = [confusion_alone(dev, 1, FRAMES, args.inner, args.rounds),
                        confusion_alone(dev, 8, 500, max(args.inner // 2, 2), args.rounds)]
    if not args.skip_numpy:
        res["label_pool"] = [end_to_end(dev, P, args.reps) for P in (1000, 4000)]
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    if not all(v["same_counts_and_modes"] for v in res["vote"]) or \
            not all(c["all_pixels_counted"] for c in res["confusion"]) or \
            not all(e["same_bytes_as_numpy"] for e in res.get("label_pool", [])):
        raise SystemExit("a result differs from its yardstick")


if __name__ == "__main__":
    main()
