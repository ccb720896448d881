"""Times of the pseudo-box evaluation at the shape of ScanNet's training split (1201 scans x 64
pseudo boxes x 16 GT boxes, 18 classes, thresholds 0.25 and 0.5), on the GPU:

  launches  ov3d_boxeval_match + ov3d_boxeval_tally on resident inputs: device events around
            the pair, 20 times after a warm-up: median, min, max; then events around each
            entry of 20 more pairs, the median; the results are checked against the numpy
            restatement
  metrics   PRCalculator.compute_metrics() end to end (packing on the host, uploads, the two
            launches, the read-back, the dict), host clock
  numpy     the restatement (tests/box_eval_ref.py, one vectorised pass per scan, one core) on
            the same data on this host

  python tools/box_eval_time.py [--out FILE.json]
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
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import ov3d_import  # noqa: E402

ov3d_import.load()
import box_eval_ref as R  # noqa: E402
from ov3d_amd import _native as nat, box_eval as BE  # noqa: E402

S, K, G, C = 1201, 64, 16, 18
THR = [0.25, 0.5]


def split(rng):
    """per scan G boxes in a room and K predictions that are jittered copies of them"""
    scans = []
    for _ in range(S):
        gc = rng.uniform([-4, -4, 0], [4, 4, 2], (G, 3))
        gs = rng.uniform(0.3, 1.5, (G, 3))
        gl = rng.integers(0, C, G)
        src = rng.integers(0, G, K)
        pc = gc[src] + rng.normal(0, 0.15, (K, 3))
        ps = gs[src] * rng.uniform(0.7, 1.4, (K, 3))
        pl = np.where(rng.random(K) < 0.8, gl[src], rng.integers(0, C, K))
        scans.append((np.concatenate([pc, ps, pl[:, None]], 1), np.concatenate([gc, gs], 1), gl))
    return scans


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs the GPU: a time taken anywhere else says nothing")
    torch.set_num_threads(1)
    dev = torch.device("cuda", 0)
    scans = split(np.random.Generator(np.random.PCG64(5)))
    calc = BE.PRCalculator(THR, device=dev)
    for pred, gt, gl in scans:
        calc.step_arrays(pred, gt, gl)
    pack, c = calc._pack()
    assert c == C
    t = [torch.from_numpy(np.ascontiguousarray(pack[k])).to(dev)
         for k in ("pred", "pred_cls", "score", "pred_off", "gt", "gt_cls", "gt_off")]
    t.append(torch.tensor(THR, dtype=torch.float64, device=dev))
    for _ in range(5):
        r = BE.launch(*t, C)
    ms = []
    for _ in range(20):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = BE.launch(*t, C)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    entries = ("ov3d_boxeval_match", "ov3d_boxeval_tally")
    nat.timing_enable(entries)                             # events around each entry of 20 more pairs
    for _ in range(20):
        BE.launch(*t, C)
    each = {n: statistics.median(x["ms"] for x in recs) for n, recs in nat.timing_collect().items()}
    t0 = time.perf_counter()
    want = R.run(pack, THR, C, flags=True)
    t_ref = time.perf_counter() - t0
    for k in ("nd", "npos", "ntp", "tp", "ovmax"):
        got = r[k].cpu().numpy()
        assert got.dtype == want[k].dtype and np.array_equal(got, want[k]), k
    calc.compute_metrics()                                 # warm-up
    ts = []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        metrics = calc.compute_metrics()
        ts.append(time.perf_counter() - t0)
    res = {"shape": {"scans": S, "predictions_per_scan": K, "gt_per_scan": G, "classes": C, "thresholds": THR},
           "device": torch.cuda.get_device_name(0),
           "launches_ms": {"median": statistics.median(ms), "min": min(ms), "max": max(ms), "repeats": len(ms)},
           "entry_ms_median": each, "pairs": S * K * G, "input_bytes": int(sum(x.nbytes for x in t)),
           "compute_metrics_s": {"median": statistics.median(ts), "all": ts},
           "numpy_restatement_s": t_ref,
           "mPrecision": {str(k): float(v["mPrecision"]) for k, v in metrics.items()},
           "AR": {str(k): float(v["AR"]) for k, v in metrics.items()}}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
