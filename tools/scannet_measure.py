"""Measure the ScanNet device loader on the GPU (numbers of DESIGN.md "ScanNet batches on the
device").  Needs a ROCm device; there is no CPU path.

    python tools/scannet_measure.py [--iters 50]

Prints one JSON line:
  get_batch at B=8, 50000 -> 40000 with colour and augmentation: host time of the random plan,
  device time per kernel (HIP events around each single launch, so the launch latency of an
  idle queue is inside the figure), wall time per batch;
  ov3d_rows_gather at 8 x 40000 rows of fp16 D=512 against torch.index_select on the same
  tensors, alternating, with bytes read + written over time as a share of the 8 TB/s HBM peak.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ov3d_import  # noqa: E402

ov3d_import.load()
from ov3d_amd import _native as nat, scannet  # noqa: E402
from ov3d_amd.dataset_config import ScannetDatasetConfig  # noqa: E402

HBM_PEAK = 8.0e12
REPS = 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no ROCm device: nothing to measure")
    cfg = ScannetDatasetConfig()
    g = np.random.Generator(np.random.PCG64(1))
    ids = np.asarray(cfg.nyu40ids, np.float64)
    scans = []
    for i in range(8):
        n, k = 50000, 8 + i
        vert = np.concatenate([g.uniform(-4, 4, (n, 3)), g.integers(0, 256, (n, 3))], 1).astype(np.float32)
        bb = np.concatenate([g.uniform(-2.5, 2.5, (k, 3)), g.uniform(0.2, 2.0, (k, 3)),
                             ids[g.integers(0, len(ids), k)][:, None]], 1)
        scans.append((vert, bb))
    ds = scannet.ScannetDetectionDataset(cfg, split_set="train", use_color=True, augment=True,
                                         device="cuda", scans=scans)
    inds = list(range(8))
    rng = np.random.RandomState(0)
    for _ in range(5):
        ds.get_batch(inds, rng=rng)
    torch.cuda.synchronize()
    # host time of the random plan alone
    ch, par = np.empty((8, 40000), np.int64), np.zeros((8, 8))
    t0 = time.perf_counter()
    for _ in range(a.iters):
        for b in range(8):
            ds._draw(rng, 50000, ch[b], par[b])
    plan_ms = (time.perf_counter() - t0) / a.iters * 1e3
    t0 = time.perf_counter()
    for _ in range(a.iters):
        ds.get_batch(inds, rng=rng)
    torch.cuda.synchronize()
    batch_ms = (time.perf_counter() - t0) / a.iters * 1e3
    names = ("ov3d_scan_sample_aug", "ov3d_scan_labels")
    nat.timing_enable(names)
    for _ in range(a.iters):
        ds.get_batch(inds, rng=rng)
    kern = {n: float(np.median([r["ms"] for r in v])) * 1e3 for n, v in nat.timing_collect().items()}

    # the row gather at the real shape against torch.index_select, alternating
    S, R, D, B, N = 8, 50000, 512, 8, 40000
    feat = torch.randn((S, R, D), device="cuda", dtype=torch.float16)
    idx = torch.arange(B, device="cuda")
    choice = torch.stack([torch.randperm(R, device="cuda")[:N] for _ in range(B)])
    flat = (idx[:, None] * R + choice).reshape(-1)
    feat2 = feat.view(S * R, D)
    out = torch.empty((B, N, D), device="cuda", dtype=torch.float16)
    out2 = torch.empty((B * N, D), device="cuda", dtype=torch.float16)
    for _ in range(5):
        scannet.rows_gather(feat, idx, choice, out=out)
        torch.index_select(feat2, 0, flat, out=out2)
    torch.cuda.synchronize()
    assert torch.equal(out.view(B * N, D), out2)
    ours, lib = [], []
    for _ in range(a.iters):
        for fn, acc in ((lambda: scannet.rows_gather(feat, idx, choice, out=out), ours),
                        (lambda: torch.index_select(feat2, 0, flat, out=out2), lib)):
            # REPS launches back to back per event pair: the queue stays full, so the host's
            # time to issue a launch is not counted as device time
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(REPS):
                fn()
            e1.record()
            e1.synchronize()
            acc.append(e0.elapsed_time(e1) * 1e3 / REPS)
    nbytes = 2 * B * N * D * 2 + B * N * 8
    res = {
        "plan_host_ms": plan_ms, "get_batch_wall_ms": batch_ms, "kernel_us": kern,
        "gather_us": float(np.median(ours)), "gather_us_min": float(np.min(ours)),
        "index_select_us": float(np.median(lib)), "index_select_us_min": float(np.min(lib)),
        "gather_bytes": nbytes,
        "gather_share_of_hbm_peak": nbytes / (float(np.median(ours)) * 1e-6) / HBM_PEAK,
        "index_select_share_of_hbm_peak": nbytes / (float(np.median(lib)) * 1e-6) / HBM_PEAK,
        "iters": a.iters,
    }
    print(json.dumps(res))


if __name__ == "__main__":
    main()
