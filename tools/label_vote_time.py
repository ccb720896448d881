"""Times of pseudo-label generation at the ScanNet shape (8 scans x 150 000 vertices x 256
boxes, 18 classes), on the GPU:

  kernel  box_label_votes (ov3d_box_points_count kind 1), float32 and float64 points: device
          events around single launches after a warm-up, the median; beside it the algorithmic
          bytes (every 8-box tile reads all N points and labels: ceil(K/8) * B * N * (12 or
          24 + 1) B, served mostly from cache after the first tile) and the rate they give;
          the results are checked against the numpy restatement on one scene
  save    LabelFormatter.save() of the same 8 scans x 256 boxes end to end (uploads, launch,
          read-back, file writes), host clock, against the restatement's gen_pseudo loop
          (tests/pseudo_label_ref.py, one numpy pass per box, one core) on the same inputs;
          the files of the two are compared

  python tools/label_vote_time.py [--out FILE.json]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import ov3d_import  # noqa: E402

ov3d_import.load()
import pseudo_label_ref as R  # noqa: E402
from ov3d_amd import label_formatter as LF  # noqa: E402

B, N, K, C = 8, 150000, 256, 18


def scene(rng, dtype):
    """a room of 18 labelled blobs and K candidate rows (centre, size, class, 1, 1, scan)"""
    cls = rng.integers(0, C, N)
    ctr = np.stack([(cls % 6) * 1.2, (cls // 6) * 1.2, np.full(N, 1.0)], 1)
    xyz = ctr + rng.integers(-48, 49, (N, 3)) / 64.0
    lab = cls.astype(np.float64)
    lab[rng.random(N) < 0.1] = -100
    bc = rng.integers(0, C, K)
    at = np.where(rng.random(K) < 0.7, bc, (bc + 1) % C)
    bctr = np.stack([(at % 6) * 1.2, (at // 6) * 1.2, np.full(K, 1.0)], 1) + rng.integers(-8, 9, (K, 3)) / 32.0
    size = rng.integers(4, 41, (K, 3)) / 32.0
    rows = np.concatenate([bctr, size, bc[:, None], np.ones((K, 2)), np.zeros((K, 1))], 1).astype(np.float32)
    return np.concatenate([xyz, lab[:, None]], 1).astype(dtype), rows


def kernel_time(dev, dtype, scans, rows, reps=30):
    pts = torch.from_numpy(np.stack([s[:, :3] for s in scans])).to(dev)
    lab = torch.from_numpy(np.stack([LF.scan_labels(s[:, 3], C, "s") for s in scans])).to(dev)
    lohi = [R.bounds(r) for r in rows]
    lo = torch.from_numpy(np.stack([x[0] for x in lohi])).to(dev)
    hi = torch.from_numpy(np.stack([x[1] for x in lohi])).to(dev)
    for _ in range(5):
        counts, mode = LF.box_label_votes(pts, lab, lo, hi, C)
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        counts, mode = LF.box_label_votes(pts, lab, lo, hi, C)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    rc, rm = R.vote(pts[:1].cpu().numpy(), lab[:1].cpu().numpy(), lo[:1].cpu().numpy(),
                    hi[:1].cpu().numpy(), C)
    assert np.array_equal(counts[:1].cpu().numpy(), rc) and np.array_equal(mode[:1].cpu().numpy(), rm)
    nbytes = -(-K // 8) * B * N * (pts.element_size() * 3 + 1)
    med = statistics.median(ms)
    return {"points": str(pts.dtype), "median_ms": med, "min_ms": min(ms), "max_ms": max(ms),
            "algorithmic_bytes": nbytes, "GBps": nbytes / med / 1e6, "launches": reps}


def save_time(dev, scans, rows):
    pb = np.concatenate([np.concatenate([r[:, :9], np.full((K, 1), i, np.float32)], 1)
                         for i, r in enumerate(rows)])
    names = ["scene%04d_00" % i for i in range(B)]
    with tempfile.TemporaryDirectory() as tmp:
        a, b = os.path.join(tmp, "device"), os.path.join(tmp, "numpy")
        os.makedirs(b)
        lf = LF.LabelFormatter("", a, None, names, device=dev, scans=scans, group=B)
        lf.pseudo_boxes = pb
        lf.save()                                        # warm-up (code objects, allocator)
        ts = []
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            kept = lf.save()
            ts.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        for i, n in enumerate(names):
            np.save(os.path.join(b, n + "_bbox.npy"), R.gen_pseudo(pb, i, scans[i]))
        t_ref = time.perf_counter() - t0
        for n in names:
            x, y = np.load(os.path.join(a, n + "_bbox.npy")), np.load(os.path.join(b, n + "_bbox.npy"))
            assert x.dtype == y.dtype and np.array_equal(x, y), n
    return {"save_s_median": statistics.median(ts), "save_s_all": ts, "numpy_gen_pseudo_s": t_ref,
            "boxes": B * K, "kept": int(kept), "speedup": t_ref / statistics.median(ts)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs the GPU: a time taken anywhere else says nothing")
    torch.set_num_threads(1)
    dev = torch.device("cuda", 0)
    res = {"shape": {"B": B, "N": N, "K": K, "C": C}, "device": torch.cuda.get_device_name(0)}
    for dtype in (np.float32, np.float64):
        rng = np.random.Generator(np.random.PCG64(77))
        pairs = [scene(rng, dtype) for _ in range(B)]
        scans, rows = [p[0] for p in pairs], [p[1] for p in pairs]
        res["kernel_" + np.dtype(dtype).name] = kernel_time(dev, dtype, scans, rows)
        if dtype == np.float32:
            res["save_float32"] = save_time(dev, scans, rows)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
