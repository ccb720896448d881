"""Times of the multiview back-projection at the ScanNet shape (50 000 vertices x 100 and 300
frames of 41 x 32 pixels, 128 feature channels), on the GPU:

  tables   image_processor.compute_projection (frame table, count, write: three launches) and
  compose  projection.compose_features, float32 features into (N, C) rows (two launches):
           device events around 20 back-to-back calls on resident inputs after a warm-up, per
           call, the median of 30 such windows; the host clock around one call ending in a
           synchronise (end to end: the allocations and launches included); the bytes the result needs (tables: 16 F (N+1)
           written; compose: F H W 4 read + N C 4 written) and the multiple of the time those
           bytes take at the measured HBM copy rate (6.29 TB/s)
  numpy    the restatement (tests/backproj_ref.py, one core) on the same inputs, on the first
           `numpy_frames` frames, scaled to F; its results are compared with the device's on
           those frames

  python tools/backproj_time.py [--out FILE.json]      (default: profiles/backproj_time.json)
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
import backproj_cases as BC  # noqa: E402
import backproj_ref as R  # noqa: E402
from lift_cases import look_at  # noqa: E402
from ov3d_amd import image_util, projection  # noqa: E402

N, C = 50000, 128
FRAMES = (100, 300)
NUMPY_FRAMES = 10
HBM_BPS = 6.29e12
W, H = BC.IMAGE_DIMS


def scene(F):
    rng = np.random.Generator(np.random.PCG64(F))
    pts = BC.draw_points(rng, N)
    par = R.params()
    poses = np.stack([look_at(rng.uniform([0.4, 0.4, 1.0], [4.6, 3.6, 2.0]),
                              pts[rng.integers(0, N)].astype(np.float64)) for _ in range(F)])
    depth = np.stack([BC.ray_cast(P, par) for P in poses])
    feats = torch.from_numpy(rng.standard_normal((F, 8, H, W)).astype(np.float32)).repeat(1, C // 8, 1, 1)
    return pts, depth, poses, feats.contiguous()


def timed(fn, reps=30, inner=20, warm=5):
    """-> per call: (device-event median ms, min, max over `reps` windows of `inner` back-to-back
    calls, host-clock median ms of one call + synchronise)"""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ev, wall = [], []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        e1.synchronize()
        ev.append(e0.elapsed_time(e1) / inner)
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ev), min(ev), max(ev), statistics.median(wall)


def measure(dev, F):
    pts, depth, poses, feats = scene(F)
    proc = image_util.image_processor()
    d = [torch.from_numpy(x).to(dev) for x in (pts, depth, poses)] + [feats.to(dev)]
    res = {"F": F, "N": N, "C": C}
    med, lo, hi, wall = timed(lambda: proc.compute_projection(*d[:3]))
    nbytes = 16 * F * (N + 1)
    res["tables"] = {"device_ms_median": med, "device_ms_min": lo, "device_ms_max": hi, "end_to_end_ms_median": wall,
                     "bytes": nbytes, "floor_ms": nbytes / HBM_BPS * 1e3, "times_floor": med / (nbytes / HBM_BPS * 1e3)}
    med, lo, hi, wall = timed(lambda: projection.compose_features(*d, rows=True))
    nbytes = F * H * W * 4 + N * C * 4
    res["compose"] = {"device_ms_median": med, "device_ms_min": lo, "device_ms_max": hi, "end_to_end_ms_median": wall,
                      "bytes": nbytes, "floor_ms": nbytes / HBM_BPS * 1e3, "times_floor": med / (nbytes / HBM_BPS * 1e3)}
    # the restatement on the first frames, one core, and the comparison
    k = NUMPY_FRAMES
    par = R.params()
    t0 = time.perf_counter()
    i3, i2 = R.tables(pts, depth[:k], poses[:k], par)
    t_tab = time.perf_counter() - t0
    f_host = feats[:k].numpy()
    t0 = time.perf_counter()
    comp, frame = R.compose_loop(f_host, i3, i2, N)
    t_comp = time.perf_counter() - t0
    g3, g2 = proc.compute_projection(d[0], d[1][:k], d[2][:k])
    out, fr = projection.compose_features(d[0], d[1][:k], d[2][:k], d[3][:k], rows=True)
    assert np.array_equal(g3.cpu().numpy(), i3) and np.array_equal(g2.cpu().numpy(), i2)
    assert np.array_equal(out.cpu().numpy(), comp.T) and np.array_equal(fr.cpu().numpy(), frame)
    res["numpy"] = {"frames_timed": k, "tables_ms_scaled_to_F": t_tab / k * F * 1e3,
                    "compose_ms_scaled_to_F": (t_tab + t_comp) / k * F * 1e3,
                    "mapped_per_frame_mean": float(i3[:, 0].mean())}
    res["tables"]["speedup_over_numpy"] = res["numpy"]["tables_ms_scaled_to_F"] / res["tables"]["end_to_end_ms_median"]
    res["compose"]["speedup_over_numpy"] = res["numpy"]["compose_ms_scaled_to_F"] / res["compose"]["end_to_end_ms_median"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "backproj_time.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs the GPU: a time taken anywhere else says nothing")
    torch.set_num_threads(1)
    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(0), "hbm_copy_rate_Bps": HBM_BPS,
           "shapes": [measure(dev, F) for F in FRAMES]}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
