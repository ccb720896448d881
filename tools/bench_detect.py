"""Time of detecting with a vocabulary chosen at inference time (ov3d_amd.detect): the
ov3d_vocab_score launch at the detector's sizes, R = 8 x 256 and 8 x 2048 query embeddings of
C = 640 channels against T = 19, 201, 1204 and 4096 text rows in float32 and bfloat16, beside the
torch form on the same device in float32 (visual @ text.T, softmax, topk: it materialises the
(R, T) scores), and detect() end to end.  Device events around single launches, rounds of the
kernel alternating with rounds of the torch form; detect() on the host clock around work that
ends in a synchronise.  Prints one JSON object.

    python tools/bench_detect.py [--reps 40] [--rounds 4]
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
from ov3d_amd import detect as D  # noqa: E402
from ov3d_amd.dataset_config import SunrgbdDatasetConfig  # noqa: E402

L2_TBS = 34.5           # aggregate L2 bandwidth of the part (MI355X_MICROARCH.md), TB/s
F32_MFMA_TFLOPS = 157.0  # 64 FLOP per clock and SIMD
K = 5


def timed(fn, reps):
    """device-event times of `reps` single calls, ms"""
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def stats(ms):
    a = np.array(ms) * 1e3
    return {"median_us": round(float(np.median(a)), 1), "min_us": round(float(a.min()), 1),
            "max_us": round(float(a.max()), 1)}


def grid_of(R, T, k):
    """the launch geometry of csrc/vocabscore.hip: (workgroups, rows per workgroup, threads)"""
    if T <= 32 or k > 8:
        rows, threads = 16, 64          # one wave
    elif R > 4096:
        rows, threads = 64, 256         # four waves, 16 rows each
    else:
        rows, threads = 16, 256         # four waves, a quarter of the tile's text blocks each
    return -(-R // rows), rows, threads


def torch_form(visual32, text32, bg):
    p = torch.softmax(visual32 @ text32.t(), -1)
    obj = 1 - p[:, bg]
    top = torch.topk(torch.cat([p[:, :bg], p[:, bg + 1:]], 1), K, dim=1)
    return obj, top.values, top.indices


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=4)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_detect: no ROCm device; nothing is measured on the host")
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    C = 640
    res = {"workload": f"ov3d_vocab_score, C = {C}, k = {K}, background last; device events, median of "
                       f"{a.reps} launches in {a.rounds} rounds alternating with the torch form",
           "device": torch.cuda.get_device_name(0), "score_queries": []}
    per = max(1, a.reps // a.rounds)
    for R in (8 * 256, 8 * 2048):
        visual = rng.standard_normal((R, C))
        for T in (19, 201, 1204, 4096):
            text = rng.standard_normal((T, C)) / np.sqrt(C)
            v32 = torch.from_numpy(visual).float().to(dev)
            t32 = torch.from_numpy(text).float().to(dev)
            row = {"R": R, "T": T}
            ours = {}
            for name, dtype in (("float32", torch.float32), ("bfloat16", torch.bfloat16)):
                vocab = D.Vocabulary(text, dtype=dtype, device=dev)
                ours[name] = (v32.to(dtype), vocab)
            runs = {"float32": [], "bfloat16": [], "torch_float32": []}
            for fn in ([lambda n=n: D.score_queries(*ours[n], K) for n in ours] + [lambda: torch_form(v32, t32, T - 1)]):
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            for _ in range(a.rounds):
                for n in ours:
                    runs[n] += timed(lambda n=n: D.score_queries(*ours[n], K), per)
                runs["torch_float32"] += timed(lambda: torch_form(v32, t32, T - 1), per)
            got = D.score_queries(*ours["float32"], K)
            want = torch_form(v32, t32, T - 1)
            fg = torch.where(got[2] >= T - 1, got[2] - 1, got[2])        # foreground numbering of the torch form
            row["top1_equal_torch"] = float((fg[:, 0].long() == want[2][:, 0]).float().mean())
            row["obj_max_abs_diff_torch"] = float((got[0] - want[0]).abs().max())
            wgs, rows, threads = grid_of(R, T, K)
            row["grid"] = {"workgroups": wgs, "rows_per_workgroup": rows, "threads": threads}
            for n, size in (("float32", 4), ("bfloat16", 2)):
                s = stats(runs[n])
                streamed = wgs * T * C * size                              # every workgroup reads the whole table
                s["text_bytes_streamed"] = streamed
                s["text_stream_TBps"] = round(streamed / (s["median_us"] * 1e-6) / 1e12, 3)
                s["share_of_L2_peak"] = round(s["text_stream_TBps"] / L2_TBS, 3)
                s["TFLOPs"] = round(2.0 * R * T * C / (s["median_us"] * 1e-6) / 1e12, 2)
                row[n] = s
            row["float32"]["share_of_f32_mfma_peak"] = round(row["float32"]["TFLOPs"] / F32_MFMA_TFLOPS, 3)
            row["torch_float32"] = stats(runs["torch_float32"])
            row["torch_over_ours_float32"] = round(row["torch_float32"]["median_us"] / row["float32"]["median_us"], 2)
            row["torch_over_ours_bfloat16"] = round(row["torch_float32"]["median_us"] / row["bfloat16"]["median_us"], 2)
            res["score_queries"].append(row)

    # detect() end to end: 8 scenes x 256 queries, 20000 points, 1203 names and a background
    B, Q, N, T = 8, 256, 20000, 1204
    cfg = SunrgbdDatasetConfig()
    cen = np.stack([rng.uniform(-2.8, 2.8, (B, Q)), rng.uniform(0.7, 6.3, (B, Q)), rng.uniform(0.1, 2.5, (B, Q))], -1)
    corners = cfg.box_parametrization_to_corners_np(cen.astype(np.float32), rng.uniform(0.2, 1.5, (B, Q, 3)).astype(
        np.float32), rng.uniform(-np.pi, np.pi, (B, Q)).astype(np.float32))
    pts = np.stack([rng.uniform(-3, 3, (B, N)), rng.uniform(-2.5, 0.5, (B, N)), rng.uniform(0.5, 6.5, (B, N))], -1)
    out = {"visual_embeds": torch.from_numpy(rng.standard_normal((B, Q, C))).float().to(dev),
           "box_corners": torch.from_numpy(np.asarray(corners, np.float32)).to(dev)}
    points = torch.from_numpy(pts).float().to(dev)
    text = rng.standard_normal((T, C)) / np.sqrt(C)
    text[-1] += 0.4 * rng.standard_normal(C) / np.sqrt(C) + 0.2 / np.sqrt(C)
    vocab = D.Vocabulary(text, device=dev)
    for _ in range(3):
        dets = D.detect(out, vocab, points).to_list()
    torch.cuda.synchronize()
    t_dev, t_all = [], []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        det = D.detect(out, vocab, points)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        det.to_list()
        t2 = time.perf_counter()
        t_dev.append((t1 - t0) * 1e3)
        t_all.append((t2 - t0) * 1e3)
    res["detect"] = {"B": B, "Q": Q, "points": N, "T": T, "topk": 5, "detections": sum(len(s) for s in dets),
                     "to_synchronise": stats(t_dev), "with_to_list": stats(t_all)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
