"""Times of the open-vocabulary classification launch at the ScanNet shape (150 000 vertices x
512 channels, the rows compose_features(rows=True) leaves), on the GPU:

  kernel  ov3d_openvocab_classify through open_vocab.classify_rows, T = 19 and T = 200, bfloat16
          and float32: device events around single launches after a warm-up, median and minimum
  torch   the restatement (features.float() @ text.float().T).max(1) on the same device and
          inputs, timed the same way, in alternation with the kernel
  floor   the bytes the launch has to move (R * C features + T * C text + 12 R of results) over
          the HBM rate, both the 8.0 TB/s of the data sheet and the 6.3 TB/s a copy achieves

The launches rotate over several feature buffers that together exceed the 256 MiB Infinity
Cache, so every timed launch streams its features from HBM.  The labels are compared with the
torch restatement's on one buffer (float32 sums in another order: near-ties may differ).

  python tools/openvocab_time.py [--out FILE.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import ov3d_import  # noqa: E402

ov3d_import.load()
from ov3d_amd import open_vocab as OV  # noqa: E402

R, C = 150000, 512
HBM_SPEC, HBM_COPY = 8.0e12, 6.3e12
CACHE = 256 << 20


def timed(fn, bufs, reps):
    ms = []
    for i in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn(bufs[i % len(bufs)])
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms


def case(dev, dtype, T, reps=40):
    gen = torch.Generator(device=dev).manual_seed(1000 + T)
    size = torch.empty((), dtype=dtype).element_size()
    nbuf = CACHE // (R * C * size) + 2
    bufs = [torch.randn((R, C), generator=gen, device=dev, dtype=torch.float32).to(dtype) for _ in range(nbuf)]
    text = OV.prepare_text(torch.randn((T, C), generator=gen, device=dev, dtype=torch.float32), dtype)
    text32 = text.float()

    def kernel(f):
        return OV.classify_rows(f, text)

    def restatement(f):
        return (f.float() @ text32.T).max(1)

    for f in bufs:
        kernel(f)
        restatement(f)
    k_ms, t_ms = [], []
    for _ in range(4):                                     # alternate: both see the same machine
        k_ms += timed(kernel, bufs, reps // 4)
        t_ms += timed(restatement, bufs, reps // 4)
    label = kernel(bufs[0])[0]
    agree = float((label.long() == restatement(bufs[0]).indices).float().mean())
    nbytes = R * C * size + T * C * size + 12 * R
    med = statistics.median(k_ms)
    return {"dtype": str(dtype), "T": T, "median_ms": med, "min_ms": min(k_ms), "max_ms": max(k_ms),
            "torch_median_ms": statistics.median(t_ms), "torch_min_ms": min(t_ms),
            "bytes": nbytes, "GBps": nbytes / med / 1e6, "flop": 2 * R * C * T,
            "floor_ms_8.0TBps": nbytes / HBM_SPEC * 1e3, "floor_ms_6.3TBps": nbytes / HBM_COPY * 1e3,
            "over_floor_6.3TBps": med / (nbytes / HBM_COPY * 1e3), "buffers": nbuf, "launches": len(k_ms),
            "labels_equal_to_torch": agree}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs the GPU: a time taken anywhere else says nothing")
    dev = torch.device("cuda", 0)
    res = {"shape": {"R": R, "C": C}, "device": torch.cuda.get_device_name(0), "cases": []}
    for dtype in (torch.bfloat16, torch.float32):
        for T in (19, 200):
            res["cases"].append(case(dev, dtype, T))
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
