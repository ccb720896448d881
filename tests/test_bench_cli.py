"""bench.py's command line: --dump-outputs writes the last timed step's loss / parameters /
gradients as float32 .npy (a fixed seeded sample of what is over the budget), and a plain run
leaves the measurements that take runs of their own (--full) out of its result line."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from helpers import ROOT


def _model():
    torch.manual_seed(3)
    m = torch.nn.Sequential(torch.nn.Linear(7, 5), torch.nn.Linear(5, 3))
    m(torch.ones(2, 7)).sum().backward()
    return m


def test_dump_outputs_whole_arrays(tmp_path):
    import bench
    m = _model()
    bench.dump_outputs(str(tmp_path / "d"), torch.tensor(1.5, dtype=torch.float64), m)
    got = {f[:-4]: np.load(tmp_path / "d" / f) for f in sorted(os.listdir(tmp_path / "d"))}
    assert sorted(got) == ["grads", "loss", "params"]
    assert all(a.dtype == np.float32 and a.ndim == 1 for a in got.values())
    assert got["loss"].tolist() == [1.5]
    flat = torch.cat([p.detach().reshape(-1) for p in m.parameters()]).numpy()
    assert np.array_equal(got["params"], flat)
    assert np.array_equal(got["grads"], torch.cat([p.grad.reshape(-1) for p in m.parameters()]).numpy())


def test_dump_outputs_samples_over_budget(tmp_path, monkeypatch):
    import bench
    m = _model()
    n = sum(p.numel() for p in m.parameters())          # 58 per array
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 4 * 41)   # loss 1 + 20 + 20 elements
    bench.dump_outputs(str(tmp_path / "a"), torch.tensor(2.0), m)
    bench.dump_outputs(str(tmp_path / "b"), torch.tensor(2.0), m)
    a = {k: np.load(tmp_path / "a" / (k + ".npy")) for k in ("loss", "params", "grads")}
    assert a["loss"].size == 1 and a["params"].size == 20 and a["grads"].size == 20
    assert sum(v.nbytes for v in a.values()) <= 4 * 41
    for k, v in a.items():   # the same positions every time
        assert np.array_equal(v, np.load(tmp_path / "b" / (k + ".npy")))
    flat = torch.cat([p.detach().reshape(-1) for p in m.parameters()]).numpy()
    pick = np.sort(np.random.Generator(np.random.PCG64(0)).choice(n, size=20, replace=False))
    assert np.array_equal(a["params"], flat[pick])


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_outputs(tmp_path):
    out = str(tmp_path / "dump")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2",
                        "--warmup", "1", "--batch", "2", "--points", "4096", "--dump-outputs", out],
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout
    res = json.loads(lines[0])
    assert res["steps"] == 2 and res["value"] > 0 and res["ms_per_step"] > 0
    assert res["unit"] == "scenes/s" and res["higher_is_better"] is True and res["dtype"] == "bf16"
    assert abs(res["value"] * res["ms_per_step"] / 1e3 - 2) < 1e-2   # scenes/s x s/step = batch
    # what takes runs of its own is measured under --full only
    assert res["roofline"] is None
    for k in ("cpu_baseline", "attn_bwd", "gemm_ceiling", "index_kernels_hbm", "fps"):
        assert k not in res, k
    arrays = {k: np.load(os.path.join(out, k + ".npy")) for k in ("loss", "params", "grads")}
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in arrays.values())
    assert arrays["loss"].shape == (1,) and arrays["params"].shape == arrays["grads"].shape
    assert arrays["params"].size > 1000 and np.abs(arrays["grads"]).max() > 0
    assert sum(a.nbytes for a in arrays.values()) <= 64 * 10 ** 6
