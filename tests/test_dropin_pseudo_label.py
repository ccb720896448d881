"""Drop-in proof for pseudo-label generation: the REFERENCE's own inference loop
(/root/reference/engine.py:235-302), imported unchanged, with ``utils.label_formatter`` aliased
to ov3d_amd.label_formatter drives the reduced product model and the
product's LabelFormatter, and ``process`` writes the same files as the same loop run with the
reference's own formatter.  Host suite: the HIP index ops come from the C oracle
(oracle/torch_shim.py) and the vote from the numpy restatement.

Runs where the reference sources are (skipped where they are absent, e.g. on the GPU box)."""
import argparse
import importlib.util
import os
import sys
import types

import numpy as np
import pytest
import torch

REF = "/root/reference"
pytestmark = pytest.mark.skipif(not os.path.isdir(REF), reason="needs the reference sources")


def _engine(monkeypatch, formatter_module):
    import ov3d_amd.dist
    monkeypatch.setitem(sys.modules, "utils.dist", ov3d_amd.dist)
    monkeypatch.setitem(sys.modules, "utils.label_formatter", formatter_module)
    spec = importlib.util.spec_from_file_location("ref_engine", os.path.join(REF, "engine.py"))
    eng = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(eng)
    return eng


def test_reference_inference_loop_drives_the_product_formatter(monkeypatch, tmp_path):
    from helpers import batch_from_fixture, build_model_from_fixture, fixture, ov3d
    from ref_loader import load_reference
    from oracle import torch_shim
    import pseudo_label_ref as R
    load_reference()
    import utils.label_formatter as ref_lf          # the reference's own module
    import ov3d_amd.label_formatter as LF
    monkeypatch.setattr(torch.cuda, "max_memory_allocated", lambda *a, **k: 0)
    monkeypatch.setattr(LF, "box_label_votes", R.vote_torch)
    torch.set_num_threads(8)
    fx = fixture("model_scannet.npz")
    saved = torch_shim.install(ov3d)                  # before the model is built: its groupers
    try:
        model, cfg, _ = build_model_from_fixture(fx, "cpu", "scannet")
        results = _run_both(monkeypatch, tmp_path, model, cfg, fx, LF, ref_lf)
    finally:
        torch_shim.uninstall(saved)
    B = 2
    (pa, ta, fa), (pb, tb, fb) = results["product"], results["reference"]
    assert pa.dtype == pb.dtype and np.array_equal(pa, pb) and pa.shape[0] >= B * 8
    assert ta == tb
    for a, b in zip(fa, fb):
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)
    assert fa[-1].shape == (0, 7)
    print("drop-in: %d past the thresholds, %d kept" % (pa.shape[0], ta))


def _run_both(monkeypatch, tmp_path, model, cfg, fx, LF, ref_lf):
    from helpers import batch_from_fixture
    batch = batch_from_fixture(fx, "cpu")
    B = batch["point_clouds"].shape[0]
    batch["scan_idx"] = torch.arange(B, dtype=torch.int64)
    names = ["scene%04d_00" % i for i in range(B + 1)]          # the last one: never stepped
    lseg = tmp_path / "lseg"
    lseg.mkdir()
    rng = np.random.Generator(np.random.PCG64(17))
    for i, n in enumerate(names):
        xyz = batch["point_clouds"][i % B, :, :3].numpy().astype(np.float64 if i == 1 else np.float32)
        lab = np.floor(xyz[:, 0] * 2 + i) % 20                   # 18, 19: ignored
        lab[rng.random(len(lab)) < 0.1] = -100
        np.save(str(lseg / (n + ".npy")), np.concatenate([xyz, lab[:, None].astype(xyz.dtype)], 1))
    results = {}
    for key, module in (("product", LF), ("reference", ref_lf)):
        out_dir = tmp_path / key
        args = argparse.Namespace(in_dir="", out_dir=str(out_dir), feature_2d_dir=str(lseg),
                                  log_every=10)
        eng = _engine(monkeypatch, module)
        assert eng.LabelFormatter is module.LabelFormatter
        lf, _ = eng.inference(args, -1, model, cfg, types.SimpleNamespace(scan_names=names),
                              [{k: v.clone() for k, v in batch.items()}], types.SimpleNamespace(
                                  log_scalars=lambda *a, **k: None), 0)
        assert type(lf) is module.LabelFormatter
        if key == "product":
            lf.device = torch.device("cpu")                  # the loop builds it with the default
            rows = lf.boxes[0].numpy()
            th_s = float(np.median(rows[:, 7]))
        if key == "reference":
            # its own save() is a process pool over gen_pseudo; call that scan by scan
            lf.compute(50, th_s, 0.0)
            total = sum(lf.gen_pseudo(i) for i in range(len(names)))
        else:
            lf.compute(50, th_s, 0.0)
            total = lf.save()
        results[key] = (lf.pseudo_boxes, total,
                        [np.load(str(out_dir / (n + "_bbox.npy"))) for n in names])
    return results
