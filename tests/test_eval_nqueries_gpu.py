"""Evaluation at more queries than the checkpoint was trained with: no parameter of the model
depends on the number of queries, so the eval fixtures' weights (model_*_eval.npz) are built
with num_queries = 512 (and 1024) and run through the eval forward and the device evaluation.

a. the bf16 HIP eval forward against the fp32 eval forward of the same weights, with the bars
   test_eval_forward_gpu.py applies to the bf16 outputs (_bf16_vs_torch: per quantile within
   2x / 2.5x PyTorch's own bf16 execution, or full_fixture.BF16_TOL);
b. the outputs through APCalculator.step_meter / compute_metrics (more than 256 proposals per
   scene) against oracle/evaldet_ref.py on the same outputs: the bars of test_evaldet_gpu.py;
c. one run per dataset at 1024 queries: forward and evaluation complete with finite results.
"""
import argparse

import numpy as np
import pytest
import torch

import full_fixture as F
from helpers import fixture_args
from test_eval_forward_gpu import _bf16_vs_torch

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
KEYS = sorted(F.fixture_prefix(F.eval_fixture(*F.EVAL_CASES[0][:2]), "out/0/"))
MAX_GT = 8     # GT boxes kept per scene: the CPU restatement walks every (detection, GT) pair


def _build(cuda, name, name_eval, ds, nqueries):
    fx = F.eval_fixture(name, name_eval)
    args = fixture_args(fx)
    assert args.nqueries < nqueries
    args = argparse.Namespace(**{**vars(args), "nqueries": nqueries})
    model, cfg, _ = F.build(fx, cuda, ds, train=False, args=args)
    batch = F.eval_batch(fx, cuda)
    present = batch["gt_box_present"]
    batch["gt_box_present"] = present * (torch.cumsum(present, 1) <= MAX_GT).to(present.dtype)
    return model, cfg, batch


_CACHE = {}


def _case(cuda, name, name_eval, ds):
    """model at 512 queries, its batch and the three forwards (fp32, bf16 HIP, bf16 PyTorch):
    computed once, read by both tests"""
    if ds not in _CACHE:
        torch.backends.cuda.matmul.allow_tf32 = False
        model, cfg, batch = _build(cuda, name, name_eval, ds, 512)
        ref = F.eval_forward(model, batch)
        hip = F.eval_forward(model, batch, BF16)
        with F.torch_bf16_path():
            base = F.eval_forward(model, batch, BF16)
        _CACHE[ds] = (cfg, batch, ref, hip, base)
    return _CACHE[ds]


def _errors(out, ref):
    rep = []
    for li, (lay, rlay) in enumerate(zip(F.layers_of(out), F.layers_of(ref))):
        assert set(lay) == set(rlay)
        for k in KEYS:              # the entries test_eval_forward_gpu.py compares
            v = lay[k]
            assert v.shape == rlay[k].shape and v.shape[1] == 512, (li, k, v.shape)
            rep.append((F.rel(v.double().cpu().numpy(), rlay[k].double().cpu().numpy()), f"{li}/{k}"))
    return {"out": sorted(rep, reverse=True)}


@pytest.mark.parametrize("name,name_eval,ds", F.EVAL_CASES)
def test_bf16_eval_forward_at_512_queries(cuda, name, name_eval, ds):
    _, _, ref, hip, base = _case(cuda, name, name_eval, ds)
    lines, bad = _bf16_vs_torch(_errors(hip, ref), _errors(base, ref), ("out",))
    print(name_eval, "512 queries, bf16 eval hip/torch vs fp32:\n  " + "\n  ".join(lines))
    assert not bad, (bad, lines)


def _check_metrics(got, ref):
    for th, d in got.items():
        assert set(d) == set(ref[th]), set(d) ^ set(ref[th])
        for k, v in d.items():
            if k == "mAP":
                assert np.float32(v) == np.float32(ref[th][k]), (th, v, ref[th][k])
            else:
                assert abs(float(v) - float(ref[th][k])) <= 1e-12, (th, k, v, ref[th][k])


@pytest.mark.parametrize("name,name_eval,ds", F.EVAL_CASES)
def test_eval_at_512_queries_into_ap_calculator(cuda, name, name_eval, ds):
    from oracle import evaldet_ref as E
    from ov3d_amd import ap_calculator as apc
    cfg, batch, _, hip, _ = _case(cuda, name, name_eval, ds)
    calc = apc.APCalculator(cfg, ap_iou_thresh=[0.25, 0.5], class2type_map=None, exact_eval=True)
    calc.step_meter(hip, batch)
    got = calc.compute_metrics()
    out = hip["outputs"]
    h = lambda t: t.detach().float().cpu().numpy()   # noqa: E731
    corners, probs, obj = h(out["box_corners"]), h(out["sem_cls_prob"]), h(out["objectness_prob"])
    assert obj.shape == (2, 512) and int(batch["gt_box_present"].sum(1).max()) <= MAX_GT
    ref_scores = E.detections(corners, probs, obj, h(batch["point_clouds"]), calc.ap_config_dict,
                              cfg.num_semcls)
    sc = h(calc._scores[0])
    print(name_eval, "512 queries: detections", int(np.isfinite(ref_scores).any(-1).sum()), "of", obj.size)
    assert np.array_equal(sc.view(np.uint32), ref_scores.view(np.uint32))
    ref = E.compute_metrics(ref_scores, corners, h(batch["gt_box_corners"]),
                            batch["gt_box_sem_cls_label"].cpu().numpy(),
                            batch["gt_box_present"].cpu().numpy(), [0.25, 0.5])
    _check_metrics(got, ref)


@pytest.mark.parametrize("name,name_eval,ds", F.EVAL_CASES)
def test_eval_at_1024_queries_completes(cuda, name, name_eval, ds):
    """SUN RGB-D: 1024 of the vanilla encoder's 2048 points; ScanNet: every one of the masked
    encoder's 1024 points is a query"""
    from ov3d_amd import ap_calculator as apc
    model, cfg, batch = _build(cuda, name, name_eval, ds, 1024)
    out = F.eval_forward(model, batch, BF16)
    for k, v in out["outputs"].items():
        assert v.shape[:2] == (2, 1024) and bool(torch.isfinite(v.float()).all()), k
    calc = apc.APCalculator(cfg, ap_iou_thresh=[0.25, 0.5], class2type_map=None, exact_eval=True)
    calc.step_meter(out, batch)
    met = calc.compute_metrics()
    for th in (0.25, 0.5):
        assert np.isfinite(float(met[th]["mAP"])) and np.isfinite(float(met[th]["AR"]))
