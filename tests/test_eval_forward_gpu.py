"""The inference forward on the GPU: model.eval() under torch.no_grad(), fp32 and bf16 autocast,
as the reference's evaluate() (engine.py:154-231) drives it, against the REFERENCE run in
float64 in eval mode (tests/golden/model_{sun,scannet}_eval.npz, made by make_golden.py).

Eval is its own kernel mix, not a subset of the training step's: the SA modules leave the fused
training kernels for SharedMLP.rows (GEMM + F.batch_norm on running statistics + the neighbour
max), the heads leave the fused BN rows / output launch for the per-head fp32 path and the
unfused box parametrisation, the fused transformer kernels run with every dropout at 0 and the
seed never advanced, and the requires_grad branches take their other side under no_grad.

The fixture's running statistics are far from the batch's own (train-mode outputs differ from
eval-mode ones by >= 10x the fp32 bar on every key: train_vs_eval/ in the fixture) and its args
have the reference's dropouts on, so batch statistics in eval or a live dropout miss the bars.

Shapes: the _full fixtures' (2 scenes x 20000 points, 2048 pre-encoder points, 128 / 256
queries, 256-d, 4 heads of 64), the smallest at which the bf16 HIP kernels are selected.
"""
import argparse
import json
import os

import numpy as np
import pytest
import torch

import full_fixture as F
from helpers import fixture_args

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
AMPS = [pytest.param(None, id="fp32"), pytest.param(BF16, id="bf16")]


def _record(kind, name, obj):
    path = os.environ.get("OV3D_PARITY_RECORD")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps({"kind": kind, "case": name, **obj}, default=str) + "\n")


def _flat(out):
    return {f"{li}/{k}": v for li, lay in enumerate(F.layers_of(out)) for k, v in lay.items()}


def _assert_bit_equal(a, b):
    a, b = _flat(a), _flat(b)
    assert set(a) == set(b)
    diff = [k for k in a if not torch.equal(a[k], b[k])]
    assert not diff, diff


def _fp32_bad(rep, fx):
    """entries above max(FP32_TOL, 3 x the reference's own fp32 error on that entry)"""
    return F.fp32_failures(rep, fx, tol=F.FP32_TOL, slack=3.0)


def _quant(rep, group, q):
    return float(np.quantile(np.array([x for x, _ in rep[group]]), q))


def _bf16_vs_torch(rep, base, groups):
    """the scheme of test_bf16_step_matches_float64_reference: per group the median and 90th
    percentile within 2x PyTorch's own bf16, the worst within max(2.5x PyTorch's, BF16_TOL)"""
    lines, bad = [], []
    for g in groups:
        q = [(_quant(rep, g, p), _quant(base, g, p)) for p in (0.5, 0.9, 1.0)]
        lines.append("%s q50 %.2e/%.2e q90 %.2e/%.2e max %.2e/%.2e (%s)" % (
            g, *[v for pair in q for v in pair], rep[g][0][1]))
        # written as "not <=": a NaN error fails
        if not (q[0][0] <= 2 * q[0][1] + 1e-6 and q[1][0] <= 2 * q[1][1] + 1e-6 and
                q[2][0] <= max(2.5 * q[2][1], F.BF16_TOL[g])):
            bad.append(g)
    return lines, bad


# ------------------------------------------------------------------ a / b: parity
@pytest.mark.parametrize("name,name_eval,ds", F.EVAL_CASES)
def test_fp32_eval_matches_float64_reference(cuda, name, name_eval, ds):
    torch.backends.cuda.matmul.allow_tf32 = False
    fx = F.eval_fixture(name, name_eval)
    rep, _ = F.run_eval(fx, ds, cuda)
    assert len(rep["loss"]) == 57 and len(rep["out"]) == 89
    bad = _fp32_bad(rep, fx)
    worst = {g: F.worst(rep, g) for g in rep}
    print(name_eval, "fp32 eval worst:", worst)
    _record("eval_fp32", name_eval, {"worst": worst, "over_bar": bad})
    assert not bad, bad


@pytest.mark.parametrize("name,name_eval,ds", F.EVAL_CASES)
def test_bf16_eval_matches_float64_reference(cuda, name, name_eval, ds):
    fx = F.eval_fixture(name, name_eval)
    rep, _ = F.run_eval(fx, ds, cuda, amp=BF16)
    with F.torch_bf16_path():
        base, _ = F.run_eval(fx, ds, cuda, amp=BF16)
    lines, bad = _bf16_vs_torch(rep, base, ("out", "loss"))
    print(name_eval, "bf16 eval hip/torch:\n  " + "\n  ".join(lines))
    _record("eval_bf16_vs_torch", name_eval, {"lines": lines})
    assert not bad, (bad, lines)


# ------------------------------------------------------------------ c: census
# What the dispatch code sends the bf16 eval forward to (derived from the code, and equal to
# the census of the run):
#   sampling / grouping    ov3d_fps, ball query (scan or cell index), the grouped rows
#   SA modules             SharedMLP.rows (pointnet2_modules.py: sa_fused is training-only):
#                          rows GEMMs, F.batch_norm on running statistics, the neighbour max
#   encoder / decoder      flash attention forward, the fused residual + LayerNorm (+ GEMM)
#                          launches, the Fourier position embedding
#   heads                  per-head GenericMLP rows (heads.supported is training-only), the
#                          unfused _box_predictions
#   SUN launches          fps 2 (pre-encoder, queries), attention 19 (3 encoder + 8 x 2 decoder),
#                          enc_post 3 (one per encoder layer: out-proj + norm2 + FFN), lngemm 24
#                          and rows_gemm_act 26 (the decoder's norm + projection pairs and FFNs,
#                          the projection MLPs), gemm256_pair 1 (the memory's K / V of all 8
#                          layers), fourier_pe 2 (memory, queries)
#   ScanNet, in addition   the interim SA (fps 3, ball query 2, the bf16 group rows, neighbour
#                          max 2, its padded-K rows_gemm products) and the packed radius masks
EVAL_BF16_KERNELS = {
    "sunrgbd": ("ov3d_fps", "ov3d_ball_query_cells", "ov3d_group_fwd", "ov3d_nbr_max_fwd",
                "ov3d_fourier_pe", "ov3d_add_cast_bf16", "ov3d_attn_fwd_masked", "ov3d_enc_post_fwd",
                "ov3d_lngemm_fwd", "ov3d_resnorm_fwd", "ov3d_relu_dropout_fwd", "ov3d_rows_gemm_act",
                "ov3d_tile_gemm", "ov3d_gemm256", "ov3d_gemm256_pair"),
    "scannet": ("ov3d_fps", "ov3d_ball_query_cells", "ov3d_group_fwd", "ov3d_group_rows_bf16",
                "ov3d_nbr_max_fwd", "ov3d_fourier_pe", "ov3d_add_cast_bf16", "ov3d_attn_fwd_masked",
                "ov3d_attn_mask_pack", "ov3d_enc_post_fwd", "ov3d_lngemm_fwd", "ov3d_resnorm_fwd",
                "ov3d_relu_dropout_fwd", "ov3d_rows_gemm", "ov3d_rows_gemm_act", "ov3d_tile_gemm",
                "ov3d_gemm256", "ov3d_gemm256_pair"),
}
# either form counts
EVAL_ALT = {"ov3d_ball_query_cells": ("ov3d_ball_query",),
            "ov3d_attn_fwd_masked": ("ov3d_attn_fwd", "ov3d_attn_fwd_pregen")}
TRAIN_ONLY_PARTS = ("_bwd", "wgrad", "adamw")
TRAIN_ONLY = ("ov3d_attn_dropgen", "ov3d_bn_stats_finalize", "ov3d_seed_next")


@pytest.mark.parametrize("name,name_eval,ds", F.EVAL_CASES)
def test_bf16_eval_census(cuda, name, name_eval, ds):
    from ov3d_amd import _native, gemm
    fx = F.eval_fixture(name, name_eval)
    model, _, _ = F.build(fx, cuda, ds, train=False)
    batch = F.eval_batch(fx, cuda)
    _native.census_start()
    try:
        F.eval_forward(model, batch, BF16)
        torch.cuda.synchronize()
    finally:
        called = _native.census_stop()
    ran = sorted(k for k, n in called.items() if n)
    print(name_eval, "bf16 eval census:", {k: called[k] for k in ran})
    _record("eval_bf16_census", name_eval, {"census": {k: called[k] for k in ran}})
    missing = [k for k in EVAL_BF16_KERNELS[ds]
               if not any(called.get(x) for x in (k,) + EVAL_ALT.get(k, ()))]
    assert not missing, (missing, ran)
    train_only = [k for k in ran if any(p in k for p in TRAIN_ONLY_PARTS) or k in TRAIN_ONLY
                  or k.startswith("ov3d_sa_dy")]
    assert not train_only, train_only
    assert not gemm._PENDING and not gemm._PENDING_COLS
    assert not [n for n, p in model.named_parameters() if p.grad is not None]


# ------------------------------------------------------------------ d: eval mutates nothing
@pytest.mark.parametrize("name,name_eval,ds", F.EVAL_CASES)
def test_eval_forward_mutates_no_state(cuda, name, name_eval, ds):
    fx = F.eval_fixture(name, name_eval)
    model, _, _ = F.build(fx, cuda, ds, train=False)
    batch = F.eval_batch(fx, cuda)
    snap = {k: v.detach().clone() for k, v in model.state_dict().items()}
    assert any(k.endswith("num_batches_tracked") for k in snap)
    for amp in (None, BF16):
        F.eval_forward(model, batch, amp)
        now = model.state_dict()
        assert set(now) == set(snap)
        changed = [k for k in snap if not torch.equal(now[k], snap[k])]
        assert not changed, (amp, changed)


# ------------------------------------------------------------------ e: dropout is inert
@pytest.mark.parametrize("name,name_eval,ds", F.EVAL_CASES)
def test_bf16_eval_is_a_function_of_the_input(cuda, name, name_eval, ds):
    from ov3d_amd import attention
    fx = F.eval_fixture(name, name_eval)
    args = fixture_args(fx)
    assert args.enc_dropout > 0 and args.dec_dropout > 0 and args.mlp_dropout > 0
    model, _, _ = F.build(fx, cuda, ds, train=False)
    batch = F.eval_batch(fx, cuda)
    a = F.eval_forward(model, batch, BF16)
    attention.next_step(cuda)          # the seed moves: a live dropout would draw another mask
    b = F.eval_forward(model, batch, BF16)
    _assert_bit_equal(a, b)
    args0 = argparse.Namespace(**{**vars(args), "enc_dropout": 0.0, "dec_dropout": 0.0,
                                  "mlp_dropout": 0.0})
    plain, _, _ = F.build(fx, cuda, ds, train=False, args=args0)
    _assert_bit_equal(a, F.eval_forward(plain, batch, BF16))


# ------------------------------------------------------------------ f: no_grad changes no value
@pytest.mark.parametrize("amp", AMPS)
@pytest.mark.parametrize("name,name_eval,ds", F.EVAL_CASES)
def test_no_grad_changes_no_value(cuda, name, name_eval, ds, amp):
    from ov3d_amd import gemm
    fx = F.eval_fixture(name, name_eval)
    model, _, _ = F.build(fx, cuda, ds, train=False)
    batch = F.eval_batch(fx, cuda)
    a = F.eval_forward(model, batch, amp, no_grad=True)
    b = F.eval_forward(model, batch, amp, no_grad=False)
    assert b["outputs"]["box_corners"].requires_grad and not a["outputs"]["box_corners"].requires_grad
    _assert_bit_equal(a, {"outputs": {k: v.detach() for k, v in b["outputs"].items()},
                          "aux_outputs": [{k: v.detach() for k, v in lay.items()}
                                          for lay in b["aux_outputs"]]})
    assert not gemm._PENDING


# ------------------------------------------------------------------ g: one scene alone
@pytest.mark.parametrize("name,name_eval,ds", F.EVAL_CASES)
def test_one_scene_alone(cuda, name, name_eval, ds):
    """B = 1, the usual inference batch (2048 encoder rows, 128 / 256 decoder rows per layer),
    against scene 1's rows of the fixture: the reference's B = 1 run equals them (b1_vs_b2)"""
    torch.backends.cuda.matmul.allow_tf32 = False
    fx = F.eval_fixture(name, name_eval)
    assert float(fx["b1_vs_b2"]) <= 1e-12
    model, _, _ = F.build(fx, cuda, ds, train=False)
    rep, _ = F.run_eval(fx, ds, cuda, scenes=[1], model=model)
    bad = _fp32_bad(rep, fx)
    print(name_eval, "B = 1 fp32 worst:", F.worst(rep, "out"))
    _record("eval_fp32_b1", name_eval, {"worst": F.worst(rep, "out"), "over_bar": bad})
    assert not bad, bad
    rep, _ = F.run_eval(fx, ds, cuda, amp=BF16, scenes=[1], model=model)
    with F.torch_bf16_path():
        base, _ = F.run_eval(fx, ds, cuda, amp=BF16, scenes=[1], model=model)
    lines, bad = _bf16_vs_torch(rep, base, ("out",))
    print(name_eval, "B = 1 bf16 hip/torch:\n  " + "\n  ".join(lines))
    _record("eval_bf16_vs_torch_b1", name_eval, {"lines": lines})
    assert not bad, (bad, lines)


# ------------------------------------------------------------------ h: a second checkpoint
CHANGED_PARAM = "decoder.layers.3.linear1.weight"


@pytest.mark.parametrize("name,name_eval,ds", F.EVAL_CASES)
def test_second_checkpoint_in_one_process(cuda, name, name_eval, ds):
    """the bf16 weight copies (gemm.cast_param) follow load_state_dict and an in-place change"""
    fx = F.eval_fixture(name, name_eval)
    model, _, _ = F.build(fx, cuda, ds, train=False)
    batch = F.eval_batch(fx, cuda)
    first = F.eval_forward(model, batch, BF16)
    seed2 = int(fx["seed"]) + 1
    # another seed's det_init values, buffers included (its fresh running statistics)
    fresh, _, _ = F.build(fx, cuda, ds, train=False, seed=seed2, load_bn=False)
    model.load_state_dict({k: v.detach().clone() for k, v in fresh.state_dict().items()})
    second = F.eval_forward(model, batch, BF16)
    assert not torch.equal(first["outputs"]["box_corners"], second["outputs"]["box_corners"])
    _assert_bit_equal(second, F.eval_forward(fresh, batch, BF16))
    # one parameter changed in place
    fresh2, _, _ = F.build(fx, cuda, ds, train=False, seed=seed2, load_bn=False)
    with torch.no_grad():
        for m in (model, fresh2):
            dict(m.named_parameters())[CHANGED_PARAM].mul_(1.5)
    third = F.eval_forward(model, batch, BF16)
    assert not torch.equal(third["outputs"]["box_corners"], second["outputs"]["box_corners"])
    _assert_bit_equal(third, F.eval_forward(fresh2, batch, BF16))


# ------------------------------------------------------------------ i: into the AP calculator
@pytest.mark.parametrize("name,name_eval,ds", F.EVAL_CASES)
def test_eval_outputs_into_ap_calculator(cuda, name, name_eval, ds):
    """the fp32 eval outputs of both scenes through the device AP calculator and, copied to the
    host, through the oracle's restatement of the reference evaluation (the default config of
    evaluate()): identical inputs, so the bars of test_evaldet_gpu.py.  Real overlapping
    predictions: NMS must keep and suppress >= 10 % of the boxes each.  (Empty-box removal is
    not claimed here; it stays with test_evaldet_gpu.py.)"""
    from oracle import evaldet_ref as E
    from ov3d_amd import ap_calculator as apc
    torch.backends.cuda.matmul.allow_tf32 = False
    fx = F.eval_fixture(name, name_eval)
    model, cfg, _ = F.build(fx, cuda, ds, train=False)
    batch = F.eval_batch(fx, cuda)
    out = F.eval_forward(model, batch)["outputs"]
    calc = apc.APCalculator(cfg, ap_iou_thresh=[0.25, 0.5], class2type_map=None, exact_eval=True)
    calc.step(out["box_corners"], out["sem_cls_prob"], out["objectness_prob"], batch["point_clouds"],
              batch["gt_box_corners"], batch["gt_box_sem_cls_label"], batch["gt_box_present"])
    got = calc.compute_metrics()
    h = lambda t: t.detach().cpu().numpy()   # noqa: E731
    corners, probs, obj = h(out["box_corners"]), h(out["sem_cls_prob"]), h(out["objectness_prob"])
    conf = calc.ap_config_dict
    assert conf["remove_empty_box"] and conf["use_3d_nms"] and conf["per_class_proposal"]
    ref_scores = E.detections(corners, probs, obj, h(batch["point_clouds"]), conf, cfg.num_semcls)
    B, Q = obj.shape
    kept = int(np.isfinite(ref_scores).any(-1).sum())
    print(name_eval, "oracle kept", kept, "of", B * Q)
    assert 0.1 * B * Q <= kept <= 0.9 * B * Q, (kept, B * Q)
    sc = h(calc._scores[0])
    assert np.array_equal(np.isfinite(sc).any(-1), np.isfinite(ref_scores).any(-1))
    assert np.array_equal(sc.view(np.uint32), ref_scores.view(np.uint32))
    ref = E.compute_metrics(ref_scores, corners, h(batch["gt_box_corners"]),
                            h(batch["gt_box_sem_cls_label"]), h(batch["gt_box_present"]), [0.25, 0.5])
    for th, d in got.items():
        assert set(d) == set(ref[th]), set(d) ^ set(ref[th])
        for k, v in d.items():
            if k == "mAP":
                assert np.float32(v) == np.float32(ref[th][k]), (th, v, ref[th][k])
            else:
                assert abs(float(v) - float(ref[th][k])) <= 1e-12, (th, k, v, ref[th][k])
