"""Generate the golden parity fixtures from the REFERENCE code (run here, where
/root/reference exists; the outputs are committed and travel to the GPU box).

    python tests/golden/make_golden.py

Fixtures (tests/golden/*.npz):
  giou.npz        reference generalized_box3d_iou: Cython path (box_util.py:624-714,
                  compiled box_intersection.pyx) and TorchScript path (517-618),
                  rotated / axis-aligned, nums in {1,4,5,40,64}; plus d(sum(G*giou))/dcorners1
                  of the TorchScript axis-aligned path (autograd).
  nms.npz         reference nms_3d_faster_samecls / nms_3d_faster (utils/nms.py) picks on
                  tie-free scores, K in {8, 128, 256}, old_type both.
  geometry.npz    reference box_parametrization_to_corners (sunrgbd.py:145-148) and
                  project_box_3d_cuda + clamp (image_util.py:117-134, criterion.py:383-391).
  model_sun.npz   reference Model3DETR (vanilla encoder, SUN config, reduced widths) +
                  SetCriterion with a fixed fake RegionCLIP: state dict, inputs, outputs of all
                  decoder layers, the 56-entry loss dict, parameter gradients.  The un-vendored
                  pointnet2 is the oracle restatement (oracle/pointnet2_ref.py).
  model_scannet.npz  same for the masked encoder + colour + ScanNet config + differentiable GIoU.
  model_{sun,scannet}_full.npz  the float64 reference at the HIP kernels' real shapes
                  (run_model_fixture_full).
  model_{sun,scannet}_eval.npz (+ .pN.npz parts)  its eval-mode twin: model.eval() under
                  no_grad with the reference's dropouts on and running statistics far from
                  the batch's own (run_model_fixture_eval); inputs / text / seed are the _full
                  file's.
"""
import argparse
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

from ref_loader import load_reference  # noqa: E402
from fake_clip import FakeRegionCLIP  # noqa: E402
import ov3d_import  # noqa: E402

ov3d = ov3d_import.load()
from ov3d_amd import synthetic  # noqa: E402


def rand_boxes(rs, cfg, B, K, rotated=True):
    c = torch.tensor(rs.uniform([-2, 1, -0.5], [2, 5, 1.5], (B, K, 3)), dtype=torch.float32)
    s = torch.tensor(rs.uniform(0.3, 2.0, (B, K, 3)), dtype=torch.float32)
    a = torch.tensor(rs.uniform(-np.pi, np.pi, (B, K)) if rotated else np.zeros((B, K)),
                     dtype=torch.float32)
    return c, s, a, cfg.box_parametrization_to_corners(c, s, a)


def gen_giou(R):
    bu = R["box_util"]
    cfg = R["sunrgbd"].SunrgbdDatasetConfig()
    rs = np.random.RandomState(1234)
    B, K1, K2 = 5, 32, 64
    out = {}
    for tag, rot in (("rot", True), ("aligned", False)):
        _, _, _, c1 = rand_boxes(rs, cfg, B, K1, rot)
        _, _, _, c2 = rand_boxes(rs, cfg, B, K2, rot)
        c2[:, :12] = c1[:, :12] + torch.tensor(rs.uniform(-0.2, 0.2, (B, 12, 1, 3)), dtype=torch.float32)
        nums = torch.tensor([1, 4, 5, 40, 64])
        out[f"{tag}_c1"] = c1.numpy()
        out[f"{tag}_c2"] = c2.numpy()
        out[f"{tag}_nums"] = nums.numpy().astype(np.int32)
        for rflag in (True, False):
            key = f"{tag}_{'r' if rflag else 'a'}"
            out[key + "_cython"] = bu.generalized_box3d_iou(c1, c2, nums, rotated_boxes=rflag,
                                                            needs_grad=False).numpy()
            out[key + "_tensor"] = bu.generalized_box3d_iou_tensor_jit(c1, c2, nums, rflag, False).numpy()
    # autograd of the differentiable axis-aligned path
    _, _, _, c1 = rand_boxes(rs, cfg, 3, 16, False)
    _, _, _, c2 = rand_boxes(rs, cfg, 3, 8, False)
    c2[:, :6] = c1[:, :6] + torch.tensor(rs.uniform(-0.3, 0.3, (3, 6, 1, 3)), dtype=torch.float32)
    nums = torch.tensor([8, 3, 6])
    G = torch.tensor(rs.randn(3, 16, 8), dtype=torch.float32)
    c1g = c1.clone().requires_grad_(True)
    g = bu.generalized_box3d_iou(c1g, c2, nums, rotated_boxes=False, needs_grad=True)
    (g * G).sum().backward()
    out.update(grad_c1=c1.numpy(), grad_c2=c2.numpy(), grad_nums=nums.numpy().astype(np.int32),
               grad_G=G.numpy(), grad_giou=g.detach().numpy(), grad_dc1=c1g.grad.numpy())
    # autograd of the differentiable ROTATED path (box_util.py:579-600: the Sutherland-Hodgman
    # clip on tensors, differentiated through every intersection vertex)
    _, _, _, c1 = rand_boxes(rs, cfg, 2, 12, True)
    _, _, _, c2 = rand_boxes(rs, cfg, 2, 9, True)
    c2[:, :8] = c1[:, :8] + torch.tensor(rs.uniform(-0.25, 0.25, (2, 8, 1, 3)), dtype=torch.float32)
    nums = torch.tensor([9, 6])
    G = torch.tensor(rs.randn(2, 12, 9), dtype=torch.float32)
    c1g = c1.clone().requires_grad_(True)
    g = bu.generalized_box3d_iou(c1g, c2, nums, rotated_boxes=True, needs_grad=True)
    (g * G).sum().backward()
    out.update(rgrad_c1=c1.numpy(), rgrad_c2=c2.numpy(), rgrad_nums=nums.numpy().astype(np.int32),
               rgrad_G=G.numpy(), rgrad_giou=g.detach().numpy(), rgrad_dc1=c1g.grad.numpy())
    np.savez_compressed(os.path.join(HERE, "giou.npz"), **out)


def gen_nms(R):
    nms = R["nms"]
    rs = np.random.RandomState(77)
    out = {}
    for i, K in enumerate((8, 128, 256)):
        lo = rs.uniform(-3, 3, (K, 3))
        sz = rs.uniform(0.2, 1.5, (K, 3))
        boxes = np.zeros((K, 8))
        boxes[:, 0:3] = lo
        boxes[:, 3:6] = lo + sz
        boxes[:, 6] = rs.permutation(K) / K + rs.uniform(0, 1e-4, K)  # tie-free
        boxes[:, 7] = rs.randint(0, 4, K)
        out[f"boxes{i}"] = boxes
        for old in (False, True):
            out[f"samecls{i}_{int(old)}"] = np.array(nms.nms_3d_faster_samecls(boxes, 0.25, old), np.int32)
            out[f"any{i}_{int(old)}"] = np.array(nms.nms_3d_faster(boxes[:, :7], 0.25, old), np.int32)
    np.savez_compressed(os.path.join(HERE, "nms.npz"), **out)


def gen_geometry(R):
    cfg = R["sunrgbd"].SunrgbdDatasetConfig()
    iu = R["image_util"]
    rs = np.random.RandomState(5)
    c, s, a, corners = rand_boxes(rs, cfg, 2, 16, True)
    Rtilt = torch.tensor(np.array([[0.99, 0.05, 0.1], [-0.05, 0.99, 0.0], [-0.1, 0.0, 0.99]]),
                         dtype=torch.float32)
    K = torch.tensor([[529.5, 0, 365.0], [0, 529.5, 265.0], [0, 0, 1]], dtype=torch.float32)
    c_img = c.clone()
    c_img[..., 1] += 2.0  # in front of the camera
    boxes2d = []
    for b in range(2):
        calib = iu.SUNRGBD_Calibration_cuda(Rtilt, K)
        bx = iu.project_box_3d_cuda(calib, c_img[b], s[b], a[b])
        mx = torch.broadcast_to(torch.tensor([[730, 530, 730, 530]]), bx.size())
        boxes2d.append(torch.minimum(torch.clamp_min(bx, 0), mx))
    np.savez_compressed(os.path.join(HERE, "geometry.npz"), center=c.numpy(), size=s.numpy(),
                        angle=a.numpy(), corners=corners.numpy(), center_img=c_img.numpy(),
                        Rtilt=Rtilt.numpy(), K=K.numpy(), boxes2d=torch.stack(boxes2d).numpy())


MODEL_KEYS = ("box_corners", "sem_cls_logits", "visual_embeds", "center_normalized", "size_normalized",
              "angle_logits", "angle_residual_normalized", "objectness_prob", "sem_cls_prob",
              "angle_continuous", "center_unnormalized", "size_unnormalized")
GRAD_PARAMS = ("pre_encoder.mlp_module.layer0.conv.weight", "pre_encoder.mlp_module.layer2.bn.bn.weight",
               "encoder.layers.0.self_attn.in_proj_weight", "encoder.layers.2.linear2.weight",
               "encoder_to_decoder_projection.layers.0.weight", "query_projection.layers.0.weight",
               "decoder.layers.0.multihead_attn.in_proj_weight", "decoder.layers.7.linear1.weight",
               "decoder.norm.weight", "mlp_heads.visual_embed_head.layers.0.weight",
               "mlp_heads.center_head.layers.8.weight", "mlp_heads.angle_cls_head.layers.8.bias",
               "mlp_heads.size_head.layers.4.weight")


def model_args(**kw):
    a = dict(model_name="3detr", enc_type="vanilla", enc_nlayers=3, enc_dim=64, enc_ffn_dim=64,
             enc_dropout=0.0, enc_nhead=4, enc_activation="relu", dec_nlayers=8, dec_dim=64,
             dec_ffn_dim=64, dec_dropout=0.0, dec_nhead=4, mlp_dropout=0.0, preenc_npoints=256,
             nqueries=32, use_color=False, matcher_giou_cost=3.0, matcher_cls_cost=1.0,
             matcher_center_cost=5.0, matcher_objectness_cost=5.0, loss_giou_weight=0.0,
             loss_sem_cls_weight=1.0, loss_no_object_weight=0.1, loss_angle_cls_weight=0.1,
             loss_angle_reg_weight=0.5, loss_center_weight=5.0, loss_size_weight=1.0,
             loss_2dalignment_weight=2e-4)
    a.update(kw)
    return argparse.Namespace(**a)


def small_images(batch, B, H=24, W=32):
    rs = np.random.RandomState(3)
    batch["image"] = torch.tensor(rs.uniform(0, 255, (B, H * W * 3)), dtype=torch.float32)
    batch["image_height"] = torch.full((B,), H, dtype=torch.int64)
    batch["image_width"] = torch.full((B,), W, dtype=torch.int64)
    batch["calib_Rtilt"] = torch.eye(3).repeat(B, 1, 1)
    f = 529.5 * W / 730
    batch["calib_K"] = torch.tensor([[f, 0, W / 2], [0, f, H / 2], [0, 0, 1]], dtype=torch.float32).repeat(B, 1, 1)
    return batch


def run_model_fixture(R, name, args, cfg, batch, text):
    tmp = tempfile.mkdtemp()
    args.clip_embed_path = os.path.join(tmp, "text.pth")
    torch.save(text, args.clip_embed_path)
    torch.manual_seed(2024)
    model, _ = R["model_3detr"].build_3detr(args, cfg)
    model.train()
    sd = {k: v.detach().clone().numpy() for k, v in model.state_dict().items()}
    inputs = {"point_clouds": batch["point_clouds"], "point_cloud_dims_min": batch["point_cloud_dims_min"],
              "point_cloud_dims_max": batch["point_cloud_dims_max"]}
    out = model(inputs)
    crit = R["criterion"].build_criterion(args, cfg)
    clip = FakeRegionCLIP()
    targets = dict(batch)
    # record the reference matcher's assignments and costs (one call per decoder layer:
    # final output first, then aux 0..L-2) so tests can pin matching separately from the
    # gradient check: near-tie costs of a random-init model flip under 1e-6 noise
    rec = []
    orig_fwd = crit.matcher.forward

    def recording_forward(outputs, targets):
        res = orig_fwd(outputs, targets)
        rec.append((res["per_prop_gt_inds"].numpy().copy(), res["proposal_matched_mask"].numpy().copy()))
        return res
    crit.matcher.forward = recording_forward
    loss, ld = crit(out, targets, clip=clip)
    loss.backward()
    named = dict(model.named_parameters())
    fx = {"sd/" + k: v for k, v in sd.items()}
    fx.update({"in/" + k: v.numpy() for k, v in batch.items()})
    layers = [out["outputs"]] + out["aux_outputs"]
    for li, lay in enumerate(layers):
        for k in MODEL_KEYS:
            if k == "visual_embeds" and li not in (0, len(layers) - 1):
                continue  # 640-d rows: keep the fixture small (pinned by the alignment loss anyway)
            fx[f"out/{li}/{k}"] = lay[k].detach().numpy()
    fx["loss"] = np.float32(loss.item())
    for k, v in ld.items():
        fx["ld/" + k] = np.float32(v.item())
    for p in GRAD_PARAMS:
        if p in named and named[p].grad is not None:
            fx["grad/" + p] = named[p].grad.numpy()
    fx["match_inds"] = np.stack([r[0] for r in rec])
    fx["match_mask"] = np.stack([r[1] for r in rec])
    fx["text"] = text.numpy()
    fx["args"] = np.array(repr(sorted(vars(args).items())))
    np.savez_compressed(os.path.join(HERE, name), **fx)
    print(name, "loss", loss.item(), "keys", len(ld), "clip calls", clip.calls)


def gen_model_sun(R):
    cfg = R["sunrgbd"].SunrgbdDatasetConfig()
    batch = synthetic.make_batch(2, seed=5, num_points=2048)
    batch = small_images(batch, 2)
    run_model_fixture(R, "model_sun.npz", model_args(), cfg, batch, synthetic.text_embedding(21, 640))


def gen_model_scannet(R):
    import datasets.scannet as scannet  # reference module (stubs installed by load_reference)
    cfg = scannet.ScannetDatasetConfig()
    batch = synthetic.make_batch(2, seed=9, num_points=4096, use_color=True)
    # ScanNet boxes are axis aligned: zero every angle and rebuild the corners
    B = 2
    batch["gt_box_angles"].zero_()
    batch["gt_angle_class_label"].zero_()
    batch["gt_angle_residual_label"].zero_()
    batch["gt_box_sem_cls_label"].clamp_(max=17)
    corners = cfg.box_parametrization_to_corners_np(batch["gt_box_centers"].numpy(),
                                                   batch["gt_box_sizes"].numpy(),
                                                   np.zeros((B, 64), np.float32))
    batch["gt_box_corners"] = torch.tensor(corners, dtype=torch.float32)
    batch = small_images(batch, B)
    args = model_args(enc_type="masked", use_color=True, preenc_npoints=512, nqueries=64,
                      matcher_giou_cost=2.0, matcher_center_cost=0.0, matcher_objectness_cost=0.0,
                      loss_giou_weight=1.0, loss_no_object_weight=0.25, loss_2dalignment_weight=0.0)
    run_model_fixture(R, "model_scannet.npz", args, cfg, batch, synthetic.text_embedding(19, 640, seed=8))


# ------------------------------------------------------------------ full-shape fixtures
# The HIP kernels' real shapes (enc / dec 256, 4 heads = head_dim 64, preenc 2048, 128 / 256
# queries, 20000 points): the bf16 fused SA, flash attention, heads-rows, rows-GEMM and
# set-loss kernels only run at these shapes.  The reference runs in FLOAT64 (model, inputs
# and criterion; the pointnet2 index restatement works on the float32 coordinates, as the
# upstream CUDA kernels do), so the fixture is the reference's exact answer and the fp32
# product is held to 1e-3 against it.  Weights: det_init (seeded by state-dict name), not
# stored.
FULL_GRAD_SLICE = 32            # rows of each large gradient stored in full
# gradients whose float64 norm is below GRAD_FLOOR x the total gradient norm are structurally
# zero (e.g. a LayerNorm bias followed by a linear layer and batch-statistics BatchNorm: the
# shift cancels); errors are measured against max(|g|, GRAD_FLOOR x total)
GRAD_FLOOR = 1e-6
# float32 reference runs whose worst error (per entry) is recorded: one on the fixture's
# weights, N_JITTER with every weight moved by <= JITTER_REL (an fp32 implementation that only
# differs in rounding is one more such run: ReLU masks / max-pool winners at ~0 margins flip)
N_JITTER = 6
# the jitter's size: 4 ulp (2^-21 relative), so the jittered runs' forward error against
# float64 (~1e-5 on the head outputs) matches an fp32 implementation with a different
# accumulation order (the product's measured forward error), not just a re-run
JITTER_REL = 2.0 ** -21
# gradients stored element-wise (first FULL_GRAD_SLICE rows when large): one or two per
# stage of the step; every other parameter is pinned by its norm and <grad, probe>
FULL_GRAD_PARAMS = GRAD_PARAMS + (
    "pre_encoder.mlp_module.layer1.conv.weight", "pre_encoder.mlp_module.layer2.conv.weight",
    "encoder.layers.0.linear1.weight", "encoder.layers.1.self_attn.out_proj.weight",
    "encoder.layers.2.norm2.weight", "decoder.layers.0.self_attn.in_proj_weight",
    "decoder.layers.3.multihead_attn.out_proj.weight", "decoder.layers.7.linear2.weight",
    "mlp_heads.sem_cls_head.bias", "mlp_heads.objectness_head.layers.0.weight",
    "encoder.interim_downsampling.mlp_module.layer0.conv.weight")


def _ref_pass(R, args, cfg, batch32, seed, dtype, replay=None, jitter=None):
    """one reference forward + criterion + backward in `dtype` with det_init weights;
    replay: matcher results of an earlier pass to hand back instead of solving;
    jitter: seed of a JITTER_REL relative perturbation of every weight"""
    import det_init
    model, _ = R["model_3detr"].build_3detr(args, cfg)
    model = model.to(dtype).train()
    filled = det_init.fill_(model, seed)
    if jitter is not None:
        g = torch.Generator().manual_seed(jitter)
        with torch.no_grad():
            for p in model.parameters():
                if p.requires_grad:
                    p.mul_(1 + JITTER_REL * (2 * torch.rand(p.shape, generator=g) - 1).to(p.dtype))
    batch = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in batch32.items()}
    inputs = {k: batch[k] for k in ("point_clouds", "point_cloud_dims_min", "point_cloud_dims_max")}
    clip = FakeRegionCLIP()          # float32 weights, made before a float64 default
    torch.set_default_dtype(dtype)
    # the reference projects the 2D boxes in float32 whatever the box dtype
    # (SUNRGBD_Calibration_cuda casts Rtilt / K with .float(), image_util.py:276-277): hand it
    # float32 boxes, as the fp32 model gives it, instead of failing on the float64 ones
    proj = R["criterion"].project_box_3d_cuda
    R["criterion"].project_box_3d_cuda = lambda calib, c, s, a: proj(calib, c.float(), s.float(),
                                                                       a.float())
    try:
        out = model(inputs)
        crit = R["criterion"].build_criterion(args, cfg)
        rec = []
        orig_fwd = crit.matcher.forward

        def recording_forward(outputs, targets):
            res = replay[len(rec)] if replay is not None else orig_fwd(outputs, targets)
            rec.append(res)
            return res
        crit.matcher.forward = recording_forward
        loss, ld = crit(out, dict(batch), clip=clip)
        loss.backward()
    finally:
        torch.set_default_dtype(torch.float32)
        R["criterion"].project_box_3d_cuda = proj
    grads = {n: p.grad.double().numpy() for n, p in model.named_parameters() if p.grad is not None}
    return dict(out=[out["outputs"]] + out["aux_outputs"], loss=loss.item(),
                ld={k: v.item() for k, v in ld.items()}, grads=grads, rec=rec, filled=filled,
                clip_calls=clip.calls)


def _rel(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def run_model_fixture_full(R, name, args, cfg, batch32, text, seed):
    """the float64 reference pass is the fixture; float32 passes of the same reference code
    on the same inputs / matching (weights as is and jittered by JITTER_REL) record the reference's
    OWN fp32 error envelope against it (ref32err/..., max over the runs): where conditioning
    (a max-pool winner or ReLU mask that flips under 1e-7 noise) moves a gradient, the
    reference's fp32 CPU path moves it too, and the tests hold the product to
    max(1e-3, 2 x that)"""
    import det_init as di
    tmp = tempfile.mkdtemp()
    args.clip_embed_path = os.path.join(tmp, "text.pth")
    torch.save(text, args.clip_embed_path)
    r64 = _ref_pass(R, args, cfg, batch32, seed, torch.float64)
    r32s = [_ref_pass(R, args, cfg, batch32, seed, torch.float32, replay=r64["rec"], jitter=j)
            for j in (None,) + tuple(range(1, N_JITTER + 1))]
    fx = {"in/" + k: v.numpy() for k, v in batch32.items()}
    fx["seed"] = np.int64(seed)
    fx["filled"] = np.array(r64["filled"])
    fx["n_ref32_runs"] = np.int64(len(r32s))
    for li, lay in enumerate(r64["out"]):
        for k in MODEL_KEYS:
            if k == "visual_embeds" and li != 0:
                continue
            ref = lay[k].detach().numpy()
            fx[f"out/{li}/{k}"] = ref.astype(np.float32)
            fx[f"ref32err/out/{li}/{k}"] = np.float64(max(
                _rel(r["out"][li][k].detach().numpy(), ref) for r in r32s))
    fx["loss"] = np.float64(r64["loss"])
    fx["ref32err/loss"] = np.float64(max(abs(r["loss"] - r64["loss"]) for r in r32s) / abs(r64["loss"]))
    for k, v in r64["ld"].items():
        fx["ld/" + k] = np.float64(v)
        fx["ref32err/ld/" + k] = np.float64(max(abs(r["ld"][k] - v) for r in r32s) / max(abs(v), 1e-3))
    total = np.sqrt(sum(float(np.linalg.norm(g)) ** 2 for g in r64["grads"].values()))
    fx["gradtotal"] = np.float64(total)
    for n, g in r64["grads"].items():
        g32s = [r["grads"][n] for r in r32s]
        nrm = float(np.linalg.norm(g))
        floor = max(nrm, GRAD_FLOOR * total)
        fx["gradnorm/" + n] = np.float64(nrm)
        pr = di.probe(n, g.shape)
        p64 = (g * pr).sum()
        fx["gradproj/" + n] = np.float64(p64)
        fx["ref32err/gradnorm/" + n] = np.float64(max(abs(np.linalg.norm(x) - nrm) for x in g32s) / floor)
        fx["ref32err/gradproj/" + n] = np.float64(max(abs((x * pr).sum() - p64) for x in g32s) / floor)
        if n in FULL_GRAD_PARAMS or (g.size <= 4096 and n.startswith(("pre_encoder", "mlp_heads"))):
            cut = (lambda a: a) if g.size <= 32768 else (lambda a: a[:FULL_GRAD_SLICE])
            sl = cut(g)
            fx["grad/" + n] = sl.astype(np.float32)
            fx["ref32err/grad/" + n] = np.float64(max(np.abs(cut(x) - sl).max() for x in g32s) /
                                                 max(np.abs(sl).max(), GRAD_FLOOR * total))
    fx["match_inds"] = np.stack([r["per_prop_gt_inds"].numpy() for r in r64["rec"]])
    fx["match_mask"] = np.stack([r["proposal_matched_mask"].numpy() for r in r64["rec"]])
    fx["text"] = text.numpy()
    fx["args"] = np.array(repr(sorted((k, v) for k, v in vars(args).items() if k != "clip_embed_path")))
    np.savez_compressed(os.path.join(HERE, name), **fx)
    worst = sorted(((float(v), k) for k, v in fx.items() if k.startswith("ref32err/")), reverse=True)
    print(name, "loss", r64["loss"], "keys", len(r64["ld"]), "clip calls", r64["clip_calls"],
          "size", os.path.getsize(os.path.join(HERE, name)), "ref fp32 worst", worst[:6])


def gen_model_sun_full(R):
    cfg = R["sunrgbd"].SunrgbdDatasetConfig()
    batch = synthetic.make_batch(2, seed=21, num_points=20000)
    batch = small_images(batch, 2)
    args = model_args(enc_dim=256, enc_ffn_dim=128, dec_dim=256, dec_ffn_dim=256,
                      preenc_npoints=2048, nqueries=128)
    run_model_fixture_full(R, "model_sun_full.npz", args, cfg, batch,
                           synthetic.text_embedding(21, 640), seed=31)


def gen_model_scannet_full(R):
    import datasets.scannet as scannet
    cfg = scannet.ScannetDatasetConfig()
    B = 2
    batch = synthetic.make_batch(B, seed=23, num_points=20000, use_color=True, dataset="scannet")
    batch["gt_box_angles"].zero_()
    batch["gt_angle_class_label"].zero_()
    batch["gt_angle_residual_label"].zero_()
    batch["gt_box_sem_cls_label"].clamp_(max=17)
    corners = cfg.box_parametrization_to_corners_np(batch["gt_box_centers"].numpy(),
                                                   batch["gt_box_sizes"].numpy(),
                                                   np.zeros((B, 64), np.float32))
    batch["gt_box_corners"] = torch.tensor(corners, dtype=torch.float32)
    batch = small_images(batch, B)
    args = model_args(enc_type="masked", use_color=True, enc_dim=256, enc_ffn_dim=128, dec_dim=256,
                      dec_ffn_dim=256, preenc_npoints=2048, nqueries=256, matcher_giou_cost=2.0,
                      matcher_center_cost=0.0, matcher_objectness_cost=0.0, loss_giou_weight=1.0,
                      loss_no_object_weight=0.25, loss_2dalignment_weight=0.0)
    run_model_fixture_full(R, "model_scannet_full.npz", args, cfg, batch,
                           synthetic.text_embedding(19, 640, seed=8), seed=37)


# ------------------------------------------------------------------ eval-mode fixtures
# The inference forward (model.eval() under no_grad, as the reference's evaluate() drives it,
# engine.py:154-231) on the inputs, text embedding, seed and det_init weights of the _full
# fixtures (not stored again: the tests read in/*, text, seed and filled from the _full file).
EVAL_STATS_SEED = 99            # synthetic batch the running statistics come from
EVAL_PERTURB_SEED = 4242        # generator of the per-channel perturbation
EVAL_A0, EVAL_B0 = 0.5, 1.0     # first amplitudes: mean += a sqrt(var) u, var *= 2^(b v)
EVAL_BLIND_BAR = 1e-2           # 10 x the fp32 bar (FP32_TOL = 1e-3) per final-layer key
EVAL_B1_TOL = 1e-12             # one scene alone against its rows of the two-scene run
# a committed file stays under 1 MiB: the fixture is written as NAME.npz + NAME.pN.npz, arrays
# above PART_CHUNK split along axis 0 into KEY#i (tests/helpers.py fixture_parts puts them back)
PART_LIMIT = 1 << 20
PART_BUDGET = 900 * 1024
PART_CHUNK = 700 * 1024
INPUT_KEYS = ("point_clouds", "point_cloud_dims_min", "point_cloud_dims_max")


def save_parts(name, fx):
    items = []
    for k, v in fx.items():
        v = np.asarray(v)
        n = -(-v.nbytes // PART_CHUNK)
        if n > 1:
            items += [(f"{k}#{i}", p) for i, p in enumerate(np.array_split(v, n))]
        else:
            items.append((k, v))
    bins = [[]]
    for k, v in sorted(items, key=lambda kv: kv[1].nbytes):      # the small entries in NAME.npz
        if bins[-1] and sum(x.nbytes for _, x in bins[-1]) + v.nbytes > PART_BUDGET:
            bins.append([])
        bins[-1].append((k, v))
    stem = os.path.join(HERE, name[:-4])
    for f in os.listdir(HERE):
        if f.startswith(name[:-4] + ".p") and f.endswith(".npz"):
            os.remove(os.path.join(HERE, f))
    paths = []
    for i, b in enumerate(bins):
        path = stem + (".npz" if i == 0 else f".p{i}.npz")
        np.savez_compressed(path, **dict(b))
        assert os.path.getsize(path) <= PART_LIMIT, (path, os.path.getsize(path))
        paths.append(path)
    return paths


def _bn_buffer_names(model):
    return [k for k in model.state_dict() if k.rsplit(".", 1)[-1] in ("running_mean", "running_var")]


def _ref_forward(R, args, cfg, batch32, seed, dtype, train, bn=None, momentum=None, jitter=None,
                 replay=None, criterion=False, scenes=None):
    """one reference forward under no_grad in `dtype` with det_init weights.
    train: module mode; bn: {state-dict name: float32 array} loaded after det_init;
    momentum: set on every BatchNorm (1.0: the running statistics become this batch's);
    jitter / replay: as _ref_pass; criterion: also the loss dict as evaluate() computes it;
    scenes: rows of the batch to run (None: all)"""
    import det_init
    model, _ = R["model_3detr"].build_3detr(args, cfg)
    model = model.to(dtype)
    det_init.fill_(model, seed)
    sd = model.state_dict(keep_vars=True)
    with torch.no_grad():
        for k, v in (bn or {}).items():
            sd[k].copy_(torch.from_numpy(np.asarray(v)).to(dtype))
        if jitter is not None:
            g = torch.Generator().manual_seed(jitter)
            for p in model.parameters():
                if p.requires_grad:
                    p.mul_(1 + JITTER_REL * (2 * torch.rand(p.shape, generator=g) - 1).to(p.dtype))
    if momentum is not None:
        for m in model.modules():
            if isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
                m.momentum = momentum
    model.train(train)
    batch = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in batch32.items()}
    if scenes is not None:
        batch = {k: v[scenes] for k, v in batch.items()}
    inputs = {k: batch[k] for k in INPUT_KEYS}
    clip = FakeRegionCLIP()
    torch.set_default_dtype(dtype)
    proj = R["criterion"].project_box_3d_cuda
    R["criterion"].project_box_3d_cuda = lambda calib, c, s, a: proj(calib, c.float(), s.float(),
                                                                       a.float())
    res = {}
    try:
        with torch.no_grad():
            torch.manual_seed(0)
            out = model(inputs)
            if criterion:
                crit = R["criterion"].build_criterion(args, cfg)
                rec = []
                orig_fwd = crit.matcher.forward

                def recording_forward(outputs, targets):
                    r = replay[len(rec)] if replay is not None else orig_fwd(outputs, targets)
                    rec.append(r)
                    return r
                crit.matcher.forward = recording_forward
                loss, ld = crit(out, dict(batch), clip=clip)
                res.update(loss=loss.item(), ld={k: v.item() for k, v in ld.items()}, rec=rec)
    finally:
        torch.set_default_dtype(torch.float32)
        R["criterion"].project_box_3d_cuda = proj
    res["out"] = [{k: lay[k].detach().double().numpy() for k in MODEL_KEYS}
                  for lay in [out["outputs"]] + out["aux_outputs"]]
    res["bn"] = {k: model.state_dict()[k].double().numpy().copy() for k in _bn_buffer_names(model)}
    return res


def _perturbed_stats(stats, a, b):
    """mean += a sqrt(var) u, var *= 2^(b v), u, v ~ U(-1, 1) per channel; rounded to float32"""
    g = np.random.RandomState(EVAL_PERTURB_SEED)
    out = {}
    for k in sorted(stats):
        if not k.endswith("running_mean"):
            continue
        kv = k[:-len("running_mean")] + "running_var"
        mean, var = stats[k], stats[kv]
        u = g.uniform(-1, 1, mean.shape)
        v = g.uniform(-1, 1, mean.shape)
        out[k] = (mean + a * np.sqrt(var) * u).astype(np.float32)
        out[kv] = (var * 2.0 ** (b * v)).astype(np.float32)
    return out


def run_model_fixture_eval(R, name, args_full, dropouts, cfg, batch32, stats_batch, text, seed):
    """Eval-mode twin of run_model_fixture_full.

    Running statistics: one train-mode float64 pass of the reference over `stats_batch` (another
    synthetic batch of the same shapes) with every BatchNorm's momentum at 1.0, then perturbed
    per channel (_perturbed_stats) and rounded to float32; stored under bn/ and loaded back into
    the reference before the eval pass.  The amplitudes (a, b) start at (EVAL_A0, EVAL_B0) and
    double until every stored key of the final layer differs between the reference's train-mode
    and eval-mode float64 outputs (same input, same weights) by >= EVAL_BLIND_BAR of its max: a
    product that used batch statistics in eval then misses the fp32 bar 10 times over on every
    key.  The train-mode passes run with the _full args (every dropout 0: the state dict is the
    same, and a train-mode pass with the dropouts on would be a random draw); the eval passes
    run with the dropouts on (enc / dec / mlp), which eval mode must make inert.

    One scene alone: the reference's eval outputs for scene 1 at B = 1 are asserted equal to
    its rows of the B = 2 run within EVAL_B1_TOL (eval BatchNorm is per row, sampling, grouping
    and attention are per scene), so no separate out1/ is stored."""
    tmp = tempfile.mkdtemp()
    args_full.clip_embed_path = os.path.join(tmp, "text.pth")
    torch.save(text, args_full.clip_embed_path)
    args = argparse.Namespace(**{**vars(args_full), **dropouts})
    stats = _ref_forward(R, args_full, cfg, stats_batch, seed, torch.float64, train=True,
                         momentum=1.0)["bn"]
    tr = _ref_forward(R, args_full, cfg, batch32, seed, torch.float64, train=True)["out"]
    a, b = EVAL_A0, EVAL_B0
    while True:
        bn = _perturbed_stats(stats, a, b)
        r64 = _ref_forward(R, args, cfg, batch32, seed, torch.float64, train=False, bn=bn,
                           criterion=True)
        tve = {f"{li}/{k}": _rel(tr[li][k], lay[k]) for li, lay in enumerate(r64["out"])
               for k in MODEL_KEYS if k != "visual_embeds" or li == 0}
        # a key that is identically zero in both modes cannot tell them apart (ScanNet's one
        # angle bin: angle_continuous is angle_logits * 0 + angle_residual * 0, model_3detr.py:45 of
        # the reference); it is listed in the fixture as exempt instead of measured
        exempt = sorted(k for k in MODEL_KEYS if not tr[0][k].any() and not r64["out"][0][k].any())
        tve = {k: v for k, v in tve.items() if k.split("/")[1] not in exempt}
        final = {k: v for k, v in tve.items() if k.startswith("0/")}
        print(name, "a", a, "b", b, "train_vs_eval (final layer):",
              {k: "%.2e" % v for k, v in sorted(final.items())})
        if min(final.values()) >= EVAL_BLIND_BAR:
            break
        assert a < 64, "no amplitude makes every key discriminate"
        a, b = 2 * a, 2 * b
    assert all(v >= EVAL_BLIND_BAR for v in final.values()), final
    for k, v in bn.items():     # the reference kept the float32 values exactly
        assert np.array_equal(r64["bn"][k], v.astype(np.float64)), k
    one = _ref_forward(R, args, cfg, batch32, seed, torch.float64, train=False, bn=bn, scenes=[1])
    b1 = max(_rel(one["out"][li][k][0], lay[k][1]) for li, lay in enumerate(r64["out"])
             for k in MODEL_KEYS)
    print(name, "scene 1 alone vs its B = 2 rows:", b1)
    assert b1 <= EVAL_B1_TOL, b1
    r32s = [_ref_forward(R, args, cfg, batch32, seed, torch.float32, train=False, bn=bn,
                         criterion=True, replay=r64["rec"], jitter=j)
            for j in (None,) + tuple(range(1, N_JITTER + 1))]
    fx = {"bn/" + k: v for k, v in bn.items()}
    fx["perturb_a"] = np.float64(a)
    fx["perturb_b"] = np.float64(b)
    fx["b1_vs_b2"] = np.float64(b1)
    fx["train_vs_eval_exempt"] = np.array(",".join(exempt))
    fx["n_ref32_runs"] = np.int64(len(r32s))
    for k, v in tve.items():
        fx["train_vs_eval/" + k] = np.float64(v)
    for li, lay in enumerate(r64["out"]):
        for k in MODEL_KEYS:
            if k == "visual_embeds" and li != 0:
                continue
            fx[f"out/{li}/{k}"] = lay[k].astype(np.float32)
            fx[f"ref32err/out/{li}/{k}"] = np.float64(max(_rel(r["out"][li][k], lay[k]) for r in r32s))
    fx["loss"] = np.float64(r64["loss"])
    fx["ref32err/loss"] = np.float64(max(abs(r["loss"] - r64["loss"]) for r in r32s) / abs(r64["loss"]))
    for k, v in r64["ld"].items():
        fx["ld/" + k] = np.float64(v)
        fx["ref32err/ld/" + k] = np.float64(max(abs(r["ld"][k] - v) for r in r32s) / max(abs(v), 1e-3))
    fx["match_inds"] = np.stack([r["per_prop_gt_inds"].numpy() for r in r64["rec"]])
    fx["match_mask"] = np.stack([r["proposal_matched_mask"].numpy() for r in r64["rec"]])
    fx["args"] = np.array(repr(sorted((k, v) for k, v in vars(args).items() if k != "clip_embed_path")))
    paths = save_parts(name, fx)
    sizes = [os.path.getsize(p) for p in paths]
    full = os.path.getsize(os.path.join(HERE, name[:-9] + "_full.npz"))
    assert sum(sizes) <= full, (sizes, full)
    worst = sorted(((float(v), k) for k, v in fx.items() if k.startswith("ref32err/")), reverse=True)
    print(name, "loss", r64["loss"], "amplitudes a", a, "b", b, "bn floats",
          sum(v.size for v in bn.values()), "sizes", sizes, "of", full, "ref fp32 worst", worst[:6])


def _sun_full_setup(R):
    cfg = R["sunrgbd"].SunrgbdDatasetConfig()
    args = model_args(enc_dim=256, enc_ffn_dim=128, dec_dim=256, dec_ffn_dim=256,
                      preenc_npoints=2048, nqueries=128)
    return cfg, args


def gen_model_sun_eval(R):
    cfg, args = _sun_full_setup(R)
    batch = small_images(synthetic.make_batch(2, seed=21, num_points=20000), 2)
    stats_batch = synthetic.make_batch(2, seed=EVAL_STATS_SEED, num_points=20000)
    run_model_fixture_eval(R, "model_sun_eval.npz", args,
                           dict(enc_dropout=0.1, dec_dropout=0.1, mlp_dropout=0.3), cfg, batch,
                           stats_batch, synthetic.text_embedding(21, 640), seed=31)


def _scannet_full_batch(cfg, seed):
    B = 2
    batch = synthetic.make_batch(B, seed=seed, num_points=20000, use_color=True, dataset="scannet")
    batch["gt_box_angles"].zero_()
    batch["gt_angle_class_label"].zero_()
    batch["gt_angle_residual_label"].zero_()
    batch["gt_box_sem_cls_label"].clamp_(max=17)
    corners = cfg.box_parametrization_to_corners_np(batch["gt_box_centers"].numpy(),
                                                   batch["gt_box_sizes"].numpy(),
                                                   np.zeros((B, 64), np.float32))
    batch["gt_box_corners"] = torch.tensor(corners, dtype=torch.float32)
    return small_images(batch, B)


def gen_model_scannet_eval(R):
    import datasets.scannet as scannet
    cfg = scannet.ScannetDatasetConfig()
    args = model_args(enc_type="masked", use_color=True, enc_dim=256, enc_ffn_dim=128, dec_dim=256,
                      dec_ffn_dim=256, preenc_npoints=2048, nqueries=256, matcher_giou_cost=2.0,
                      matcher_center_cost=0.0, matcher_objectness_cost=0.0, loss_giou_weight=1.0,
                      loss_no_object_weight=0.25, loss_2dalignment_weight=0.0)
    run_model_fixture_eval(R, "model_scannet_eval.npz", args,
                           dict(enc_dropout=0.3, dec_dropout=0.1, mlp_dropout=0.3), cfg,
                           _scannet_full_batch(cfg, 23), _scannet_full_batch(cfg, EVAL_STATS_SEED),
                           synthetic.text_embedding(19, 640, seed=8), seed=37)


if __name__ == "__main__":
    torch.set_num_threads(8)
    R = load_reference()
    which = sys.argv[1:] or ["giou", "nms", "geometry", "model_sun", "model_scannet",
                             "model_sun_full", "model_scannet_full", "model_sun_eval",
                             "model_scannet_eval"]
    for w in which:
        globals()["gen_" + w](R)
    for f in sorted(os.listdir(HERE)):
        if f.endswith(".npz"):
            print(f, os.path.getsize(os.path.join(HERE, f)))
